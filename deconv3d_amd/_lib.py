# coding=utf-8
"""
ctypes binding of ``libdeconv3d_hip.so`` (C ABI: include/deconv3d_hip.h).

There is deliberately NO fallback: if the shared library is missing, or no HIP
device is visible when an :class:`Engine` is created, this raises.  The CPU
oracle under ``oracle/`` is test infrastructure and is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DECONV3D_HIP_LIB: another build of the same library (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("DECONV3D_HIP_LIB") or os.path.join(_HERE, "csrc", "libdeconv3d_hip.so")

# every symbol include/deconv3d_hip.h declares (tests check the export list)
SYMBOLS = [
    "d3d_version", "d3d_source_hash", "d3d_last_error", "d3d_device_count",
    "d3d_ctx_create", "d3d_ctx_destroy", "d3d_ctx_set_stream", "d3d_sync",
    "d3d_ctx_set_option", "d3d_ctx_get_option", "d3d_has_experiments",
    "d3d_timer_start", "d3d_timer_stop",
    "d3d_set_taps", "d3d_set_data", "d3d_set_params", "d3d_get_params", "d3d_set_line_shape", "d3d_set_line_table",
    "d3d_build_clean", "d3d_convolve", "d3d_forward", "d3d_simulate", "d3d_residual",
    "d3d_chi2_map", "d3d_upload_slot", "d3d_download_slot",
    "d3d_convolve_slots", "d3d_stage_upload", "d3d_stage_convolve", "d3d_stage_download",
    "d3d_mh_config", "d3d_mh_set_sweep_origin", "d3d_window_stats",
    "d3d_mh_sweeps", "d3d_mh_colour_lines", "d3d_get_dlog", "d3d_variance_is_uniform", "d3d_mh_layers",
    "d3d_colour_count", "d3d_rtnorm", "d3d_philox",
    "d3d_set_tile", "d3d_set_parts", "d3d_mh_phase", "d3d_mh_sweeps_batch", "d3d_mh_accepted", "d3d_flush",
    "d3d_halo_plan", "d3d_comm_unique_id", "d3d_comm_init", "d3d_comm_destroy", "d3d_comm_info",
    "d3d_halo_time",
    "d3d_halo_exchange", "d3d_halo_pack", "d3d_halo_unpack", "d3d_halo_buffers",
    "d3d_halo_download", "d3d_halo_upload", "d3d_device_copy",
    "d3d_mh_colour", "d3d_export_updates", "d3d_apply_updates",
    "d3d_post_begin", "d3d_post_schedule", "d3d_post_accumulate", "d3d_post_count", "d3d_post_get",
    "d3d_post_end",
    "d3d_hist_begin", "d3d_hist_count", "d3d_hist_get", "d3d_hist_quantiles", "d3d_hist_end",
    "d3d_region_begin", "d3d_region_count", "d3d_region_get", "d3d_region_end",
    "d3d_adapt_begin", "d3d_adapt_get", "d3d_adapt_set", "d3d_adapt_end",
    "d3d_prior_begin", "d3d_prior_get", "d3d_prior_end", "d3d_prior_energy",
    "d3d_line_search",
    "d3d_running_median", "d3d_channel_stats", "d3d_prepare",
    "d3d_temper_create", "d3d_temper_swap", "d3d_temper_get", "d3d_temper_last", "d3d_temper_destroy",
    "d3d_temper_set_patch", "d3d_temper_last_patches", "d3d_temper_get_patches",
    "d3d_robust_begin", "d3d_robust_step", "d3d_robust_get", "d3d_robust_end",
    "d3d_pred_begin", "d3d_pred_count", "d3d_pred_get", "d3d_pred_maps", "d3d_pred_cubes", "d3d_pred_end",
    "d3d_noise_begin", "d3d_noise_step", "d3d_noise_count", "d3d_noise_get", "d3d_noise_end",
]

# posterior moments (a table, so that tools/posterior_time.py can load the PARENT commit's library,
# which lacks them, for its A/B: it empties the table and drops the names from SYMBOLS first)
POST_PROTOTYPES = {
    "d3d_post_begin": [C.c_int],
    "d3d_post_schedule": [C.c_int, C.c_int],
    "d3d_post_accumulate": [],
    "d3d_post_count": [C.POINTER(C.c_int64)],
    "d3d_post_get": [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "d3d_post_end": [],
}
# posterior histograms (a table for the same reason: tools/hist_time.py loads the parent's library)
HIST_PROTOTYPES = {
    "d3d_hist_begin": [C.c_int64, C.c_double],
    "d3d_hist_count": [C.POINTER(C.c_int64)],
    "d3d_hist_get": [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)],
    "d3d_hist_quantiles": [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                           C.POINTER(C.c_double)],
    "d3d_hist_end": [],
}
# region posteriors (a table for the same reason: tools/region_time.py loads the parent's library)
REGION_PROTOTYPES = {
    "d3d_region_begin": [C.POINTER(C.c_int32), C.c_int, C.c_int64, C.c_int],
    "d3d_region_count": [C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "d3d_region_get": [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)],
    "d3d_region_end": [],
}
# per-spaxel jump scales (a table for the same reason: tools that load the parent's library)
ADAPT_PROTOTYPES = {
    "d3d_adapt_begin": [C.c_double, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double],
    "d3d_adapt_get": [C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int64),
                      C.POINTER(C.c_int64)],
    "d3d_adapt_set": [C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int64, C.c_int64],
    "d3d_adapt_end": [],
}
# smoothness prior between neighbouring spaxels (a table for the same reason)
PRIOR_PROTOTYPES = {
    "d3d_prior_begin": [C.POINTER(C.c_double)],
    "d3d_prior_get": [C.POINTER(C.c_double), C.POINTER(C.c_int)],
    "d3d_prior_end": [],
    "d3d_prior_energy": [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)],
}
# matched-filter line search (a table for the same reason)
SEARCH_PROTOTYPES = {
    "d3d_line_search": [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                        C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)],
}
# preparation of a raw cube (a table for the same reason)
PREP_PROTOTYPES = {
    "d3d_running_median": [C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_double)],
    "d3d_channel_stats": [C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_double),
                          C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    "d3d_prepare": [C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int, C.c_double,
                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
}
# replica exchange between tempered chains (a table for the same reason; the first argument is the
# group's handle, d3d_temper_create's the address it is returned through)
TEMPER_PROTOTYPES = {
    "d3d_temper_create": [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_double),
                          C.c_uint64],
    "d3d_temper_swap": [C.c_void_p, C.c_int64],
    "d3d_temper_get": [C.c_void_p] + [C.POINTER(C.c_int64)] * 4 + [C.POINTER(C.c_double)] * 2
                      + [C.POINTER(C.c_int32)],
    "d3d_temper_last": [C.c_void_p] + [C.POINTER(C.c_double)] * 3 + [C.POINTER(C.c_int32)],
    "d3d_temper_destroy": [C.c_void_p],
    "d3d_temper_set_patch": [C.c_void_p, C.c_int],
    "d3d_temper_last_patches": [C.c_void_p, C.POINTER(C.c_int32)] + [C.POINTER(C.c_double)] * 3
                               + [C.POINTER(C.c_int32)],
    "d3d_temper_get_patches": [C.c_void_p] + [C.POINTER(C.c_int64)] * 2,
}
# weights of a Student-t likelihood (a table for the same reason: tools/robust_time.py)
ROBUST_PROTOTYPES = {
    "d3d_robust_begin": [C.c_int, C.c_int, C.c_int64, C.c_int64],
    "d3d_robust_step": [C.c_int64],
    "d3d_robust_get": [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    "d3d_robust_end": [],
}
# pointwise predictive accuracy (a table for the same reason: tools/predictive_time.py)
PRED_PROTOTYPES = {
    "d3d_pred_begin": [],
    "d3d_pred_count": [C.POINTER(C.c_int64)],
    "d3d_pred_get": [C.POINTER(C.c_double)] * 4,
    "d3d_pred_maps": [C.POINTER(C.c_double)],
    "d3d_pred_cubes": [C.POINTER(C.c_double)] * 2,
    "d3d_pred_end": [],
}
# variance factors of channel groups (a table for the same reason: tools/noise_time.py)
NOISE_PROTOTYPES = {
    "d3d_noise_begin": [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint8), C.c_double, C.c_double, C.c_int,
                        C.c_int64, C.c_int64],
    "d3d_noise_step": [C.c_int64],
    "d3d_noise_count": [C.POINTER(C.c_int64)],
    "d3d_noise_get": [C.POINTER(C.c_double), C.POINTER(C.c_int64)] + [C.POINTER(C.c_double)] * 3,
    "d3d_noise_end": [],
}
POST_CLEAN, POST_CONVOLVED = 1, 2                   # d3d_post_begin: bits of `what`
POST_PARAMETERS, POST_CLEAN_CUBE, POST_CONVOLVED_CUBE = 0, 1, 2   # d3d_post_get: `which`
REGION_SPECTRA = 1                                    # d3d_region_begin: bit of `what`

PLAN_PARAMS = 16          # D3D_PLAN_PARAMS
COMM_UID_BYTES = 128      # D3D_COMM_UID_BYTES

SLOT_DATA, SLOT_IVAR, SLOT_ERR, SLOT_SIM, SLOT_TMP0, SLOT_TMP1 = range(6)

ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -4, -5

# read-only options spatial_path / spectral_path / stage_path: the kernel family the dispatcher took
# last (include/deconv3d_hip.h: D3D_SPATIAL_*, D3D_SPECTRAL_*, D3D_STAGE_*)
SPATIAL_CONV_ROWS, SPATIAL_CONV_ROWS_ZB, SPATIAL_CONV_ROWS_LSF = 1, 2, 3
SPATIAL_MARCH_XY, SPATIAL_MARCH_X, SPATIAL_MARCH = 10, 11, 12
SPATIAL_SEP, SPATIAL_SEP_LSF, SPATIAL_MARCH_EXPERIMENT = 13, 14, 15
SPATIAL_GENERIC, SPATIAL_DEEP = 30, 40
SPATIAL_TILE = 10000      # the tile kernel k_spatial<NT>: SPATIAL_TILE + NT
SPECTRAL_BLOCKS, SPECTRAL_DEEP, SPECTRAL_DENSE, SPECTRAL_TAPS, SPECTRAL_SHFL = 1, 2, 3, 4, 5
STAGE_ZMAJOR, STAGE_TRANSPOSE = 1, 2

# read-only options mh_path / mh_path_layers / mh_path_launches: what the dispatcher of the MH sweep
# launched (include/deconv3d_hip.h: D3D_MH_*).  mh_path_fields() takes the packed code apart.
MH_FAMILY_MASK = 0xf
(MH_WS, MH_SMALL, MH_SMALL_WIDE, MH_ZB, MH_BATCH_WS, MH_BATCH_SMALL, MH_DEFER, MH_IMMEDIATE, MH_DEEP,
 MH_FLOW, MH_PAIR, MH_CHAIN, MH_SMALL_FULL) = range(1, 14)
MH_U_SHIFT, MH_U_MASK = 4, 0xf
MH_M_SHIFT, MH_M_MASK = 8, 0x3
MH_K_SHIFT, MH_K_MASK = 10, 0x7
MH_NTV, MH_UV, MH_PRIOR, MH_MULTI = 1 << 13, 1 << 14, 1 << 15, 1 << 16
MH_NS_SHIFT, MH_NS_MASK = 17, 0x7ff
MH_FAMILY_NAMES = {MH_WS: "ws", MH_SMALL: "small", MH_SMALL_WIDE: "small wide", MH_ZB: "zb",
                   MH_BATCH_WS: "batch ws", MH_BATCH_SMALL: "batch small", MH_DEFER: "defer",
                   MH_IMMEDIATE: "immediate", MH_DEEP: "deep", MH_FLOW: "flow", MH_PAIR: "pair",
                   MH_CHAIN: "chain", MH_SMALL_FULL: "small full"}


def mh_path_fields(code):
    """The fields of a packed mh_path code: family (its name, None for 0: nothing launched), NS
    (streaming threads), U (window positions in flight), M (pending layers the kernel can apply), K
    (staging registers; U and K are 0 where the kernel has no such parameter) and the flags NTV, UV,
    prior and multi."""
    code = int(code)
    return {"family": MH_FAMILY_NAMES.get(code & MH_FAMILY_MASK),
            "NS": (code >> MH_NS_SHIFT) & MH_NS_MASK,
            "U": (code >> MH_U_SHIFT) & MH_U_MASK,
            "M": (code >> MH_M_SHIFT) & MH_M_MASK,
            "K": (code >> MH_K_SHIFT) & MH_K_MASK,
            "NTV": bool(code & MH_NTV), "UV": bool(code & MH_UV),
            "prior": bool(code & MH_PRIOR), "multi": bool(code & MH_MULTI)}


def mh_layers_seen(bits):
    """The pending-layer counts in an mh_path_layers word, as a sorted tuple."""
    return tuple(n for n in range(4) if (int(bits) >> n) & 1)


class HipLibraryMissing(ImportError):
    """libdeconv3d_hip.so has not been built (run __graft_entry__.build())."""


class HipError(RuntimeError):
    """A HIP runtime call failed, or no HIP device is available."""


_lib = None


def _dp(arr):
    return arr.ctypes.data_as(C.POINTER(C.c_double))


def load():
    """Load the shared library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). deconv3d_amd has no CPU "
            "fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    ctx_p = C.c_void_p
    dbl_p = C.POINTER(C.c_double)
    lib.d3d_version.restype = C.c_int
    lib.d3d_last_error.restype = C.c_char_p
    lib.d3d_source_hash.restype = C.c_char_p
    lib.d3d_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.d3d_ctx_create.argtypes = [C.POINTER(ctx_p)] + [C.c_int] * 6
    lib.d3d_ctx_destroy.argtypes = [ctx_p]
    lib.d3d_ctx_set_stream.argtypes = [ctx_p, C.c_void_p]
    lib.d3d_sync.argtypes = [ctx_p]
    lib.d3d_ctx_set_option.argtypes = [ctx_p, C.c_char_p, C.c_long]
    lib.d3d_ctx_get_option.argtypes = [ctx_p, C.c_char_p, C.POINTER(C.c_long)]
    lib.d3d_has_experiments.restype = C.c_int
    lib.d3d_timer_start.argtypes = [ctx_p]
    lib.d3d_timer_stop.argtypes = [ctx_p, dbl_p]
    lib.d3d_set_taps.argtypes = [ctx_p, dbl_p, dbl_p, C.c_double]
    lib.d3d_set_data.argtypes = [ctx_p, dbl_p, dbl_p, C.c_double,
                                 C.POINTER(C.c_uint8)]
    lib.d3d_set_params.argtypes = [ctx_p, dbl_p]
    lib.d3d_get_params.argtypes = [ctx_p, dbl_p]
    lib.d3d_set_line_shape.argtypes = [ctx_p, C.c_int, dbl_p, dbl_p]
    lib.d3d_set_line_table.argtypes = [ctx_p, C.c_int, C.c_double, dbl_p, C.c_double]
    lib.d3d_build_clean.argtypes = [ctx_p, dbl_p]
    lib.d3d_convolve.argtypes = [ctx_p, dbl_p, dbl_p]
    lib.d3d_forward.argtypes = [ctx_p, dbl_p]
    lib.d3d_residual.argtypes = [ctx_p, dbl_p]
    lib.d3d_simulate.argtypes = [ctx_p, dbl_p, C.c_int, dbl_p]
    lib.d3d_mh_set_sweep_origin.argtypes = [ctx_p, C.c_int64]
    lib.d3d_chi2_map.argtypes = [ctx_p, dbl_p, dbl_p]
    lib.d3d_upload_slot.argtypes = [ctx_p, C.c_int, dbl_p]
    lib.d3d_download_slot.argtypes = [ctx_p, C.c_int, dbl_p]
    lib.d3d_convolve_slots.argtypes = [ctx_p, C.c_int, C.c_int]
    lib.d3d_stage_upload.argtypes = [ctx_p, dbl_p]
    lib.d3d_stage_convolve.argtypes = [ctx_p]
    lib.d3d_stage_download.argtypes = [ctx_p, dbl_p]
    lib.d3d_mh_config.argtypes = [ctx_p, dbl_p, dbl_p, dbl_p, C.c_double,
                                  C.c_uint64, C.c_int]
    lib.d3d_window_stats.argtypes = [ctx_p, C.c_int, C.c_int, dbl_p, dbl_p]
    lib.d3d_mh_sweeps.argtypes = [ctx_p, C.c_int, C.c_int, C.c_int, dbl_p,
                                  dbl_p, C.POINTER(C.c_int64)]
    lib.d3d_get_dlog.argtypes = [ctx_p, dbl_p]
    lib.d3d_variance_is_uniform.argtypes = [ctx_p, C.POINTER(C.c_int)]
    lib.d3d_mh_layers.argtypes = [ctx_p, C.POINTER(C.c_int)]
    lib.d3d_mh_colour_lines.argtypes = [ctx_p, C.c_int, C.c_int, C.POINTER(C.c_int), dbl_p,
                                        dbl_p, C.c_int, dbl_p]
    lib.d3d_colour_count.argtypes = [ctx_p, C.c_int, C.POINTER(C.c_int)]
    lib.d3d_rtnorm.argtypes = [ctx_p, C.c_long] + [C.c_double] * 4 + [C.c_uint64, C.c_int, dbl_p]
    u32_p = C.POINTER(C.c_uint32)
    lib.d3d_philox.argtypes = [ctx_p, C.c_long, u32_p, u32_p, u32_p, dbl_p]
    lib.d3d_set_tile.argtypes = [ctx_p] + [C.c_int] * 7
    int_p = C.POINTER(C.c_int)
    lib.d3d_set_parts.argtypes = [ctx_p, C.c_int, int_p, int_p]
    lib.d3d_mh_phase.argtypes = [ctx_p, C.c_int, C.c_int]
    lib.d3d_mh_sweeps_batch.argtypes = [C.POINTER(ctx_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.d3d_mh_accepted.argtypes = [ctx_p, C.POINTER(C.c_int64), C.c_int]
    lib.d3d_flush.argtypes = [ctx_p]
    lib.d3d_halo_plan.argtypes = [ctx_p, C.c_int, C.c_int, int_p]
    lib.d3d_comm_unique_id.argtypes = [C.c_void_p]
    lib.d3d_comm_init.argtypes = [ctx_p, C.c_int, C.c_int, C.c_void_p]
    lib.d3d_comm_destroy.argtypes = [ctx_p]
    lib.d3d_comm_info.argtypes = [ctx_p, int_p, int_p]
    lib.d3d_halo_time.argtypes = [ctx_p, dbl_p, C.POINTER(C.c_long), C.c_int]
    lib.d3d_halo_exchange.argtypes = [ctx_p, C.c_int]
    lib.d3d_halo_pack.argtypes = [ctx_p, C.c_int]
    lib.d3d_halo_unpack.argtypes = [ctx_p, C.c_int]
    lib.d3d_halo_buffers.argtypes = [ctx_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_size_t)]
    lib.d3d_halo_download.argtypes = [ctx_p, C.c_int, C.c_int, dbl_p]
    lib.d3d_halo_upload.argtypes = [ctx_p, C.c_int, C.c_int, dbl_p]
    lib.d3d_device_copy.argtypes = [ctx_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.d3d_mh_colour.argtypes = [ctx_p, C.c_int, C.c_int]
    lib.d3d_export_updates.argtypes = [ctx_p, C.c_int, C.POINTER(C.c_int), dbl_p]
    lib.d3d_apply_updates.argtypes = [ctx_p, C.c_int, dbl_p]
    for name, argtypes in (list(POST_PROTOTYPES.items()) + list(ADAPT_PROTOTYPES.items())
                           + list(SEARCH_PROTOTYPES.items()) + list(PREP_PROTOTYPES.items())
                           + list(PRIOR_PROTOTYPES.items()) + list(HIST_PROTOTYPES.items())
                           + list(REGION_PROTOTYPES.items()) + list(ROBUST_PROTOTYPES.items())
                           + list(PRED_PROTOTYPES.items()) + list(NOISE_PROTOTYPES.items())):
        getattr(lib, name).argtypes = [ctx_p] + argtypes
    for name, argtypes in TEMPER_PROTOTYPES.items():
        getattr(lib, name).argtypes = argtypes
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("d3d_version", "d3d_last_error", "d3d_source_hash", "d3d_has_experiments"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def source_hash():
    """Hash of the sources the loaded binary was compiled from (csrc/Makefile)."""
    return load().d3d_source_hash().decode("ascii", "replace")


def has_experiments():
    """True when the library was built with `make EXPERIMENTS=1`."""
    return bool(load().d3d_has_experiments())


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (rank 0 draws it, every rank
    passes it to Engine.comm_init)."""
    buf = C.create_string_buffer(COMM_UID_BYTES)
    _check(load().d3d_comm_unique_id(C.cast(buf, C.c_void_p)))
    return buf.raw


def mh_sweeps_batch(engines, n_sweeps, first_sweep=1, keep_one_in=1, chains=None, dlogs=None):
    """d3d_mh_sweeps_batch: the chains of several Engines of one geometry, one launch per colour
    class for all of them.  chains / dlogs: per-engine host arrays as Engine.mh_sweeps takes
    them (or None; a None entry skips that engine).  Returns the accepted counts."""
    lib = load()
    n = len(engines)
    last = (first_sweep + n_sweeps - 1) // keep_one_in

    def pointers(arrs, tail):
        if arrs is None:
            return None
        if len(arrs) != n:
            raise ValueError("one array (or None) per engine")
        out = (C.c_void_p * n)()
        for i, (a, e) in enumerate(zip(arrs, engines)):
            if a is None:
                continue
            H, W = e.shape[1:]
            if (a.dtype != np.float64 or not a.flags.c_contiguous or a.shape[1:] != (H, W) + tail
                    or a.shape[0] <= last):
                raise ValueError("chain / dlog array %d: float64, C-contiguous, (>%d, %d, %d%s)"
                                 % (i, last, H, W, ", 3" if tail else ""))
            out[i] = a.ctypes.data
        return out

    arr = (C.c_void_p * n)(*[e._ctx.value for e in engines])
    acc = (C.c_int64 * n)()
    _check(lib.d3d_mh_sweeps_batch(arr, n, int(n_sweeps), int(first_sweep), int(keep_one_in),
                                   pointers(chains, (3,)), pointers(dlogs, ()), acc))
    return [int(v) for v in acc]


class TemperGroup(object):
    """d3d_temper_*: replica exchange between the chains of ``engines`` -- one geometry, rung r
    fed ``var / betas[r]`` by its owner -- at inverse temperatures ``betas`` (1 first, strictly
    decreasing).  ``seed`` keys the swaps' uniforms.  ``patch``: None (whole cubes trade places) or
    the side p >= 1 of the tiles whose spaxels do (d3d_temper_set_patch).  Close the group before its
    engines."""

    def __init__(self, engines, betas, seed=12345, patch=None):
        self._lib = load()
        self._t = C.c_void_p(None)
        self.engines = list(engines)          # (kept alive: the group holds their contexts)
        self.n = len(self.engines)
        self.betas = np.ascontiguousarray(betas, dtype=np.float64)
        if self.betas.ndim != 1 or self.betas.shape[0] != self.n:
            raise ValueError("one beta per engine: %d engine(s), betas of shape %s"
                             % (self.n, self.betas.shape))
        arr = (C.c_void_p * max(self.n, 1))(*[e._ctx.value for e in self.engines])
        _check(self._lib.d3d_temper_create(C.byref(self._t), arr, self.n, _dp(self.betas),
                                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)))
        self.patch = None
        if patch is not None:
            self.set_patch(patch)

    def set_patch(self, patch):
        """d3d_temper_set_patch: None or 0 for whole cubes, p >= 1 for tiles of p x p spaxels."""
        p = 0 if patch is None else int(patch)
        _check(self._lib.d3d_temper_set_patch(self._t, p))
        self.patch = p if p > 0 else None

    def close(self):
        if getattr(self, "_t", None) is not None and self._t.value:
            self._lib.d3d_temper_destroy(self._t)
            self._t = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def swap(self, round):
        """One exchange round (asynchronous): the pairs (i, i + 1) with i of ``round``'s parity."""
        _check(self._lib.d3d_temper_swap(self._t, int(round)))

    def get(self):
        """dict(rounds, attempts, accepts (n-1), energy_n, energy_mean, energy_m2, labels (n))."""
        n = self.n
        rounds = C.c_int64(0)
        attempts, accepts = np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=np.int64)
        e_n, labels = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        mean, m2 = np.zeros(n), np.zeros(n)
        i64 = C.POINTER(C.c_int64)
        _check(self._lib.d3d_temper_get(self._t, C.byref(rounds), attempts.ctypes.data_as(i64),
                                        accepts.ctypes.data_as(i64), e_n.ctypes.data_as(i64), _dp(mean),
                                        _dp(m2), labels.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(rounds=int(rounds.value), attempts=attempts, accepts=accepts, energy_n=e_n,
                    energy_mean=mean, energy_m2=m2, labels=labels)

    def last(self):
        """The last round: dict(energy (n), u, logu (n-1, NaN where not proposed), decided (n-1:
        1 accepted, 0 rejected, -1 not proposed))."""
        n = self.n
        energy, u, logu = np.zeros(n), np.zeros(n - 1), np.zeros(n - 1)
        decided = np.zeros(n - 1, dtype=np.int32)
        _check(self._lib.d3d_temper_last(self._t, _dp(energy), _dp(u), _dp(logu),
                                         decided.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(energy=energy, u=u, logu=logu, decided=decided)

    def last_patches(self):
        """The last round, a patch round: dict(oy, ox, nty, ntx, my, mx, terms (n-1, nty, ntx, 5: sum
        ivar_i e_i delta, sum ivar_j e_j delta, 1/2 sum ivar_i delta^2, 1/2 sum ivar_j delta^2, the
        prior's term), u, logu (n-1, nty, ntx; NaN where not proposed), decided (n-1, nty, ntx: 1, 0,
        -1 = not proposed))."""
        geom = np.zeros(6, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        _check(self._lib.d3d_temper_last_patches(self._t, geom.ctypes.data_as(i32), None, None, None, None))
        oy, ox, nty, ntx, my, mx = (int(v) for v in geom)
        shape = (self.n - 1, nty, ntx)
        terms, u, logu = np.zeros(shape + (5,)), np.zeros(shape), np.zeros(shape)
        decided = np.zeros(shape, dtype=np.int32)
        _check(self._lib.d3d_temper_last_patches(self._t, None, _dp(terms), _dp(u), _dp(logu),
                                                 decided.ctypes.data_as(i32)))
        return dict(oy=oy, ox=ox, nty=nty, ntx=ntx, my=my, mx=mx, terms=terms, u=u, logu=logu, decided=decided)

    def get_patches(self):
        """dict(attempts, accepts (n-1)): the patches proposed and accepted per pair so far."""
        attempts, accepts = np.zeros(self.n - 1, dtype=np.int64), np.zeros(self.n - 1, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _check(self._lib.d3d_temper_get_patches(self._t, attempts.ctypes.data_as(i64), accepts.ctypes.data_as(i64)))
        return dict(attempts=attempts, accepts=accepts)


def device_count():
    lib = load()
    n = C.c_int(0)
    lib.d3d_device_count(C.byref(n))
    return n.value


def _check(rc):
    if rc == 0:
        return
    msg = load().d3d_last_error().decode("utf-8", "replace")
    if rc == ERR_INVALID:
        raise ValueError(msg)
    if rc == ERR_STATE:
        raise RuntimeError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise HipError(msg)


def _c64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a


class Engine(object):
    """
    One device context: cube shape ``(D, H, W)``, FSF shape ``(fh, fw)``.
    Thin, typed mirror of the C ABI; arrays in the reference's layouts.
    """

    def __init__(self, shape, fsf_shape, device=0, options=None):
        """options: {key: int} passed to :meth:`set_option` (d3d_ctx_set_option) right
        after the context exists -- per-context, unlike the D3D_<KEY> environment
        defaults."""
        self._lib = load()
        self._ctx = C.c_void_p(None)
        D, H, W = [int(v) for v in shape]
        fh, fw = [int(v) for v in fsf_shape]
        self.shape = (D, H, W)
        self.fsf_shape = (fh, fw)
        _check(self._lib.d3d_ctx_create(C.byref(self._ctx), int(device),
                                        D, H, W, fh, fw))
        for key, value in (options or {}).items():
            self.set_option(key, value)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.d3d_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- plumbing ---------------------------------------------------------
    def set_option(self, key, value):
        """Per-context kernel selection switch (include/deconv3d_hip.h: d3d_ctx_set_option)."""
        _check(self._lib.d3d_ctx_set_option(self._ctx, str(key).encode("ascii"), int(value)))

    def get_option(self, key):
        v = C.c_long(0)
        _check(self._lib.d3d_ctx_get_option(self._ctx, str(key).encode("ascii"), C.byref(v)))
        return v.value

    def set_stream(self, stream_handle):
        _check(self._lib.d3d_ctx_set_stream(self._ctx, C.c_void_p(stream_handle)))

    def sync(self):
        _check(self._lib.d3d_sync(self._ctx))

    def timer_start(self):
        _check(self._lib.d3d_timer_start(self._ctx))

    def timer_stop(self):
        ms = C.c_double(0.)
        _check(self._lib.d3d_timer_stop(self._ctx, C.byref(ms)))
        return ms.value

    # -- inputs -----------------------------------------------------------
    def set_taps(self, fsf, lsf, lsf_rel_threshold=-1e-16):
        """lsf_rel_threshold < 0: taps are dropped within that error bound of sum|lsf|
        (include/deconv3d_hip.h); >= 0: relative to the largest tap."""
        fsf = _c64(fsf, self.fsf_shape)
        lsf_p = None
        if lsf is not None:
            lsf = _c64(lsf, (self.shape[0],))
            lsf_p = _dp(lsf)
        _check(self._lib.d3d_set_taps(self._ctx, _dp(fsf), lsf_p,
                                      float(lsf_rel_threshold)))

    def set_data(self, data, var=None, var_scalar=1.0, mask=None):
        data = _c64(data, self.shape)
        var_p = None
        if var is not None:
            var = _c64(var, self.shape)
            var_p = _dp(var)
        mask_p = None
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) == 1, dtype=np.uint8)
            if mask.shape != self.shape[1:]:
                raise ValueError("mask shape %s != %s" % (mask.shape, self.shape[1:]))
            mask_p = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        _check(self._lib.d3d_set_data(self._ctx, _dp(data), var_p,
                                      float(var_scalar), mask_p))

    def set_params(self, params):
        params = _c64(params, self.shape[1:] + (3,))
        _check(self._lib.d3d_set_params(self._ctx, _dp(params)))

    def set_line_shape(self, offsets, ratios):
        """Unit line of the kernels (include/deconv3d_hip.h: d3d_set_line_shape): 1 to 4
        Gaussians at channel ``offsets`` from the centre with flux ``ratios`` relative to the
        first (offsets[0] == 0, ratios[0] == 1).  Default: one Gaussian, ([0], [1])."""
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        rat = np.ascontiguousarray(ratios, dtype=np.float64).reshape(-1)
        if off.size != rat.size:
            raise ValueError("line shape: %d offsets but %d ratios" % (off.size, rat.size))
        if off.size == 0:
            raise ValueError("a line shape has 1 to 4 components, got 0")
        _check(self._lib.d3d_set_line_shape(self._ctx, int(off.size), _dp(off), _dp(rat)))

    def set_line_table(self, table, support=0., flux_factor=0.):
        """Tabulated profile of the unit line (include/deconv3d_hip.h: d3d_set_line_table):
        ``table`` holds 8 to 65537 samples of phi on the uniform grid over
        ``[-support, support]``, the sample of largest magnitude equal to 1; ``flux_factor`` is
        the integral of phi.  ``table=None`` (or empty) returns the context to Gaussians."""
        if table is None:
            tab = np.zeros(0)
        else:
            tab = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        _check(self._lib.d3d_set_line_table(self._ctx, int(tab.size), float(support),
                                            _dp(tab) if tab.size else None, float(flux_factor)))

    def get_params(self):
        out = np.empty(self.shape[1:] + (3,), dtype=np.float64)
        _check(self._lib.d3d_get_params(self._ctx, _dp(out)))
        return out

    # -- forward model ----------------------------------------------------
    def build_clean(self):
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_build_clean(self._ctx, _dp(out)))
        return out

    def convolve(self, cube):
        cube = _c64(cube, self.shape)
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_convolve(self._ctx, _dp(cube), _dp(out)))
        return out

    def forward(self, fetch=True):
        out = np.empty(self.shape, dtype=np.float64) if fetch else None
        _check(self._lib.d3d_forward(self._ctx, _dp(out) if fetch else None))
        return out

    def simulate(self, params, convolved=True):
        """simulate_clean / simulate_convolved of an explicit parameter map; the
        chain state on the device is left alone."""
        params = _c64(params, self.shape[1:] + (3,))
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_simulate(self._ctx, _dp(params), 1 if convolved else 0, _dp(out)))
        return out

    def residual(self, fetch=True):
        out = np.empty(self.shape, dtype=np.float64) if fetch else None
        _check(self._lib.d3d_residual(self._ctx, _dp(out) if fetch else None))
        return out

    def chi2_map(self, fetch=True):
        if not fetch:                       # device only, no wait (timing)
            _check(self._lib.d3d_chi2_map(self._ctx, None, None))
            return None
        out = np.empty(self.shape[1:], dtype=np.float64)
        tot = C.c_double(0.)
        _check(self._lib.d3d_chi2_map(self._ctx, _dp(out), C.byref(tot)))
        return out, tot.value

    def upload_slot(self, slot, cube):
        cube = _c64(cube, self.shape)
        _check(self._lib.d3d_upload_slot(self._ctx, int(slot), _dp(cube)))

    def download_slot(self, slot):
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_download_slot(self._ctx, int(slot), _dp(out)))
        return out

    def convolve_slots(self, src, dst):
        _check(self._lib.d3d_convolve_slots(self._ctx, int(src), int(dst)))

    def stage_upload(self, cube):
        cube = _c64(cube, self.shape)
        _check(self._lib.d3d_stage_upload(self._ctx, _dp(cube)))

    def stage_convolve(self):
        _check(self._lib.d3d_stage_convolve(self._ctx))

    def stage_download(self):
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_stage_download(self._ctx, _dp(out)))
        return out

    # -- MH within Gibbs --------------------------------------------------
    def mh_config(self, min_b, max_b, jump_amp, gibbs_apriori_variance, seed=12345,
                  refresh_every=1000):
        mn = _c64(min_b, (3,))
        mx = _c64(max_b, (3,))
        amp = _c64(np.ones(3) * np.asarray(jump_amp, dtype=np.float64), (3,))
        _check(self._lib.d3d_mh_config(self._ctx, _dp(mn), _dp(mx), _dp(amp),
                                       float(gibbs_apriori_variance),
                                       C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                       int(refresh_every)))

    def set_sweep_origin(self, origin):
        _check(self._lib.d3d_mh_set_sweep_origin(self._ctx, int(origin)))

    def window_stats(self, y, x, p_new):
        p = _c64(p_new, (3,))
        out = np.empty(5, dtype=np.float64)
        _check(self._lib.d3d_window_stats(self._ctx, int(y), int(x), _dp(p), _dp(out)))
        return out

    def mh_sweeps(self, n_sweeps, first_sweep, keep_one_in=1, chain=None, dlog=None):
        """Returns the number of accepted MH proposals."""
        H, W = self.shape[1:]
        chain_p = None
        dlog_p = None
        last = (first_sweep + n_sweeps - 1) // keep_one_in
        if chain is not None:
            if (chain.dtype != np.float64 or not chain.flags.c_contiguous
                    or chain.shape[1:] != (H, W, 3) or chain.shape[0] <= last):
                raise ValueError("chain must be C-contiguous float64 (n>%d,%d,%d,3)"
                                 % (last, H, W))
            chain_p = _dp(chain)
        if dlog is not None:
            if (dlog.dtype != np.float64 or not dlog.flags.c_contiguous
                    or dlog.shape[1:] != (H, W) or dlog.shape[0] <= last):
                raise ValueError("dlog must be C-contiguous float64 (n>%d,%d,%d)"
                                 % (last, H, W))
            dlog_p = _dp(dlog)
        acc = C.c_int64(0)
        _check(self._lib.d3d_mh_sweeps(self._ctx, int(n_sweeps), int(first_sweep),
                                       int(keep_one_in), chain_p, dlog_p,
                                       C.byref(acc)))
        return acc.value

    def mh_colour_lines(self, sweep, spaxels, in3, lines, gibbs=True):
        """One colour class with host-evaluated unit lines (custom LineModel).
        spaxels [n] local indices, in3 [n,3] = (amplitude, oob, log u),
        lines [n,2,D] = (current, proposed).  Returns [n,3] = (accepted,
        amplitude, delta)."""
        spaxels = np.ascontiguousarray(spaxels, dtype=np.int32)
        n = spaxels.shape[0]
        in3 = _c64(in3, (n, 3))
        lines = _c64(lines, (n, 2, self.shape[0]))
        out = np.empty((n, 3), dtype=np.float64)
        if n:
            _check(self._lib.d3d_mh_colour_lines(
                self._ctx, int(sweep), n, spaxels.ctypes.data_as(C.POINTER(C.c_int)),
                _dp(in3), _dp(lines), 1 if gibbs else 0, _dp(out)))
        return out

    def get_dlog(self):
        out = np.empty(self.shape[1:], dtype=np.float64)
        _check(self._lib.d3d_get_dlog(self._ctx, _dp(out)))
        return out

    def variance_is_uniform(self):
        flag = C.c_int(0)
        _check(self._lib.d3d_variance_is_uniform(self._ctx, C.byref(flag)))
        return bool(flag.value)

    def mh_layers(self):
        n = C.c_int(0)
        _check(self._lib.d3d_mh_layers(self._ctx, C.byref(n)))
        return n.value

    def colour_count(self, colour):
        n = C.c_int(0)
        _check(self._lib.d3d_colour_count(self._ctx, int(colour), C.byref(n)))
        return n.value

    def rtnorm(self, lo, hi, mu=0., sigma=1., size=1, seed=12345, wave_mode=False):
        """`size` draws of N(mu, sigma^2) truncated to [lo, hi] on the device:
        drop-in for rtnorm(a, b, mu, sigma, size) of lib/rtnorm.py:21-92."""
        out = np.empty(int(size), dtype=np.float64)
        _check(self._lib.d3d_rtnorm(self._ctx, int(size), float(lo), float(hi), float(mu),
                                    float(sigma), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                    1 if wave_mode else 0, _dp(out)))
        return out

    def philox(self, counters, keys):
        """Test hook (d3d_philox): the device's Philox4x32-10 and its uniforms for
        ``counters`` (n,4) and ``keys`` (n,2), uint32.  Returns (words (n,4) uint32,
        pairs (n,2) float64)."""
        counters = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
        keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
        n = counters.shape[0]
        if keys.shape[0] != n:
            raise ValueError("one key per counter: %d counters, %d keys" % (n, keys.shape[0]))
        words = np.empty((n, 4), dtype=np.uint32)
        pairs = np.empty((n, 2), dtype=np.float64)
        u32 = C.POINTER(C.c_uint32)
        if n:
            _check(self._lib.d3d_philox(self._ctx, n, counters.ctypes.data_as(u32),
                                        keys.ctypes.data_as(u32), words.ctypes.data_as(u32),
                                        _dp(pairs)))
        return words, pairs

    # -- spatial tiling (deconv3d_amd/tiling.py) ----------------------------
    def set_tile(self, gy0, gx0, Wg, oy0, oy1, ox0, ox1):
        _check(self._lib.d3d_set_tile(self._ctx, int(gy0), int(gx0), int(Wg), int(oy0),
                                      int(oy1), int(ox0), int(ox1)))

    def set_parts(self, rects, phases):
        """rects [n,4] = (y0, y1, x0, x1) local, phases [n]."""
        rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
        phases = np.ascontiguousarray(phases, dtype=np.int32).reshape(-1)
        if rects.shape[0] != phases.shape[0]:
            raise ValueError("one phase per part")
        ip = C.POINTER(C.c_int)
        _check(self._lib.d3d_set_parts(self._ctx, rects.shape[0], rects.ctypes.data_as(ip),
                                       phases.ctypes.data_as(ip)))

    def mh_phase(self, phase, sweep):
        _check(self._lib.d3d_mh_phase(self._ctx, int(phase), int(sweep)))

    def mh_accepted(self, reset=False):
        n = C.c_int64(0)
        _check(self._lib.d3d_mh_accepted(self._ctx, C.byref(n), 1 if reset else 0))
        return n.value

    def flush(self):
        _check(self._lib.d3d_flush(self._ctx))

    def halo_plan(self, plan, entries):
        """entries [n,10] = (peer, kind, send y0,y1,x0,x1, recv y0,y1,x0,x1), local."""
        entries = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1, 10)
        _check(self._lib.d3d_halo_plan(self._ctx, int(plan), entries.shape[0],
                                       entries.ctypes.data_as(C.POINTER(C.c_int))))

    def comm_init(self, nranks, rank, uid):
        if len(uid) != COMM_UID_BYTES:
            raise ValueError("uid must be %d bytes" % COMM_UID_BYTES)
        buf = C.create_string_buffer(bytes(uid), COMM_UID_BYTES)
        _check(self._lib.d3d_comm_init(self._ctx, int(nranks), int(rank), C.cast(buf, C.c_void_p)))

    def comm_destroy(self):
        _check(self._lib.d3d_comm_destroy(self._ctx))

    def comm_info(self):
        """(ranks RCCL says joined the communicator, this rank as RCCL numbers it)."""
        n, r = C.c_int(0), C.c_int(0)
        _check(self._lib.d3d_comm_info(self._ctx, C.byref(n), C.byref(r)))
        return n.value, r.value

    def halo_time(self, reset=False):
        """(milliseconds, exchanges) of the halo exchanges d3d_mh_sweeps ran since the last
        reset (needs option halo_timing = 1)."""
        ms, n = C.c_double(0.), C.c_long(0)
        _check(self._lib.d3d_halo_time(self._ctx, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def halo_exchange(self, plan):
        _check(self._lib.d3d_halo_exchange(self._ctx, int(plan)))

    def halo_pack(self, plan):
        _check(self._lib.d3d_halo_pack(self._ctx, int(plan)))

    def halo_unpack(self, plan):
        _check(self._lib.d3d_halo_unpack(self._ctx, int(plan)))

    def halo_buffers(self, plan, entry):
        """(send pointer, send bytes, receive pointer, receive bytes) of one entry."""
        sp, rp = C.c_void_p(None), C.c_void_p(None)
        sb, rb = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.d3d_halo_buffers(self._ctx, int(plan), int(entry), C.byref(sp),
                                          C.byref(sb), C.byref(rp), C.byref(rb)))
        return sp.value, sb.value, rp.value, rb.value

    def halo_download(self, plan, entry):
        _, nbytes, _, _ = self.halo_buffers(plan, entry)
        out = np.empty(nbytes // 8, dtype=np.float64)
        _check(self._lib.d3d_halo_download(self._ctx, int(plan), int(entry), _dp(out)))
        return out

    def halo_upload(self, plan, entry, values):
        _, _, _, nbytes = self.halo_buffers(plan, entry)
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if values.shape[0] * 8 != nbytes:
            raise ValueError("entry expects %d doubles, got %d" % (nbytes // 8, values.shape[0]))
        _check(self._lib.d3d_halo_upload(self._ctx, int(plan), int(entry), _dp(values)))

    def device_copy(self, dst, src, nbytes):
        _check(self._lib.d3d_device_copy(self._ctx, C.c_void_p(dst), C.c_void_p(src),
                                         C.c_size_t(nbytes)))

    def mh_colour(self, colour, sweep):
        _check(self._lib.d3d_mh_colour(self._ctx, int(colour), int(sweep)))

    def export_updates(self, spaxels):
        """[n,8] records {global y, global x, a,c,w before, a,c,w after} of the
        last update of the given local spaxel indices (y*W+x)."""
        spaxels = np.ascontiguousarray(spaxels, dtype=np.int32)
        out = np.empty((spaxels.shape[0], 8), dtype=np.float64)
        if spaxels.shape[0]:
            _check(self._lib.d3d_export_updates(
                self._ctx, spaxels.shape[0],
                spaxels.ctypes.data_as(C.POINTER(C.c_int)), _dp(out)))
        return out

    def apply_updates(self, records):
        """Replay records whose first two columns are LOCAL coordinates."""
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 8)
        if records.shape[0]:
            _check(self._lib.d3d_apply_updates(self._ctx, records.shape[0], _dp(records)))

    # -- posterior moments ------------------------------------------------------
    def post_begin(self, what=POST_CLEAN | POST_CONVOLVED):
        """Allocate and zero the running moments (include/deconv3d_hip.h: d3d_post_begin):
        the (a, c, w, F) map always, ``what`` bit 0 the clean cube, bit 1 the convolved cube."""
        _check(self._lib.d3d_post_begin(self._ctx, int(what)))

    def post_schedule(self, first_sweep, every=1):
        """mh_sweeps / mh_sweeps_batch take the state after the sweeps first_sweep,
        first_sweep + every, ... as samples."""
        _check(self._lib.d3d_post_schedule(self._ctx, int(first_sweep), int(every)))

    def post_accumulate(self):
        """The current parameters as one more sample."""
        _check(self._lib.d3d_post_accumulate(self._ctx))

    def post_count(self):
        n = C.c_int64(0)
        _check(self._lib.d3d_post_count(self._ctx, C.byref(n)))
        return n.value

    def post_get(self, which):
        """(mean, M2) of the parameter map (which = 0: (H,W,4), columns a, c, w, F), the clean
        cube (1) or the convolved cube (2: (D,H,W)); variance = M2 / (count - 1)."""
        shape = self.shape[1:] + (4,) if int(which) == POST_PARAMETERS else self.shape
        mean = np.empty(shape, dtype=np.float64)
        m2 = np.empty(shape, dtype=np.float64)
        _check(self._lib.d3d_post_get(self._ctx, int(which), _dp(mean), _dp(m2)))
        return mean, m2

    def post_end(self):
        _check(self._lib.d3d_post_end(self._ctx))

    # -- posterior histograms -----------------------------------------------------
    def hist_begin(self, pilot=200, span=6.0):
        """Allocate the per-spaxel histograms of (a, c, w, F) (include/deconv3d_hip.h:
        d3d_hist_begin) and start the moments afresh: their first ``pilot`` samples freeze every
        range at mean +- ``span`` standard deviations (clipped to the bounds of mh_config), every
        later sample is binned.  Needs post_begin and mh_config."""
        _check(self._lib.d3d_hist_begin(self._ctx, int(pilot), float(span)))

    def hist_count(self):
        n = C.c_int64(0)
        _check(self._lib.d3d_hist_count(self._ctx, C.byref(n)))
        return n.value

    def hist_get(self):
        """(bins (H,W,4,64) uint32, tails (H,W,4,2) uint32 = below | above, range (H,W,4,2) = lo | hi)."""
        hw4 = self.shape[1:] + (4,)
        bins = np.empty(hw4 + (64,), dtype=np.uint32)
        tails = np.empty(hw4 + (2,), dtype=np.uint32)
        rng = np.empty(hw4 + (2,), dtype=np.float64)
        u32 = C.POINTER(C.c_uint32)
        _check(self._lib.d3d_hist_get(self._ctx, bins.ctypes.data_as(u32), tails.ctypes.data_as(u32), _dp(rng)))
        return bins, tails, rng

    def hist_quantiles(self, qs):
        """(quantiles (H,W,4,len(qs)), mode (H,W,4), outside (H,W,4)) extracted on the device; 1 to 8
        ``qs`` inside (0, 1)."""
        q = np.ascontiguousarray(qs, dtype=np.float64).reshape(-1)
        hw4 = self.shape[1:] + (4,)
        quant = np.empty(hw4 + (max(q.size, 1),), dtype=np.float64)
        mode = np.empty(hw4, dtype=np.float64)
        outside = np.empty(hw4, dtype=np.float64)
        _check(self._lib.d3d_hist_quantiles(self._ctx, int(q.size), _dp(q), _dp(quant), _dp(mode), _dp(outside)))
        return quant, mode, outside

    def hist_end(self):
        _check(self._lib.d3d_hist_end(self._ctx))

    # -- region posteriors ----------------------------------------------------------
    def region_begin(self, labels, K=None, capacity=0, spectra=True):
        """Lay out the regions 1 .. ``K`` (default: the largest label) of the int32 (H, W) map
        ``labels`` (0: no region), allocate a series of ``capacity`` samples of their (F, C, S) and,
        with ``spectra``, their summed clean spectra's moments (include/deconv3d_hip.h:
        d3d_region_begin), and start the moments afresh.  Needs post_begin."""
        labels = np.asarray(labels)
        if labels.shape != self.shape[1:] or labels.dtype.kind not in "iu":
            raise ValueError("labels: an integer array of shape %s, got %s of %s"
                             % (self.shape[1:], labels.dtype, labels.shape))
        if labels.size and (labels.min() < -2 ** 31 or labels.max() >= 2 ** 31):
            raise ValueError("labels: beyond int32")
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        K = int(lab.max()) if K is None else int(K)
        _check(self._lib.d3d_region_begin(self._ctx, lab.ctypes.data_as(C.POINTER(C.c_int32)), K, int(capacity),
                                          REGION_SPECTRA if spectra else 0))
        self._region = (K, bool(spectra))

    def region_count(self):
        """(samples taken, rows of the series): the second stops at the capacity."""
        n, stored = C.c_int64(0), C.c_int64(0)
        _check(self._lib.d3d_region_count(self._ctx, C.byref(n), C.byref(stored)))
        return n.value, stored.value

    def region_get(self):
        """(series (stored, K, 3) = F | C | S, spectrum mean (K, D), spectrum M2 (K, D), sizes (K));
        the spectra are None when they were not begun."""
        K, spectra = getattr(self, "_region", None) or (0, False)
        stored = self.region_count()[1]
        series = np.empty((stored, K, 3), dtype=np.float64)
        mean = np.empty((K, self.shape[0]), dtype=np.float64) if spectra else None
        m2 = np.empty((K, self.shape[0]), dtype=np.float64) if spectra else None
        sizes = np.empty(K, dtype=np.int32)
        _check(self._lib.d3d_region_get(self._ctx, _dp(series), _dp(mean) if spectra else None,
                                        _dp(m2) if spectra else None, sizes.ctypes.data_as(C.POINTER(C.c_int32))))
        return series, mean, m2, sizes

    def region_end(self):
        _check(self._lib.d3d_region_end(self._ctx))
        self._region = None

    # -- per-spaxel jump scales ---------------------------------------------------
    def adapt_begin(self, target=0.25, window=50, last_sweep=0, gain=2.0, scale_range=(1e-3, 1e3)):
        """Allocate the (H,W) jump scale map (all 1) and accept counters (include/deconv3d_hip.h:
        d3d_adapt_begin): every ``window`` sweeps up to sweep ``last_sweep`` each spaxel's scale
        moves towards the acceptance rate ``target``; ``window = 0`` keeps a fixed map."""
        _check(self._lib.d3d_adapt_begin(self._ctx, float(target), int(window), int(last_sweep),
                                         float(gain), float(scale_range[0]), float(scale_range[1])))

    def adapt_get(self):
        """(scale map, accepted counters, sweeps counted since they were cleared, steps taken)."""
        scale = np.empty(self.shape[1:], dtype=np.float64)
        acc = np.empty(self.shape[1:], dtype=np.uint32)
        n_win, k = C.c_int64(0), C.c_int64(0)
        _check(self._lib.d3d_adapt_get(self._ctx, _dp(scale), acc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       C.byref(n_win), C.byref(k)))
        return scale, acc, n_win.value, k.value

    def adapt_set(self, scale=None, accepted=None, n_win=0, k=0):
        """Install a scale map and / or counters (resume; a fixed map with ``window = 0``)."""
        hw = self.shape[1:]
        sp = ap = None
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64)
            if scale.shape != hw:
                raise ValueError("scale map MUST have shape %s, got %s" % (hw, scale.shape))
            sp = _dp(scale)
        if accepted is not None:
            accepted = np.ascontiguousarray(accepted, dtype=np.uint32)
            if accepted.shape != hw:
                raise ValueError("accepted map MUST have shape %s, got %s" % (hw, accepted.shape))
            ap = accepted.ctypes.data_as(C.POINTER(C.c_uint32))
        _check(self._lib.d3d_adapt_set(self._ctx, sp, ap, int(n_win), int(k)))

    def adapt_end(self):
        _check(self._lib.d3d_adapt_end(self._ctx))

    # -- weights of a Student-t likelihood ------------------------------------------------
    def robust_begin(self, nu, every=1, start=0, accumulate_from=0):
        """Arm the per-voxel weights of a Student-t likelihood with ``nu`` degrees of freedom
        (include/deconv3d_hip.h: d3d_robust_begin): after every sweep s >= ``start`` with
        ``(s - start) % every == 0`` (the run's numbering) the device redraws them from the residual
        and rewrites 1/variance; the draws of the sweeps from ``accumulate_from`` on enter their
        running mean.  Needs set_data."""
        _check(self._lib.d3d_robust_begin(self._ctx, int(nu), int(every), int(start), int(accumulate_from)))

    def robust_step(self, sweep_number):
        """One draw now, as the one after sweep ``sweep_number`` (the run's numbering)."""
        _check(self._lib.d3d_robust_step(self._ctx, int(sweep_number)))

    def robust_get(self, weights=True, weight_mean=True):
        """(current weights (D,H,W), their running mean (D,H,W), accumulated draws); NaN where the
        voxel carries no information, None for an array that was not asked for."""
        w = np.empty(self.shape, dtype=np.float64) if weights else None
        m = np.empty(self.shape, dtype=np.float64) if weight_mean else None
        n = C.c_int64(0)
        _check(self._lib.d3d_robust_get(self._ctx, _dp(w) if weights else None,
                                        _dp(m) if weight_mean else None, C.byref(n)))
        return w, m, n.value

    def robust_end(self):
        """Disarm: the base 1/variance back, bit for bit."""
        _check(self._lib.d3d_robust_end(self._ctx))

    # -- variance factors of channel groups ----------------------------------------------
    def noise_begin(self, group, n_groups=None, spaxels=None, shape=0., rate=0., every=1, start=0, capacity=1):
        """Arm the variance factors of the channel groups (include/deconv3d_hip.h: d3d_noise_begin):
        ``group`` (D,) maps every channel to 0 .. n_groups-1 or -1 (never rescaled), ``spaxels`` (H,W)
        0/1 the counted spaxels (None: all); after every sweep s >= ``start`` with ``(s - start) %
        every == 0`` (the run's numbering) the device redraws the factors from the residual and rewrites
        1/variance; ``capacity`` draws fit the series.  Needs set_data."""
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.shape != (self.shape[0],):
            raise ValueError("group must have shape (%d,), got %s" % (self.shape[0], group.shape))
        if n_groups is None:
            n_groups = int(group.max()) + 1
        sp = None
        if spaxels is not None:
            sp = np.ascontiguousarray(np.asarray(spaxels) != 0, dtype=np.uint8)
            if sp.shape != tuple(self.shape[1:]):
                raise ValueError("spaxels must have shape %s, got %s" % (tuple(self.shape[1:]), sp.shape))
        _check(self._lib.d3d_noise_begin(
            self._ctx, group.ctypes.data_as(C.POINTER(C.c_int32)), int(n_groups),
            None if sp is None else sp.ctypes.data_as(C.POINTER(C.c_uint8)), float(shape), float(rate),
            int(every), int(start), int(capacity)))
        self._noise_groups = int(n_groups)

    def noise_step(self, sweep_number):
        """One draw now, as the one after sweep ``sweep_number`` (the run's numbering)."""
        _check(self._lib.d3d_noise_step(self._ctx, int(sweep_number)))

    def noise_count(self):
        """Draws in the series."""
        n = C.c_int64(0)
        _check(self._lib.d3d_noise_count(self._ctx, C.byref(n)))
        return n.value

    def noise_get(self):
        """``(scale (n, G), sweeps (n,), voxels (G,), last_sum (G,), tau (D,))``: the series of scales
        (NaN: a group of fewer than 2 counted voxels) and the sweep of every row, N_g and Q_g of the last
        draw, and the factor 1/variance carries in every channel now."""
        n = self.noise_count()
        G = self._noise_groups
        series = np.empty((n, G), dtype=np.float64)
        sweeps = np.empty((n,), dtype=np.int64)
        voxels, last = np.empty((G,), dtype=np.float64), np.empty((G,), dtype=np.float64)
        tau = np.empty((self.shape[0],), dtype=np.float64)
        _check(self._lib.d3d_noise_get(self._ctx, _dp(series), sweeps.ctypes.data_as(C.POINTER(C.c_int64)),
                                       _dp(voxels), _dp(last), _dp(tau)))
        return series, sweeps, voxels, last, tau

    def noise_end(self):
        """Disarm: the base 1/variance back, bit for bit."""
        _check(self._lib.d3d_noise_end(self._ctx))

    # -- pointwise predictive accuracy --------------------------------------------------
    def pred_begin(self):
        """Allocate and zero the four accumulators of the pointwise log density (include/
        deconv3d_hip.h: d3d_pred_begin) and start the moments afresh: every sample of theirs is
        from now on one of these too.  Needs post_begin; after robust_begin when both are wanted."""
        _check(self._lib.d3d_pred_begin(self._ctx))

    def pred_count(self):
        n = C.c_int64(0)
        _check(self._lib.d3d_pred_count(self._ctx, C.byref(n)))
        return n.value

    def pred_get(self):
        """The raw accumulators (M, S, mean, M2) of q, each (D,H,W), 0 where the voxel is not counted."""
        out = [np.empty(self.shape, dtype=np.float64) for _ in range(4)]
        _check(self._lib.d3d_pred_get(self._ctx, *[_dp(a) for a in out]))
        return tuple(out)

    def pred_maps(self):
        """(H,W,4): sum of lppd_v, sum of p_v, counted voxels, sum of (lppd_v - p_v)^2 per spaxel."""
        out = np.empty(self.shape[1:] + (4,), dtype=np.float64)
        _check(self._lib.d3d_pred_maps(self._ctx, _dp(out)))
        return out

    def pred_cubes(self, lppd=True, p_waic=True):
        """(lppd_v, p_v), each (D,H,W) with NaN where the voxel is not counted; None for one not asked for."""
        a = np.empty(self.shape, dtype=np.float64) if lppd else None
        b = np.empty(self.shape, dtype=np.float64) if p_waic else None
        _check(self._lib.d3d_pred_cubes(self._ctx, _dp(a) if lppd else None, _dp(b) if p_waic else None))
        return a, b

    def pred_end(self):
        _check(self._lib.d3d_pred_end(self._ctx))

    # -- smoothness prior between neighbouring spaxels ----------------------------------
    def prior_begin(self, lam):
        """Turn the pairwise Gaussian prior between 4-neighbours on with ``lam = 1 / sigma^2`` of
        (a, c, w) (include/deconv3d_hip.h: d3d_prior_begin)."""
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
        if lam.size != 3:
            raise ValueError("lam MUST hold the 3 values of (a, c, w), got %d" % lam.size)
        _check(self._lib.d3d_prior_begin(self._ctx, _dp(lam)))

    def prior_get(self):
        """(lam, on): the prior's weights as begun (zeros when off) and whether it is on."""
        lam = np.zeros(3, dtype=np.float64)
        on = C.c_int(0)
        _check(self._lib.d3d_prior_get(self._ctx, _dp(lam), C.byref(on)))
        return lam, bool(on.value)

    def prior_end(self):
        _check(self._lib.d3d_prior_end(self._ctx))

    def prior_energy(self, params=None):
        """(E_a, E_c, E_w, pairs): the sums of squared differences between unmasked 4-neighbours
        of an (H,W,3) map (None: the current parameters), summed on the device."""
        pp = None
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            if params.shape != tuple(self.shape[1:]) + (3,):
                raise ValueError("parameter map MUST have shape %s, got %s"
                                 % (tuple(self.shape[1:]) + (3,), params.shape))
            pp = _dp(params)
        energy = np.zeros(3, dtype=np.float64)
        pairs = C.c_int64(0)
        _check(self._lib.d3d_prior_energy(self._ctx, pp, _dp(energy), C.byref(pairs)))
        return float(energy[0]), float(energy[1]), float(energy[2]), int(pairs.value)

    # -- matched-filter line search ---------------------------------------------------
    def line_search(self, centres, widths, bank=None):
        """(best, stat) of include/deconv3d_hip.h: d3d_line_search -- per spaxel the index
        ``i_w * n_c + i_c`` of the best template over ``widths`` x ``centres`` (-1: none, or
        masked) and ``{N, Q, s(i_c - 1), s(i_c + 1)}``.  ``bank``: ``(n_w * n_c, D)`` templates
        evaluated on the host, used instead of the device's."""
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        widths = np.ascontiguousarray(widths, dtype=np.float64).reshape(-1)
        bank_p = None
        if bank is not None:
            bank = _c64(bank, (centres.size * widths.size, self.shape[0]))
            bank_p = _dp(bank)
        best = np.empty(self.shape[1:], dtype=np.int32)
        stat = np.empty(self.shape[1:] + (4,), dtype=np.float64)
        _check(self._lib.d3d_line_search(self._ctx, int(centres.size), _dp(centres), int(widths.size),
                                         _dp(widths), bank_p,
                                         best.ctypes.data_as(C.POINTER(C.c_int32)), _dp(stat)))
        return best, stat

    # -- preparation of a raw cube ------------------------------------------------------
    def _bytes(self, a, shape, what):
        if a is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
        if a.shape != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (what, tuple(shape), a.shape))
        return a, a.ctypes.data_as(C.POINTER(C.c_uint8))

    def running_median(self, cube, half_window, valid=None):
        """include/deconv3d_hip.h: d3d_running_median -- the median along z of every voxel's
        ``2 half_window + 1`` window over the valid voxels (``valid``: (D,H,W), non-zero = valid;
        default the finite ones)."""
        cube = _c64(cube, self.shape)
        valid, valid_p = self._bytes(valid, self.shape, "valid")
        out = np.empty(self.shape, dtype=np.float64)
        _check(self._lib.d3d_running_median(self._ctx, _dp(cube), valid_p, int(half_window), _dp(out)))
        return out

    def channel_stats(self, cube, select=None):
        """include/deconv3d_hip.h: d3d_channel_stats -- ``(median, mad, count)`` of every channel
        plane over the finite voxels of the spaxels ``select`` (H,W) marks (default all)."""
        cube = _c64(cube, self.shape)
        select, select_p = self._bytes(select, self.shape[1:], "select")
        depth = self.shape[0]
        m, mad = np.empty(depth), np.empty(depth)
        n = np.empty(depth, dtype=np.int64)
        _check(self._lib.d3d_channel_stats(self._ctx, _dp(cube), select_p, _dp(m), _dp(mad),
                                           n.ctypes.data_as(C.POINTER(C.c_int64))))
        return m, mad, n

    def prepare(self, cube, half_window, reject=None, select=None):
        """include/deconv3d_hip.h: d3d_prepare -- ``(continuum, residual, median, sigma, count)``:
        the running-median continuum, ``cube - continuum`` and per channel the residual's median,
        ``1.4826 MAD`` (NaN: no information) and count; ``reject``: sigmas of the one rejection
        pass, ``None`` for none."""
        cube = _c64(cube, self.shape)
        select, select_p = self._bytes(select, self.shape[1:], "select")
        cont = np.empty(self.shape, dtype=np.float64)
        res = np.empty(self.shape, dtype=np.float64)
        chan = np.empty((self.shape[0], 3), dtype=np.float64)
        _check(self._lib.d3d_prepare(self._ctx, _dp(cube), select_p, int(half_window),
                                     float("nan") if reject is None else float(reject),
                                     _dp(cont), _dp(res), _dp(chan)))
        return cont, res, chan[:, 0].copy(), chan[:, 1].copy(), chan[:, 2].astype(np.int64)
