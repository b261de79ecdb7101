/*
 * deconv3d_hip.h -- C ABI of libdeconv3d_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-iteration likelihood path of irap-omp/deconv3d.
 * The reference has NO FFI of its own (it is pure python/numpy),
 * so every entry point below cites the reference python code it replaces
 * (paths relative to the reference root).  The reference-side binding a
 * maintainer would add (a ctypes stub inside lib/run.py) is shown in
 * INTEGRATION.md; the build's own host side is deconv3d_amd/_lib.py.
 *
 * Conventions
 *   - all floating point is IEEE fp64; host arrays are C-contiguous and
 *     caller-owned, in the reference's layouts:
 *         cube   (D, H, W)   x fastest            lib/run.py:146-149
 *         params (H, W, 3)   (a, c, w)            lib/line_models.py:70-71
 *         fsf    (fh, fw)    odd sizes            lib/run.py:209-211
 *         lsf    [D]         centred as lib/spread_functions.py:251
 *         mask   (H, W)      uint8, 1 = iterate   lib/run.py:151-165
 *   - the library copies host data to HBM and never retains a host pointer
 *     after the call returns;
 *   - every function returns 0 on success and a negative d3d_status on error;
 *     d3d_last_error() returns a thread-local human readable message;
 *   - a d3d_ctx is bound to one device and one HIP stream; it is not
 *     thread-safe; use one ctx per device (one process per GPU in multi-GPU
 *     runs).  There is NO CPU fallback: without a HIP device d3d_ctx_create
 *     fails with D3D_ERR_NO_DEVICE.
 */
#ifndef DECONV3D_HIP_H
#define DECONV3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct d3d_ctx d3d_ctx;

typedef enum d3d_status {
    D3D_OK = 0,
    D3D_ERR_INVALID = -1,    /* bad argument / shape (python: ValueError)   */
    D3D_ERR_NO_DEVICE = -2,  /* no usable HIP device                        */
    D3D_ERR_HIP = -3,        /* a HIP runtime call failed                   */
    D3D_ERR_STATE = -4,      /* call sequence error (taps/data/params unset)*/
    D3D_ERR_UNSUPPORTED = -5 /* shape outside the kernels' limits           */
} d3d_status;

/* Device cubes owned by a ctx, addressable through the *_slot functions.   */
typedef enum d3d_slot {
    D3D_SLOT_DATA = 0,   /* observed cube (NaN -> 0 with ivar 0)             */
    D3D_SLOT_IVAR = 1,   /* 1/variance                                       */
    D3D_SLOT_ERR = 2,    /* residual data - sim carried by the MH loop       */
    D3D_SLOT_SIM = 3,    /* last forward model                               */
    D3D_SLOT_TMP0 = 4,   /* scratch (LSF-convolved lines / user cube)        */
    D3D_SLOT_TMP1 = 5,   /* scratch                                          */
    D3D_SLOT_COUNT = 6
} d3d_slot;

/* library version: major*10000 + minor*100 + patch */
int d3d_version(void);
/* sha256 (first 16 hex digits) of the HIP/C++ sources this binary was compiled
 * from (csrc/Makefile bakes it in); __graft_entry__.build() compares it with the
 * sources in the tree and rebuilds on a mismatch. */
const char *d3d_source_hash(void);
/* thread-local message of the last failing call ("" if none) */
const char *d3d_last_error(void);
/* number of visible HIP devices (0 and D3D_OK when there is none) */
int d3d_device_count(int *count);

/* ---- context ----------------------------------------------------------- */

/* Replaces the shape bookkeeping of Run.__init__, lib/run.py:145-149,219-224.
 * D,H,W: cube shape; fh,fw: FSF shape (odd).  Allocates all device cubes. */
int d3d_ctx_create(d3d_ctx **ctx, int device, int D, int H, int W, int fh, int fw);
int d3d_ctx_destroy(d3d_ctx *ctx);
/* Run on a caller-owned HIP stream (e.g. torch's current stream) instead of
 * the ctx's own; NULL restores the own stream.  The handle must come from the HIP runtime
 * this library is linked to: a stream of a second copy of the runtime in the process (a
 * PyTorch wheel that bundles its own libamdhip64) means nothing to this one. */
int d3d_ctx_set_stream(d3d_ctx *ctx, void *hip_stream);
/* Block until everything queued on the ctx stream has finished. */
int d3d_sync(d3d_ctx *ctx);
/* HIP-event stopwatch on the ctx stream (for bench.py's roofline leg). */
int d3d_timer_start(d3d_ctx *ctx);
int d3d_timer_stop(d3d_ctx *ctx, double *elapsed_ms);
/* Per-context options: which kernel family / geometry a ctx uses where the library
 * has more than one (the reference has no counterpart: numpy picks nothing,
 * lib/run.py:3-31 is its whole import list).  Every default is the measured best and
 * every choice gives the same chain (bit for bit unless DESIGN.md says "to rounding"),
 * so none is needed in normal use; they exist for the bit-identity tests and for A/B
 * measurements.  An option belongs to ONE ctx: two contexts of a process may differ.
 * The environment variable D3D_<KEY> (upper case) only supplies a NEW ctx's default.
 * Changing an option flushes pending residual updates and re-derives what depends
 * on it (work lists, tap analysis), so it may be called at any time between calls.
 * Keys: mh_defer 0|1|2, mh_zblocks, mh_layers 0(auto)|1|2|3,
 * mh_wide, mh_props, halo_timing, mh_zigzag, mh_nt_ivar -1(auto)|0|1, mh_strips 0(auto)|1|2|3|4,
 * mh_strip_order 0(auto)|1 joined|2 chained, mh_strip_lag (tests only), mh_nt, uniform_ivar, conv_rows,
 * conv_zb, conv_hy, spatial_sep, sep_fuse, spatial_mode, march_hy, zmajor, zmajor_hy,
 * spectral_dense, spectral_blocks, lines_dense, lines_rounds, spatial_nt, xcd_remap, alt_dir, stagger,
 * post_nt, noise_timing; a build with
 * `make EXPERIMENTS=1` adds mh_chain, mh_prio, mh_maxit, mh_flow, mh_pair, spectral_shfl, fuse_lsf, march_pf,
 * march_one, march_stamp.  Unknown key or value out of range: D3D_ERR_INVALID.
 * d3d_ctx_get_option also answers the read-only key "chain_parts": how many of the
 * ctx's parts run their sweeps as one launch of persistent workgroups (k_mh_chain), and
 * "search_bank_ns" / "search_kernel_ns": device time of the last d3d_line_search call's bank build
 * and of its search kernel, and "prep_median_ns" / "prep_stats_ns": device time of the running-median
 * and channel-statistics kernels of the last d3d_running_median / d3d_channel_stats / d3d_prepare.
 * Three more read-only keys name the kernel family the dispatcher took LAST (a host-side int per
 * ctx, 0 before the first launch; the tests assert them, nothing in the library reads them):
 * "spatial_path" (the last FSF pass -- d3d_convolve_slots, d3d_forward, d3d_residual, d3d_simulate,
 * a residual rebuilt by the sweeps), "spectral_path" (the last stand-alone LSF pass of
 * d3d_convolve_slots) and "stage_path" (the last d3d_stage_convolve / d3d_convolve): the
 * D3D_SPATIAL_*, D3D_SPECTRAL_* and D3D_STAGE_* codes below.
 * "noise_sums_ns" / "noise_draw_ns" / "noise_apply_ns" (read-only): device time of the three kernels of
 * the last d3d_noise_step made with the option noise_timing = 1 (HIP events between its launches; the
 * draws of the sweeps are never timed).
 * "device_bytes" (read-only): the bytes of device memory the library holds, over all contexts and
 * tempering groups of the process (the pinned snapshot ring is host memory and not counted).
 * Three read-only keys say what the dispatcher of the MH sweep launched (host-side words of the ctx,
 * written where each sweep kernel is launched; no kernel argument, nothing in the library reads them):
 * "mh_path", the packed D3D_MH_* code of the LAST sweep-kernel launch (0: none since the record was
 * cleared) -- kernel family, streaming threads NS, window positions in flight U, pending layers the
 * kernel can apply M, staging registers K and the flags NTV (non-temporal 1/variance, write-through
 * residual), UV (uniform variance), PRIOR and MULTI (multiplet or tabulated line); "mh_path_layers",
 * bit n set when a launch found n layers pending (n = 0..3); "mh_path_launches", the launches counted.
 * All three count since the record was last cleared: by d3d_mh_config, and by READING
 * "mh_path_launches" (read it last).  A launch in lattice-row strips counts once per strip; of a
 * d3d_mh_sweeps_batch the record is the leader's (ctx 0).
 * "device_cus" (read-only): the compute units of the ctx's device.  A colour launch of fewer than 2
 * workgroups per compute unit "does not fill the chip": the rule by which the dispatcher picks the
 * variants with more window positions in flight. */
enum {
    D3D_MH_FAMILY_MASK = 0xf,      /* code & mask: one of the families below */
    D3D_MH_WS = 1,                 /* k_mh_ws (NS 256, 512, or the wide form's) */
    D3D_MH_SMALL = 2,              /* k_mh_small, 256 threads */
    D3D_MH_SMALL_WIDE = 3,         /* k_mh_small, the wide form of a partitioned ctx at 128 channels */
    D3D_MH_ZB = 4,                 /* k_mh_ws<..., ZBK> on (window, 256-channel block) + k_mh_zdecide */
    D3D_MH_BATCH_WS = 5,           /* d3d_mh_sweeps_batch: k_mh_ws<..., BATCH> */
    D3D_MH_BATCH_SMALL = 6,        /* d3d_mh_sweeps_batch: k_mh_small<..., BATCH> */
    D3D_MH_DEFER = 7,              /* k_mh_defer<NS> (option mh_defer = 2; deep cubes without z-blocks) */
    D3D_MH_IMMEDIATE = 8,          /* k_mh<NS> (option mh_defer = 0, d3d_mh_colour) */
    D3D_MH_DEEP = 9,               /* k_mh_deep: more than 1024 channels, threads loop over z-pairs */
    D3D_MH_FLOW = 10,              /* k_mh_flow (`make EXPERIMENTS=1`) */
    D3D_MH_PAIR = 11,              /* k_mh_pair (`make EXPERIMENTS=1`) */
    D3D_MH_CHAIN = 12,             /* k_mh_chain (`make EXPERIMENTS=1`) */
    D3D_MH_SMALL_FULL = 13,        /* k_mh_small<..., FULL> (`make EXPERIMENTS=1`, option mh_small = 2) */
    D3D_MH_U_SHIFT = 4,            /* 4 bits: window positions in flight per thread (0: not a parameter) */
    D3D_MH_U_MASK = 0xf,
    D3D_MH_M_SHIFT = 8,            /* 2 bits: pending layers the kernel can apply */
    D3D_MH_M_MASK = 0x3,
    D3D_MH_K_SHIFT = 10,           /* 3 bits: registers a staged G row takes (0: not a parameter) */
    D3D_MH_K_MASK = 0x7,
    D3D_MH_NTV = 1 << 13,          /* non-temporal 1/variance loads, write-through residual stores */
    D3D_MH_UV = 1 << 14,           /* the uniform-variance instantiation */
    D3D_MH_PRIOR = 1 << 15,        /* the smoothness prior's terms (d3d_prior_begin) */
    D3D_MH_MULTI = 1 << 16,        /* the multiplet / tabulated form of the unit line */
    D3D_MH_NS_SHIFT = 17,          /* 11 bits: streaming threads (k_mh, k_mh_defer, k_mh_deep: all threads) */
    D3D_MH_NS_MASK = 0x7ff
};
enum {
    D3D_SPATIAL_CONV_ROWS = 1,     /* k_conv_rows, FSF only, one block of <= 128 channels */
    D3D_SPATIAL_CONV_ROWS_ZB = 2,  /* k_conv_rows in z-blocks of 128 channels (FSF only) */
    D3D_SPATIAL_CONV_ROWS_LSF = 3, /* k_conv_rows with the LSF epilogue */
    D3D_SPATIAL_MARCH_XY = 10,     /* k_spatial_march<SYMX, SYMY>: both mirror symmetries */
    D3D_SPATIAL_MARCH_X = 11,      /* k_spatial_march<SYMX>: x symmetry only */
    D3D_SPATIAL_MARCH = 12,        /* k_spatial_march without symmetry */
    D3D_SPATIAL_SEP = 13,          /* k_spatial_sep: outer-product FSF */
    D3D_SPATIAL_SEP_LSF = 14,      /* k_spatial_sep_lsf: outer-product FSF and LSF in one pass */
    D3D_SPATIAL_MARCH_EXPERIMENT = 15, /* a march variant of a `make EXPERIMENTS=1` build */
    D3D_SPATIAL_GENERIC = 30,      /* k_spatial_generic: any FSF shape */
    D3D_SPATIAL_DEEP = 40,         /* k_spatial_deep: more than 1024 channels */
    D3D_SPATIAL_TILE = 10000,      /* k_spatial<NT> (tile kernel): D3D_SPATIAL_TILE + NT */
    D3D_SPECTRAL_BLOCKS = 1,       /* k_spectral_blocks */
    D3D_SPECTRAL_DEEP = 2,         /* k_spectral_deep */
    D3D_SPECTRAL_DENSE = 3,        /* k_spectral_dense */
    D3D_SPECTRAL_TAPS = 4,         /* k_spectral (tap list) */
    D3D_SPECTRAL_SHFL = 5,         /* k_spectral_shfl (`make EXPERIMENTS=1`) */
    D3D_STAGE_ZMAJOR = 1,          /* k_spectral_z / k_spatial_z in the reference layout */
    D3D_STAGE_TRANSPOSE = 2        /* transpose, slot kernels (d3d_convolve_slots), transpose back */
};
int d3d_ctx_set_option(d3d_ctx *ctx, const char *key, long value);
int d3d_ctx_get_option(d3d_ctx *ctx, const char *key, long *value);
/* 1 when the library was built with `make EXPERIMENTS=1` (the measured-but-not-faster
 * kernel variants of DESIGN.md section 3 are present), else 0. */
int d3d_has_experiments(void);

/* ---- inputs ------------------------------------------------------------ */

/* Taps produced once per run by instrument.fsf.as_image / lsf.as_vector,
 * lib/run.py:207-211.  lsf may be NULL (no spectral pass: lib/run.py:675-676,
 * 1015-1016).  LSF taps with |lsf[t]| <= lsf_rel_threshold*max|lsf| are
 * dropped (0 keeps every non-zero tap).  A NEGATIVE value is an error bound: the
 * smallest taps are dropped while their summed magnitude stays within
 * |lsf_rel_threshold| * sum|lsf| (the python host uses -1e-16: below the rounding of
 * the fp64 sum). */
int d3d_set_taps(d3d_ctx *ctx, const double *fsf, const double *lsf,
                 double lsf_rel_threshold);
/* Data / variance / mask setup of lib/run.py:137-200.  var may be NULL (then
 * var_scalar is the constant variance, lib/run.py:186-192); zero variances
 * become 1e12 (lib/run.py:180); NaN voxels get data 0 and 1/var 0 (SURVEY.md
 * appendix A); mask may be NULL (all ones). */
int d3d_set_data(d3d_ctx *ctx, const double *data, const double *var,
                 double var_scalar, const uint8_t *mask);
/* Current parameter map, lib/run.py:294-314,338. */
int d3d_set_params(d3d_ctx *ctx, const double *params);
int d3d_get_params(d3d_ctx *ctx, double *params);
/* Unit line of the line model (lib/line_models.py:17-61, 92-109): K Gaussians of the
 * spaxel's one centre c and width w at channel offsets offsets[k] from c, with flux ratios
 * ratios[k] relative to the first,
 *   sum_k ratios[k] * exp(-((z - c) - offsets[k])^2 / (2 w^2)),
 * summed in component order -- a multiplet with tied kinematics ([OII] 3726,3729, Halpha
 * with [NII]; python: GaussianMultipletLineModel).  Still linear in the amplitude a, so the
 * parameters stay (a, c, w).  1 <= K <= 4, offsets[0] == 0 and ratios[0] == 1 (c and a are
 * the first line's), every value finite, ratios >= 0, offsets distinct; anything else is
 * D3D_ERR_INVALID.  Default on creation: K = 1, {0}, {1} (SingleGaussianLineModel, bit for
 * bit).  Writes the pending updates back, then invalidates the residual and the sweep's
 * proposal / line tables: every later line build (forward model, simulate, MH updates,
 * residual refresh) uses the new shape. */
int d3d_set_line_shape(d3d_ctx *ctx, int K, const double *offsets, const double *ratios);
/* A tabulated profile phi in place of the Gaussian of the unit line (lib/line_models.py:17-61,
 * 92-109: the reference's LineModel plugin, here for any a * phi((z - c) / w)): table holds n
 * samples of phi on the uniform grid u_j = -support + j h, h = 2 support / (n - 1), and every
 * component of the line shape becomes ratios[k] * phi(((z - c) - offsets[k]) / w) (python:
 * TabulatedLineModel).  The curve is the Catmull-Rom cubic through the table padded with one
 * zero on each side: with u = d / w, t = (u + support) * inv_h, inv_h = (n - 1) / (2 support),
 * the value is 0 unless 0 <= t <= n - 1 (NaN: 0); else j = min(floor(t), n - 2), s = t - j,
 * p0..p3 the padded samples j-1 .. j+2 and
 *   p1 + 0.5 s ((p2 - p0) + s ((2 p0 - 5 p1 + 4 p2 - p3) + s (3 (p1 - p2) + (p3 - p0)))),
 * one IEEE double operation per step in this order; w == 0: phi(0) where d == 0, else 0.
 * 8 <= n <= 65537, support finite and > 0, every sample finite, the sample of largest
 * magnitude equal to 1 (a stays the peak amplitude; negative lobes are allowed), table not
 * NULL; anything else is D3D_ERR_INVALID and the old table stays.  flux_factor: the integral
 * of phi over u (the table's trapezoid sum times h), finite: the integrated flux of the
 * posterior moments and histograms is F = a w flux_factor sum_k ratios[k].  n == 0 (support,
 * table and flux_factor ignored) returns the ctx to Gaussians.  The ctx keeps its own copy.
 * d3d_set_line_shape sets offsets and ratios only and leaves the table alone.  Side effects as
 * d3d_set_line_shape: pending updates written back with the old line, residual, proposal /
 * line tables and posterior moments invalidated. */
int d3d_set_line_table(d3d_ctx *ctx, int n, double support, const double *table, double flux_factor);

/* ---- forward model ------------------------------------------------------ */

/* Run.simulate_clean, lib/run.py:597-621 (masked spaxels are zero). */
int d3d_build_clean(d3d_ctx *ctx, double *out_cube);
/* LSF (x) FSF convolution of an arbitrary cube: convolve_1d along z of every
 * spectrum (lib/convolution.py:89-120) then convolve2d(..., 'same') of every
 * channel (lib/run.py:1027-1029). */
int d3d_convolve(d3d_ctx *ctx, const double *in_cube, double *out_cube);
/* Fused forward model of the current parameters == Run.simulate_convolved
 * (lib/run.py:623-652) == the sim of _compute_error_in_one_step
 * (lib/run.py:999-1029).  out_sim may be NULL (result stays in SLOT_SIM). */
int d3d_forward(d3d_ctx *ctx, double *out_sim);
/* Run.simulate_clean(shape, parameters) (convolved = 0, lib/run.py:597-621) and
 * Run.simulate_convolved(shape, parameters) (convolved = 1, lib/run.py:623-652)
 * for an EXPLICIT (H,W,3) parameter map: the chain state (d3d_set_params, the
 * carried residual) is not touched.  Masked spaxels are zero. */
int d3d_simulate(d3d_ctx *ctx, const double *params, int convolved, double *out_cube);
/* err = data - forward(params), lib/run.py:334 and :525-534 / :999-1031.
 * Stored in SLOT_ERR; out_err may be NULL. */
int d3d_residual(d3d_ctx *ctx, double *out_err);
/* Per-spaxel 0.5*sum_z err^2/var of SLOT_ERR (the quantity of
 * lib/run.py:423 summed per spectrum) and its total.  Either may be NULL; with both NULL
 * the map stays on the device and the call returns without waiting for it. */
int d3d_chi2_map(d3d_ctx *ctx, double *out_hw, double *total);

/* The same convolution on a cube that stays on the device in the REFERENCE
 * layout (D,H,W) (lib/run.py:146-149): upload once, convolve in place any
 * number of times, download.  d3d_convolve == upload + convolve + download.
 * With mirror-symmetric FSFs and a compact LSF both passes run in that layout
 * (lanes along x), otherwise through the spectrum-contiguous slot kernels. */
int d3d_stage_upload(d3d_ctx *ctx, const double *cube);
int d3d_stage_convolve(d3d_ctx *ctx);
int d3d_stage_download(d3d_ctx *ctx, double *cube);

/* Device-resident variants (no host traffic; used by bench.py). */
int d3d_upload_slot(d3d_ctx *ctx, int slot, const double *cube);
int d3d_download_slot(d3d_ctx *ctx, int slot, double *cube);
int d3d_convolve_slots(d3d_ctx *ctx, int src_slot, int dst_slot);

/* ---- MH-within-Gibbs ---------------------------------------------------- */

/* Bounds (lib/run.py:235-245), Cauchy jump amplitudes (:251-262; the Gibbs
 * parameter's amplitude is forced to 0), a-priori variance of the amplitude
 * (:264-265), RNG seed (the reference is unseeded), and the cadence of the
 * from-scratch residual refresh (:525; 0 disables). */
int d3d_mh_config(d3d_ctx *ctx, const double min_b[3], const double max_b[3],
                  const double jump_amp[3], double gibbs_apriori_variance,
                  uint64_t seed, int refresh_every);
/* Resumed runs: sweep s draws the random numbers of sweep s + origin, so that a
 * chain continued from a checkpoint (lib/run.py:790-797 -> initial_parameters)
 * does not replay the random numbers of its first segment.  Default 0. */
int d3d_mh_set_sweep_origin(d3d_ctx *ctx, int64_t origin);
/* Parity probe: for a proposal p_new at spaxel (y,x) against the current
 * state, out = {ar_old, ar_new, ar_old-ar_new, sum ek^2/var, sum ek*ul/var}
 * (lib/run.py:400-426, 464-493).  Does not modify the state. */
int d3d_window_stats(d3d_ctx *ctx, int y, int x, const double p_new[3],
                     double out[5]);
/* n_sweeps sweeps of the inner loop lib/run.py:367-519 over every unmasked
 * spaxel, numbered first_sweep .. first_sweep+n_sweeps-1 (the reference's
 * cur_iteration).  After sweep s with s % keep_one_in == 0 the parameter map
 * is copied to chain_out[(s/keep_one_in)] ((H,W,3) each, lib/run.py:447-451)
 * and the log acceptance ratios to dlog_out[(s/keep_one_in)] ((H,W) each,
 * lib/run.py:428-432); either may be NULL.  *accepted (may be NULL) receives
 * the number of accepted MH proposals (lib/run.py:440). */
int d3d_mh_sweeps(d3d_ctx *ctx, int n_sweeps, int first_sweep, int keep_one_in,
                  double *chain_out, double *dlog_out, int64_t *accepted);
/* The same update for a line model evaluated on the HOST (a python LineModel
 * plugin with its own modelize(), lib/line_models.py:17-61): n spaxels of one
 * colour class (disjoint FSF windows; the caller guarantees it), per spaxel i
 *   spaxels[i]          local index y*W+x
 *   in3[i*3 + 0..2]     current Gibbs amplitude (1 if the model has none),
 *                       out-of-bounds flag of the proposal (lib/run.py:379-384),
 *                       log(u) of the acceptance test (lib/run.py:435)
 *   lines[(i*2+0)*D..]  current line, unit amplitude (lib/run.py:472, 481-488)
 *   lines[(i*2+1)*D..]  proposed line, unit amplitude
 * The device applies the LSF, the window statistics, accept, the Gibbs draw of
 * the amplitude when gibbs != 0 (bounds min_b[0]/max_b[0] of d3d_mh_config) and
 * the residual update; out3[i*3 + 0..2] = {accepted, new amplitude, delta}. */
int d3d_mh_colour_lines(d3d_ctx *ctx, int sweep, int n, const int *spaxels, const double *in3,
                        const double *lines, int gibbs, double *out3);
/* rtnorm(a, b, mu, sigma, size), lib/rtnorm.py:21-92: n draws of the normal
 * N(mu, sigma^2) truncated to [lo, hi], with the sampler the Gibbs step uses
 * (own algorithm, same distribution; the reference's Chopin tables are GPL and
 * are not reproduced).  Draw i uses the Philox stream (seed, i); wave_mode = 1
 * runs the wavefront-cooperative form of the MH kernel (bit-identical draws). */
int d3d_rtnorm(d3d_ctx *ctx, long n, double lo, double hi, double mu, double sigma,
               uint64_t seed, int wave_mode, double *out);
/* Test hook, like d3d_rtnorm: the raw generator under the sampler, for arbitrary
 * counters and keys.  For block i < n, out_words[4i..4i+3] = Philox4x32-10 of
 * counters[4i..4i+3] under keys[2i..2i+1] (the chain's layout: counter = {global
 * spaxel, sweep, block, 0}, key = {seed low, seed high}); out_pairs[2i], [2i+1]
 * = the two uniforms in [2^-53, 1 - 2^-53] made of words {1,0} and {3,2}. */
int d3d_philox(d3d_ctx *ctx, long n, const uint32_t *counters, const uint32_t *keys,
               uint32_t *out_words, double *out_pairs);
/* Last sweep's log acceptance ratios, (H,W). */
int d3d_get_dlog(d3d_ctx *ctx, double *out_hw);
/* *out = 1 when d3d_set_data found one constant variance and no NaN voxel -- the
 * reference's default when Run gets variance=None (lib/run.py:171-178 builds a
 * constant cube from median_clip) -- so that d3d_mh_sweeps streams the residual
 * only (16 instead of 24 bytes per window voxel; results are bit-identical to
 * the general kernel).  Option uniform_ivar = 0 turns the variant off. */
int d3d_variance_is_uniform(d3d_ctx *ctx, int *out);
/* *out = number of colours whose residual updates d3d_mh_sweeps keeps pending as
 * (colour, coefficient rows) layers before it writes the residual back: 2 by
 * default (the residual is stored every second colour: writing it costs about
 * twice what reading it does on MI355X), 1 for cubes whose colour launches do not
 * fill the chip or whose depth exceeds 256, 0 when updates are written at once (tiled contexts).  The chain
 * is bit-identical for every value.  Option mh_layers = 1|2|3 forces a depth; a
 * partitioned ctx reports the most layers any of its parts uses. */
int d3d_mh_layers(d3d_ctx *ctx, int *out);

/* ---- posterior moments -------------------------------------------------- */
/* The reference's only estimator is the mean of the last 20 % of the saved parameter chain
 * (Run.extract_parameters, lib/run.py:581-593), and its cubes are built from that mean map
 * (lib/run.py:597-652).  These entries keep, on the device, the running mean and the sum of
 * squared deviations M2 (Welford) of the SAMPLES' cubes -- what np.mean / np.var over
 * simulate_clean / simulate_convolved (lib/run.py:597-652) of every chain slot would give, with no
 * cube crossing to the host per sample -- and of the parameters with the integrated flux
 * F = a w sqrt(2 pi) sum_k ratios[k].  variance = M2 / (n - 1).  Off until begun: a ctx that
 * never calls d3d_post_begin allocates and launches nothing for them. */

/* Allocate and zero the accumulators: the (H,W,4) map of (a, c, w, F) always; what bit 0 the
 * clean cube (lib/run.py:597-621 per sample), bit 1 the convolved cube (lib/run.py:623-652 per
 * sample): two cubes each.  Calling it again starts afresh.  A tile ctx (d3d_set_tile) is
 * D3D_ERR_UNSUPPORTED; an allocation failure is D3D_ERR_HIP, frees what it got and leaves the ctx
 * usable for the chain.  d3d_set_line_shape, d3d_set_taps and d3d_set_data on a ctx with
 * accumulators reset them (count 0). */
int d3d_post_begin(d3d_ctx *ctx, int what);
/* d3d_mh_sweeps and d3d_mh_sweeps_batch (every ctx of the batch that has a schedule) take the
 * state after every sweep s >= first_sweep with (s - first_sweep) % every == 0 as a sample -- s
 * in the caller's numbering, the reference's cur_iteration (lib/run.py:344-353), where the saved
 * sweeps are copied to the chain (lib/run.py:447-451).  every >= 1. */
int d3d_post_schedule(d3d_ctx *ctx, int first_sweep, int every);
/* The current parameters as one more sample (callers that drive d3d_mh_phase / d3d_mh_colour
 * themselves; tests).  Needs parameters, and taps for the convolved cube: D3D_ERR_STATE. */
int d3d_post_accumulate(d3d_ctx *ctx);
/* *n = samples accumulated since d3d_post_begin or the last reset. */
int d3d_post_count(d3d_ctx *ctx, int64_t *n);
/* which = 0: the map, mean and m2 (H,W,4) each; 1: the clean cube; 2: the convolved cube, (D,H,W)
 * each in the reference's layout (lib/run.py:146-149).  Either pointer may be NULL.  A moment
 * that was not begun is D3D_ERR_STATE. */
int d3d_post_get(d3d_ctx *ctx, int which, double *mean, double *m2);
/* Free the accumulators and drop the schedule (d3d_ctx_destroy does it too). */
int d3d_post_end(d3d_ctx *ctx);

/* ---- posterior histograms ------------------------------------------------- */
/* The moments summarise a spaxel's (a, c, w, F) badly where they are heavy-tailed or bimodal, and
 * the reference can read a median or an interval only off the saved chain (lib/run.py:447-451,
 * 581-593).  These entries keep, per unmasked spaxel and per quantity of the d3d_post_get map, a
 * histogram of 64 equal bins and two tail counters (below, above), all uint32, filled on the device
 * from every sample the moments take after their first `pilot`:
 *   range, frozen once, right after sample number pilot:  sd = sqrt(M2 / (pilot - 1)),
 *     lo = max(mean - span sd, L), hi = min(mean + span sd, U), with L, U the bounds of
 *     d3d_mh_config for a, c, w and min_a min_w flux_k, max_a max_w flux_k for F; when !(sd > 0)
 *     or !(hi > lo): lo = L, hi = U; when still !(hi > lo) the series is never counted.  Masked
 *     spaxels are never counted and their range is NaN, as is every range before the freeze;
 *   counting:  b = floor((v - lo) * (64 / (hi - lo))); b < 0 -> below, b >= 64 -> above, else bin b;
 *   quantile q:  n = below + sum(bins) + above, t = q n; NaN when n == 0; lo when t <= below; hi
 *     when t > n - above; else, b the first bin with below + cum[b] >= t,
 *     lo + (b + (t - (below + cum[b] - cnt[b])) / cnt[b]) * ((hi - lo) / 64);
 *   mode:  lo + (b* + 0.5) * ((hi - lo) / 64), b* the lowest bin with the largest count; NaN when
 *     every bin is empty;
 *   outside:  (below + above) / n, the share of the samples the frozen range missed -- a second
 *     mode the pilot never visited is counted here, not resolved.
 * Every step is a plain IEEE double operation in the written order.  1120 bytes per spaxel. */

/* Allocate the counters (needs d3d_post_begin and d3d_mh_config: D3D_ERR_STATE) and start the
 * moments afresh (count 0): their first `pilot` samples set the ranges.  pilot < 2, or a span that
 * is not finite and positive: D3D_ERR_INVALID.  An allocation failure is D3D_ERR_HIP, frees what it
 * got and leaves the ctx usable.  Whatever resets the moments zeroes the counters and unfreezes the
 * ranges; d3d_post_begin and d3d_post_end free them. */
int d3d_hist_begin(d3d_ctx *ctx, int64_t pilot, double span);
/* *n = samples counted into every histogram: max(moments' count - pilot, 0). */
int d3d_hist_count(d3d_ctx *ctx, int64_t *n);
/* bins (H,W,4,64), tails (H,W,4,2) = below | above, range (H,W,4,2) = lo | hi.  Any may be NULL. */
int d3d_hist_get(d3d_ctx *ctx, uint32_t *bins, uint32_t *tails, double *range);
/* quantiles (H,W,4,n_q) for q[0..n_q), mode (H,W,4) and outside (H,W,4), extracted on the device
 * (k_hist_quantiles).  Outputs may be NULL.  n_q outside 1..8 or a q outside (0,1): D3D_ERR_INVALID. */
int d3d_hist_quantiles(d3d_ctx *ctx, int n_q, const double *q, double *quantiles, double *mode, double *outside);
/* Free the counters; the moments go on. */
int d3d_hist_end(d3d_ctx *ctx);

/* ---- region posteriors ---------------------------------------------------- */
/* Under an FSF wider than a spaxel neighbours trade flux, and what is well determined is a SET of
 * spaxels: the flux of an aperture, the flux-weighted velocity and dispersion of a ring, the
 * integrated deconvolved spectrum of a region.  The reference's only estimator is the mean of the
 * saved chain per spaxel (Run.extract_parameters, lib/run.py:581-593), and the std of a sum is not
 * derivable from per-spaxel moments: the covariances between trading neighbours are what matters.
 * These entries keep, for every sample the moments take (number n, counted from 1) and every region
 * k = 1..K of an int32 label map (H,W) -- 0: no region --
 *   F_i = (a_i w_i) flux_k of member i (the F of d3d_post_get's map),
 *   F_k = sum F_i,   C_k = (sum F_i c_i) / F_k,
 *   S_k = sqrt((sum F_i (w_i^2 + (c_i - C_k)^2)) / F_k)   (a second pass, with C_k known),
 *   F_k == 0 (no member, or no flux):  (F, C, S) = (0, NaN, NaN),
 * as row n - 1 of a series (capacity, K, 3) -- past `capacity` the series stops, nothing else does --
 * and, with the spectra on, the region's clean spectrum of the sample (lib/run.py:597-621 per
 * sample, summed over the members)
 *   s_k(z) = sum_i a_i unit_line(z, c_i, w_i)
 * into a running mean and M2 (K, D) by the Welford update of the moments.
 * THE ORDER OF EVERY SUM IS FIXED; it depends on the label map and the mask alone:
 *   members of region k: its unmasked spaxels in row-major order, m = 0 .. n_k - 1, cut into
 *     consecutive chunks of 64 (the last may be short);
 *   a scalar chunk partial: its 64 terms (absent ones +0.0) folded by halves,
 *     v[0:32] + v[32:64], then v[0:16] + v[16:32], ... down to one;
 *   a spectrum chunk partial, per channel: the members' terms one after the other in ascending
 *     m, starting from +0.0;
 *   a region's sum: its chunk partials one after the other in ascending order, from +0.0.
 * Every step is a plain IEEE double operation (no contraction), so F, C and S -- only + * / sqrt
 * -- are reproducible bit for bit on the host (tests/region_oracle.py). */

/* Lay out the members of the K regions of `labels` under the mask in force (d3d_set_data lays
 * them out again), allocate the series and -- what bit 0 -- the spectra, and start the moments
 * afresh (count 0).  Needs d3d_post_begin: D3D_ERR_STATE.  A tile ctx is D3D_ERR_UNSUPPORTED.  A
 * label outside 0..K, K < 1, capacity < 0 or what outside 0..1: D3D_ERR_INVALID.  An allocation
 * failure is D3D_ERR_HIP, frees what it got and leaves the ctx usable.  Whatever resets the moments
 * zeroes the series and the spectra; d3d_post_begin and d3d_post_end free them.  A ctx that never
 * calls it allocates and launches nothing for regions. */
int d3d_region_begin(d3d_ctx *ctx, const int32_t *labels, int K, int64_t capacity, int what);
/* *n = samples taken (the moments' count), *stored = rows of the series: min(n, capacity).  Either
 * may be NULL; both 0 without regions. */
int d3d_region_count(d3d_ctx *ctx, int64_t *n, int64_t *stored);
/* series (stored, K, 3) = F | C | S, spec_mean and spec_m2 (K, D) (variance = M2 / (n - 1)), sizes
 * (K) = members of every region.  Any may be NULL.  Spectra that were not begun: D3D_ERR_STATE. */
int d3d_region_get(d3d_ctx *ctx, double *series, double *spec_mean, double *spec_m2, int32_t *sizes);
/* Free them; the moments go on. */
int d3d_region_end(d3d_ctx *ctx);

/* ---- matched-filter line search ------------------------------------------ */
/* The reference starts every spaxel from a uniform draw inside the bounds (lib/run.py:310-314) and
 * its only mask helper thresholds the spectrally summed flux (lib/masks.py:17-29).  This entry
 * contracts every spaxel's prepared data d and 1/variance iv (as d3d_set_data leaves them: a NaN
 * voxel has d = 0, iv = 0) against a bank of templates T_k, k = i_w * n_c + i_c: the LSF-convolved
 * unit line of the ctx's line shape at (c, w) = (centres[i_c], widths[i_w]) -- the spectrum the
 * line kernels write for the parameters (1, c, w); the FSF is not involved --
 *     N_k = sum_z T_k[z] d[z] iv[z]    Q_k = sum_z T_k[z]^2 iv[z]    s_k = N_k / sqrt(Q_k) (0 if Q_k = 0)
 * best_out[y*W+x] = the lowest k attaining the maximum of s_k over the candidates with Q_k > 0 and
 * N_k > 0, or -1 when there is none or the spaxel is masked (the mask given to d3d_set_data; the
 * NaN rule is in iv); stat_out[(y*W+x)*4 ..] = {N_best, Q_best, s(i_w, i_c - 1), s(i_w, i_c + 1)},
 * NaN for a neighbour beyond the grid, four zeros where best = -1.  a = N/Q is the amplitude of the
 * best template, s the detection S/N.  host_bank (may be NULL): [n_w*n_c][D] templates evaluated by
 * the caller (a host LineModel), used instead of the device's; centres and widths then only give
 * the grid's shape.  The bank is built, used and freed inside the call; nothing of the chain's
 * state is written.  D3D_ERR_STATE before taps and data are set; D3D_ERR_UNSUPPORTED on a tile ctx
 * (d3d_set_tile) and for a bank above 256 MiB (n_w * n_c * D * 8 bytes: search fewer centres at a
 * time); D3D_ERR_INVALID for an empty grid, a width that is not positive, a value not finite. */
int d3d_line_search(d3d_ctx *ctx, int n_c, const double *centres, int n_w, const double *widths,
                    const double *host_bank, int32_t *best_out, double *stat_out);

/* ---- preparing a raw cube: continuum removal and channel noise ------------ */
/* The chain and d3d_line_search fit one line on a zero baseline, and without a variance cube the
 * reference takes ONE constant for the whole cube, median_clip(data[2:-2, 2:-4, 2:4], 2.5)
 * (lib/run.py:171-192; 1e12 is its "no information" variance, lib/run.py:180).  These entries remove
 * the continuum under the line and estimate the noise of every channel.  Host layout (D,H,W), fp64;
 * finite(v): neither NaN nor +-inf.  Both selections are exact; an even count n gives
 * (lo + hi) * 0.5 of the two middle order statistics, an odd one the middle one, n = 0 NaN
 * (numpy.nanmedian, bit for bit; -0.0 and 0.0 may come out as either).
 *
 * d3d_running_median: out[z,y,x] = the median of {cube[z',y,x] : max(0, z - half_window) <= z' <=
 * min(D - 1, z + half_window), valid[z',y,x]} -- the window shrinks at the ends and skips invalid
 * voxels; defined at every voxel, invalid ones included.  valid (may be NULL: finite(cube)):
 * (D,H,W) bytes, non-zero = valid; a NaN voxel is never valid.  1 <= half_window <= 128; a half
 * window of D or more is the whole spectrum.  The kernel counts ranks: O((2 half_window + 1)^2)
 * comparisons per voxel.
 *
 * d3d_channel_stats: over the spaxels with select[y*W+x] != 0 (NULL: all) and finite(cube[z,y,x]):
 * n_out[z] their count, m_out[z] their median, mad_out[z] the median of |cube[z,y,x] - m_out[z]|;
 * NaN, NaN, 0 where there is none.
 *
 * d3d_prepare: (1) valid0 = finite(cube), cont = running median of (cube, valid0), res = cube - cont;
 * (2) (m, mad, n) = channel statistics of (res, select), sigma_z = 1.4826 mad_z, NaN where n_z < 2
 * or mad_z == 0; (3) unless reject is NaN, ONE rejection pass: valid1 = valid0 & (|res| <= reject *
 * sigma_z) (a channel whose sigma is NaN rejects nothing), cont and res again with valid1, and (2)
 * again.  continuum_out, residual_out: (D,H,W); chan_out[z*3 ..] = {m_z, sigma_z, n_z}.  No cube
 * crosses to the host in between (the [D][3] statistics do).
 *
 * All three allocate and free everything inside the call, need neither taps nor data, and write
 * nothing of the chain's state (DATA, IVAR, ERR, SIM, parameters, RNG counters).
 * D3D_ERR_INVALID: half_window outside 1..128, reject zero or negative; D3D_ERR_UNSUPPORTED on a
 * tile ctx (d3d_set_tile). */
int d3d_running_median(d3d_ctx *ctx, const double *cube, const uint8_t *valid, int half_window, double *out);
int d3d_channel_stats(d3d_ctx *ctx, const double *cube, const uint8_t *select, double *m_out, double *mad_out,
                      int64_t *n_out);
int d3d_prepare(d3d_ctx *ctx, const double *cube, const uint8_t *select, int half_window, double reject,
                double *continuum_out, double *residual_out, double *chan_out);

/* ---- per-spaxel jump scales ---------------------------------------------- */
/* The reference proposes (c, w) of every spaxel with ONE Cauchy amplitude, jump_amplitude
 * (lib/run.py:251-262, 570-579), and its only acceptance feature is the stop rule on the pooled
 * rate (lib/run.py:344-364).  These entries keep one multiplicative scale per spaxel -- the
 * amplitudes of spaxel (y,x) are amp[] * scale[y,x] in every device kernel -- count every
 * spaxel's accepted proposals on the device, and, during burn-in, move each scale towards a
 * target acceptance rate.  Off until begun: a ctx that never calls d3d_adapt_begin allocates and
 * launches nothing for them and runs the chain it always ran, bit for bit. */

/* Allocate the scale map (all 1) and the counters (all 0).  After every `window`-th counted sweep
 * s of d3d_mh_sweeps / d3d_mh_sweeps_batch with s + sweep origin <= last_sweep (the run's
 * numbering, lib/run.py:344-353 cur_iteration; d3d_mh_set_sweep_origin), with k the number of
 * steps so far including this one, on the device:
 *     rate  = accepted[y,x] / window
 *     scale = clamp(scale * exp(gain / sqrt(k) * (rate - target)), scale_min, scale_max)
 *     accepted[y,x] = 0
 * Masked spaxels keep their scale.  After the last step the counters go on counting, so that
 * accepted / n_win (d3d_adapt_get) is the acceptance-rate map of the frozen chain.  window = 0:
 * a fixed map (d3d_adapt_set) that never adapts.  Calling it again starts afresh.
 * D3D_ERR_INVALID: target outside (0,1), window < 0, gain not positive, a scale range that is
 * not finite and positive or has scale_min > scale_max.  D3D_ERR_UNSUPPORTED: a tile ctx
 * (d3d_set_tile), or -- EXPERIMENTS builds -- option mh_chain, mh_flow or mh_pair, whose kernels keep
 * their proposals' inputs across sweeps (setting one later is refused alike).
 * d3d_mh_colour_lines draws its proposals on the host (lib/run.py:570-579 there): untouched. */
int d3d_adapt_begin(d3d_ctx *ctx, double target, int window, int64_t last_sweep, double gain,
                    double scale_min, double scale_max);
/* The (H,W) scale map, the (H,W) counters, the sweeps counted since the counters were last
 * cleared and the steps taken so far: accepted / n_win is the per-spaxel form of the rate the
 * reference pools over the cube (lib/run.py:344-364).  Any pointer may be NULL. */
int d3d_adapt_get(d3d_ctx *ctx, double *scale_hw, uint32_t *accepted_hw, int64_t *n_win, int64_t *k);
/* Install them (a resumed run continues the jump scales of lib/run.py:570-579 where the
 * checkpoint left them; with window = 0 a caller-given fixed map).  Either map may be NULL: kept.
 * A scale that is not finite and positive, or a negative n_win / k: D3D_ERR_INVALID. */
int d3d_adapt_set(d3d_ctx *ctx, const double *scale_hw, const uint32_t *accepted_hw, int64_t n_win,
                  int64_t k);
/* Free the maps: the ctx proposes with the one amplitude of lib/run.py:251-262 again
 * (d3d_ctx_destroy does it too). */
int d3d_adapt_end(d3d_ctx *ctx);

/* ---- smoothness prior between neighbouring spaxels ------------------------ */
/* The reference samples a flat prior inside the bounds, every spaxel on its own: its MH ratio is
 * the likelihood's alone (lib/run.py:426-438) and its Gibbs draw sees only the prior variance ra
 * (lib/run.py:491-496).  Where the FSF is wider than a spaxel, neighbours trade flux and the
 * parameter maps are noise.  These entries add a pairwise Gaussian prior between 4-neighbours,
 *     log p(theta) = -1/2 sum_<i,j> sum_k lam[k] (theta_i,k - theta_j,k)^2,   k = (a, c, w),
 * over the horizontally and vertically adjacent pairs of unmasked spaxels (mask == 1).  Off until
 * begun: a ctx that never calls d3d_prior_begin runs the chain it always ran, bit for bit. */

/* Turn the prior on with lam[k] = 1 / sigma_k^2 >= 0 (0: none on that parameter).  With N(i) the
 * unmasked 4-neighbours of spaxel i inside the cube, as they are when i is decided, every update of
 * every device kernel then compares (lib/run.py:426-438)
 *     delta = (ar_old - ar_new)
 *             - 1/2 sum_{j in N(i)} sum_{k in (c,w)} lam[k] (p_new,k - p_old,k)(p_new,k + p_old,k - 2 theta_j,k)
 * with log(u) -- d3d_get_dlog and the dlog of d3d_mh_sweeps hold this total -- and draws the
 * amplitude (lib/run.py:491-496) from
 *     s_ee' = s_ee + lam[0] |N(i)|,  s_eu' = s_eu + lam[0] sum_{j in N(i)} a_j,
 *     ro = ra / (1 + ra s_ee'),  mu = ro s_eu',  r ~ TN(min_a, max_a; mu, sqrt(ro)).
 * Random numbers and the residual update are unchanged; all lam = 0 is the chain without the
 * prior, bit for bit.  Two spaxels of one colour class are fh rows or fw columns apart, so no
 * neighbour moves in the launch that decides i: exact for every fh, fw >= 2.  Calling it again
 * replaces lam.
 * D3D_ERR_INVALID: a lam that is negative or not finite; fh == 1 or fw == 1 (adjacent spaxels
 * would share a colour class).  D3D_ERR_UNSUPPORTED: a tile ctx (d3d_set_tile), a ctx cut into
 * more than one part (d3d_set_parts), or -- EXPERIMENTS builds -- option mh_chain, mh_flow or
 * mh_pair, whose kernels decide more than one colour class in a launch; each of these, and
 * d3d_mh_colour_lines, is refused alike while the prior is on.  The ctxs of one
 * d3d_mh_sweeps_batch call must all have the prior on or all off (D3D_ERR_INVALID; their lam may
 * differ).  d3d_window_stats keeps returning
 * the likelihood terms only. */
int d3d_prior_begin(d3d_ctx *ctx, const double lam[3]);
/* lam as begun (zeros when off) and whether the prior is on: what the MH ratio of
 * lib/run.py:426-438 is extended by. */
int d3d_prior_get(d3d_ctx *ctx, double lam[3], int *on);
/* Turn it off: the ctx samples the flat prior of lib/run.py:426-438, 491-496 again. */
int d3d_prior_end(d3d_ctx *ctx);
/* E_k = sum_<i,j> (theta_i,k - theta_j,k)^2 over the pairs above for k = (a, c, w), and their
 * number: -2 log p = sum_k lam[k] E_k, the term the ratio of lib/run.py:426-438 is extended by.
 * params: an (H,W,3) map on the host, or NULL for the ctx's current parameters.  Summed on the
 * device in fp64 in a fixed order: two calls return the same bits.  Works with the prior off. */
int d3d_prior_energy(d3d_ctx *ctx, const double *params, double energy[3], int64_t *pairs);

/* ---- replica exchange between tempered chains ----------------------------- */
/* The reference runs one chain whose MH ratio is the likelihood's (lib/run.py:426-438): between
 * two modes of c -- a wrong line, a neighbour's line, a noise spike -- it does not cross.  These
 * entries generalise that ratio to parallel tempering: n ctxs of ONE geometry (as
 * d3d_mh_sweeps_batch takes them) sample L^beta_r x prior at inverse temperatures
 * 1 = beta_0 > beta_1 > ... > beta_{n-1}, and adjacent rungs trade their states with a Metropolis
 * rule that leaves every rung's tempered posterior invariant.  The tempered posterior is the same
 * model with the variance divided by beta: the caller gives rung r d3d_set_data(data, var /
 * beta_r) and no sweep kernel changes -- the MH log-ratio of lib/run.py:426 scales by beta, the
 * Gibbs draw of lib/run.py:491-496 becomes ro = ra / (1 + ra beta sum ek^2/var), mu = ro beta sum
 * ek ul/var, the priors (ra, bounds, d3d_prior_begin) stay untempered.  A ctx that never joins a
 * group allocates and launches nothing new. */
typedef struct d3d_temper d3d_temper;

/* A group over ctxs[0..n), rung r at betas[r].  D3D_ERR_INVALID: n outside 2..64; betas[0] != 1,
 * betas not strictly decreasing, finite and > 0; a ctx that is NULL, appears twice, or differs
 * from ctxs[0] in device, shape, mask, FSF, LSF, line shape or line table (the comparisons of
 * d3d_mh_sweeps_batch).  D3D_ERR_UNSUPPORTED: a tiled, partitioned or communicator ctx, or one
 * driven by d3d_mh_colour_lines.  D3D_ERR_STATE: taps or data not set.  seed keys the swaps'
 * uniforms.  Allocates one small device block (energies, block partials, flags, counters,
 * labels; labels[r] = r).  Destroy the group before any of its ctxs. */
int d3d_temper_create(d3d_temper **t, d3d_ctx **ctxs, int n, const double *betas, uint64_t seed);
/* One exchange round, asynchronous, on ctxs[0]'s stream (every ctx's own stream is synchronised
 * first and its pending residual layers are written back, as d3d_mh_sweeps_batch does).  Every
 * ctx needs a valid carried residual (D3D_ERR_STATE).  Three launches with nothing but device
 * memory between them:
 *   1. E_r = (sum_v 1/2 err_r[v]^2 / var_r[v]) / betas[r]: minus log L of state r under the
 *      untempered variance, summed in fp64 in a fixed order (no floating-point atomics: a run
 *      reproduces under its seed);
 *   2. for the pairs (i, i+1) with i = round mod 2 (mod 2): u = the first uniform of Philox4x32-10
 *      at counter {0xFFFFFFFF, (uint32_t)round, i, 1} under the group's seed (the chains' streams
 *      have a last counter word of 0; only the low 32 bits of round enter the counter, so rounds
 *      2^32 apart draw the same uniforms, while both 32-bit words of the seed key them),
 *      accepted iff log(u) < (betas[i] - betas[i+1]) (E_i -
 *      E_{i+1}); attempts, accepts and labels follow, and E_r -- of the state at rung r before the
 *      exchange -- enters rung r's running (n, mean, M2);
 *   3. an accepted pair trades SLOT_ERR (the raw padded buffer) and the (H,W,3) parameters,
 *      nothing else: data, 1/variance, jump scales and their counters, accepted counters,
 *      posterior accumulators, the log ratios of d3d_get_dlog and the seed belong to the RUNG.
 * Afterwards every ctx's proposal table is stale (as after d3d_set_params) and its residual still
 * valid; work enqueued later on the other ctxs' streams waits, on the device, for the exchange. */
int d3d_temper_swap(d3d_temper *t, int64_t round);
/* Rounds so far, attempts / accepts per pair [n-1], the energy moments per rung [n] (count, mean,
 * sum of squared deviations) and labels [n]: labels[r] is the rung the state now at rung r
 * started from.  Any pointer may be NULL.  Waits for the stream. */
int d3d_temper_get(d3d_temper *t, int64_t *rounds, int64_t *attempts, int64_t *accepts,
                   int64_t *energy_n, double *energy_mean, double *energy_m2, int32_t *labels);
/* The last round: energy [n]; u, logu [n-1] (NaN for a pair not proposed); decided [n-1] (1
 * accepted, 0 rejected, -1 not proposed).  Any pointer may be NULL.  Waits for the stream.
 * D3D_ERR_STATE before the first round. */
int d3d_temper_last(d3d_temper *t, double *energy, double *u, double *logu, int32_t *decided);
/* Exchange PATCHES of spaxels instead of whole cubes.  The energy gap of two rungs grows with the
 * parameters of the whole field, so whole-cube swaps need a ladder as fine as sqrt(2 / parameters);
 * a patch of p x p spaxels carries 3 p^2 parameters and its energy difference lives in the patch
 * dilated by the FSF, so a coarse ladder swaps.  p = 0 (the default): whole cubes, exactly the three
 * launches above.  p >= 1: later d3d_temper_swap calls run the rule below.  D3D_ERR_INVALID below 0
 * (and above 2^24).
 * The device block of the per-tile record is allocated by the first patch round.
 *
 * A patch round of rungs i, j = i + 1 (the pairs of the round's parity, as above):
 *   tiles     (oy, ox) = (w0 mod p, w1 mod p), w = Philox4x32-10 at {0xFFFFFFFE, (uint32_t)round, 0, 1}
 *             under the group's seed; spaxel (y, x) lies in tile (ty, tx) = ((y + p - oy) / p,
 *             (x + p - ox) / p); nty = (H - 1 + p - oy) / p + 1, ntx likewise.  A PATCH P is the set
 *             of unmasked spaxels of one tile; a tile without one is not proposed.
 *   colours   my = 1 + ceil((fh - 1) / p), mx = 1 + ceil((fw - 1) / p): the tiles with
 *             (ty mod my, tx mod mx) = (cy, cx) have disjoint FSF-dilated footprints (and for fh, fw
 *             >= 3 are not adjacent).  One launch per colour, in ascending cy mx + cx; one workgroup
 *             per (tile, pair), which decides by itself.
 *   proposal  trade the parameters of P.  delta = sum_{s in P} [contribution(s, x_i[s]) -
 *             contribution(s, x_j[s])] (the LSF-convolved line times the FSF: a contribution at
 *             (y + dy, x + dx) carries fsf[fhh + dy, fhw + dx]); e_i' = e_i + delta, e_j' = e_j - delta.
 *   ratio     Delta = (-(t0 + t2) - (t3 - t1)) + t4 with the five terms t0 = sum ivar_i e_i delta,
 *             t1 = sum ivar_j e_j delta, t2 = 1/2 sum ivar_i delta^2, t3 = 1/2 sum ivar_j delta^2 (ivar_r
 *             the rung's own 1/variance, beta_r / var) and t4 = Delta_prior: with d3d_prior_begin on
 *             (every rung the same lam, D3D_ERR_INVALID otherwise), over the adjacent pairs <s, t> with
 *             s in P, t unmasked outside the tile, -1/2 sum_k lam_k [(x_j[s] - x_i[t])^2 - (x_i[s] -
 *             x_i[t])^2 + (x_i[s] - x_j[t])^2 - (x_j[s] - x_j[t])^2]; 0 with the prior off.  Bounds and
 *             ra cancel.  Sums in fp64 in a fixed order, no floating-point atomics.
 *   decision  u = the first uniform of Philox at {0xFFFFFFFF, (uint32_t)round, i, 2 + ty ntx + tx}
 *             (word 1 is the whole-cube swap, word 0 the chains); accepted iff log(u) < Delta.  Then
 *             e_i += delta, e_j -= delta and the (a, c, w) of the spaxels of P trade places.
 * The round still computes E_r and folds it -- of the state before the exchange -- into the rungs'
 * moments, but takes no whole-cube decision: d3d_temper_last reports every pair as not proposed,
 * the whole-cube attempts / accepts stand still, and labels stay as created (states no longer
 * travel whole).  Every rung's SLOT_TMP0 is overwritten (the lines of the round). */
int d3d_temper_set_patch(d3d_temper *t, int p);
/* The last round, when it was a patch round (D3D_ERR_STATE otherwise): geometry = {oy, ox, nty,
 * ntx, my, mx}; per (pair i, tile ty ntx + tx), i major: terms [n-1][nty ntx][5] = t0 .. t4 above,
 * u, logu [n-1][nty ntx] and decided [n-1][nty ntx] (1 accepted, 0 rejected, -1 not proposed: the
 * other parity, or no unmasked spaxel; NaN terms, u, logu there).  Any pointer may be NULL: ask for
 * the geometry first to size the rest.  Waits for the stream. */
int d3d_temper_last_patches(d3d_temper *t, int32_t geometry[6], double *terms, double *u, double *logu,
                            int32_t *decided);
/* Patches proposed and accepted per pair [n-1] since the group was made (zeros before the first
 * patch round).  Any pointer may be NULL.  Waits for the stream. */
int d3d_temper_get_patches(d3d_temper *t, int64_t *attempts, int64_t *accepts);
int d3d_temper_destroy(d3d_temper *t);

/* ---- spatial tiling (one chain over several GPUs) --------- */
/* The reference has no counterpart (single process).  What makes tiling possible is
 * that an update at (y,x) touches only its FSF window (lib/run.py:404-419), and that
 * the scan order is overridable (lib/run.py:553-560).
 *
 * A TILE ctx holds a sub-region of the global cube: the spaxels it owns plus a
 * frame.  Random numbers and colour classes are keyed by GLOBAL coordinates.  The
 * owned spaxels are cut into PARTS (rectangles), each with a PHASE number: a sweep
 * runs the phases in order, and within a phase every part runs its fh*fw colour
 * launches.  Parts of one phase -- on this GPU or on others -- are chosen so that
 * their windows are disjoint (deconv3d_amd/tiling.py), so a phase runs on every
 * GPU at once with no communication, and after it each GPU sends the residual
 * cells it changed that a neighbour also holds: a bulk HALO copy per phase (2-4
 * per sweep, a few MB each) instead of an exchange per colour class.  The tiled
 * chain is bit-identical to a single ctx given the same parts (d3d_set_parts). */

/* Declare this ctx a tile: its (H,W) cube is the region starting at global
 * (gy0,gx0) of a cube Wg spaxels wide; it owns local rows [oy0,oy1) and columns
 * [ox0,ox1) (other spaxels are never updated here).  Call before d3d_set_data. */
int d3d_set_tile(d3d_ctx *ctx, int gy0, int gx0, int Wg, int oy0, int oy1, int ox0, int ox1);
/* Cut the owned spaxels into nparts rectangles rects[4*i..] = {y0,y1,x0,x1} (local,
 * disjoint, inside the owned rectangle) with phases[i] in [0,16).  nparts = 0
 * restores the single part.  Spaxels in no part are not updated. */
int d3d_set_parts(d3d_ctx *ctx, int nparts, const int *rects, const int *phases);
/* Several independent chains of ONE geometry in one launch per colour class (the ensemble of
 * BASELINE config 5 on one device; lib/run.py has one chain per Run(), its sweep loop is
 * lib/run.py:344-537).  ctxs[0..n_ctx): contexts on one device with the same shape, mask, FSF and
 * LSF (data, variance values, bounds, parameters, seed may all differ), unpartitioned, at
 * most 256 channels.  Every chain is the chain d3d_mh_sweeps would produce for its ctx alone
 * (same kernels, same random streams); a small cube's colour launch, which alone leaves the chip
 * idle, carries n_ctx times the windows for the same latency.  keep_one_in, chain_out[n_ctx],
 * dlog_out[n_ctx] (arrays of per-chain pointers, or NULL; a NULL entry skips that chain): as in
 * d3d_mh_sweeps, per chain.  accepted[n_ctx] (may be NULL): accepted proposals per chain. */
int d3d_mh_sweeps_batch(d3d_ctx **ctxs, int n_ctx, int n_sweeps, int first_sweep, int keep_one_in,
                        double **chain_out, double **dlog_out, int64_t *accepted);
/* One phase of sweep `sweep`: every colour class of every part of that phase
 * (lib/run.py:367-519 restricted to them).  For callers that exchange the halos
 * themselves (loop-back, host-staged transports); d3d_mh_sweeps does whole sweeps
 * including the exchange once d3d_comm_init was called. */
int d3d_mh_phase(d3d_ctx *ctx, int phase, int sweep);
/* Accepted proposals since the counter was last reset (d3d_mh_sweeps resets it). */
int d3d_mh_accepted(d3d_ctx *ctx, int64_t *count, int reset);
/* Write pending (deferred) residual updates into SLOT_ERR now. */
int d3d_flush(d3d_ctx *ctx);

/* Halo plan `plan` (0..15: after that phase; D3D_PLAN_PARAMS: the parameter gather
 * before a from-scratch residual, lib/run.py:521-534): n entries of 10 ints
 * {peer rank, kind (0 residual cells, 1 parameter map), send rectangle y0,y1,x0,x1,
 * receive rectangle y0,y1,x0,x1} in local coordinates (an empty rectangle = none). */
#define D3D_PLAN_PARAMS 16
int d3d_halo_plan(d3d_ctx *ctx, int plan, int n, const int *entries);
/* RCCL transport: rank 0 draws a unique id (D3D_COMM_UID_BYTES bytes), every rank
 * passes it to d3d_comm_init (ncclCommInitRank on the ctx's device).  Then
 * d3d_halo_exchange(plan) = pack the send rectangles, ncclSend/ncclRecv them inside
 * one ncclGroupStart/End on the ctx stream (point-to-point: one xGMI link per
 * neighbour, no ring), unpack -- device buffers only, no host synchronisation. */
#define D3D_COMM_UID_BYTES 128
int d3d_comm_unique_id(void *uid);
int d3d_comm_init(d3d_ctx *ctx, int nranks, int rank, const void *uid);
int d3d_comm_destroy(d3d_ctx *ctx);
int d3d_halo_exchange(d3d_ctx *ctx, int plan);
/* What RCCL itself reports for the ctx's communicator (ncclCommCount, ncclCommUserRank):
 * how many ranks actually joined, and which one this is (bench.py's tiled record). */
int d3d_comm_info(d3d_ctx *ctx, int *nranks, int *rank);
/* With option halo_timing = 1, d3d_mh_sweeps brackets every halo exchange (pack, RCCL
 * send/recv, unpack; lib/run.py has no counterpart: the reference is one process) with
 * HIP events on the ctx stream: *ms = their summed duration since the last reset,
 * *count (may be NULL) = how many exchanges that was. */
int d3d_halo_time(d3d_ctx *ctx, double *ms, long *count, int reset);
/* The same exchange in steps, for other transports: pack the send rectangles into
 * the plan's device send buffer / scatter the device receive buffer; device
 * pointers and sizes of one entry's buffers; host staging of one entry;
 * a device-to-device copy queued on ctx's stream (loop-back between contexts). */
int d3d_halo_pack(d3d_ctx *ctx, int plan);
int d3d_halo_unpack(d3d_ctx *ctx, int plan);
int d3d_halo_buffers(d3d_ctx *ctx, int plan, int entry, void **send_ptr, size_t *send_bytes,
                     void **recv_ptr, size_t *recv_bytes);
int d3d_halo_download(d3d_ctx *ctx, int plan, int entry, double *host);
int d3d_halo_upload(d3d_ctx *ctx, int plan, int entry, const double *host);
int d3d_device_copy(d3d_ctx *ctx, void *dst, const void *src, size_t bytes);

/* Number of owned unmasked spaxels of global colour (cy,cx) = ((y+gy0) mod fh,
 * (x+gx0) mod fw), colour = cy*fw + cx. */
int d3d_colour_count(d3d_ctx *ctx, int colour, int *count);
/* One colour class of sweep `sweep` over every part, residual written back
 * immediately (per-colour stepping for tests and probes). */
int d3d_mh_colour(d3d_ctx *ctx, int colour, int sweep);
/* Per-update records, the finer-grained alternative to the halo copies: {global y,
 * global x, a,c,w before, a,c,w after} of the last update of the n listed local
 * spaxels (y*W+x), out[n*8] ... */
int d3d_export_updates(d3d_ctx *ctx, int n, const int *spaxels, double *out);
/* ... and their replay on another ctx: the first two entries are LOCAL coordinates
 * of this tile (they may lie outside it); err += f*G on the window's part inside. */
int d3d_apply_updates(d3d_ctx *ctx, int n, const double *records);

/* ---- Student-t likelihood: per-voxel noise weights ------------------------- */
/* The reference's likelihood is Gaussian with a known variance (lib/run.py:171-192 sets it up,
 * lib/run.py:407-426 is its chi2 over the window).  A Student-t error with nu degrees of freedom is
 * that Gaussian with the variance of voxel v divided by a latent weight lambda_v ~ Gamma(nu/2, rate
 * nu/2); given the residual r_v (SLOT_ERR) and the base 1/variance i0_v (what d3d_set_data left in
 * SLOT_IVAR) the weights are independent,
 *     lambda_v | r_v ~ Gamma(shape (nu + 1) / 2, rate (nu + r_v^2 i0_v) / 2),
 * and given the weights the chain is the per-voxel-variance chain of lib/run.py:407-426 with
 * SLOT_IVAR[v] = lambda_v i0_v.  These entries redraw the weights on the device between sweeps: an
 * exact Gibbs step that leaves single voxels tens of sigma off (cosmic rays, sky-line residuals)
 * without pull on the lines.  Off until begun: a ctx that never calls d3d_robust_begin allocates
 * and launches nothing for them and runs the chain it always ran, bit for bit.
 *
 * The draw, in fp64 without contraction, m = (nu + 1) / 2 (integer division):
 *     g      = -log(u_0 * u_1 * ... * u_{m-1})           (the product from the left)
 *     g      = g + (-log(u_m)) * cos(6.283185307179586 * u_{m+1})^2     (nu even only)
 *     lambda = (2 g) / (nu + (r r) i0)
 * u_{2b}, u_{2b+1} are the two uniforms of Philox4x32-10 with the key of d3d_mh_config's seed and
 * the counter (voxel, sweep number, b, 0x52425354), voxel = z H W + y W + x, the sweep number in
 * the run's numbering (d3d_mh_set_sweep_origin): no rejection, nothing of the layout, the padding,
 * the launch geometry or the options enters.  Where i0 == 0 (NaN voxels) SLOT_IVAR gets 0. */

/* Arm: keep a copy of SLOT_IVAR as the base cube and a zeroed weight mean (two more cubes of
 * device memory).  From then on d3d_mh_sweeps / d3d_mh_sweeps_batch redraw the weights after every
 * sweep s (the run's numbering) with s >= start and (s - start) % every == 0 -- after the
 * snapshot, the posterior sample, the adaptation step and the from-scratch residual of
 * lib/run.py:521-534, with the pending residual updates written back first -- and a draw of a
 * sweep s >= accumulate_from also enters the running mean of the weights.  Until the first draw
 * SLOT_IVAR holds the base cube's bits; d3d_variance_is_uniform answers 0 while armed (the
 * per-voxel kernels run; they are bit-identical to the uniform ones on a constant cube).
 * d3d_chi2_map, the log ratios and d3d_window_stats are those of the conditional Gaussian
 * under the current weights.  Calling it again starts afresh from the base cube.
 * D3D_ERR_INVALID: nu outside 1..30, every < 1, a negative sweep.  D3D_ERR_STATE: no data.
 * D3D_ERR_UNSUPPORTED: a tile ctx (d3d_set_tile), or D*H*W >= 2^32.  While armed d3d_set_data,
 * d3d_set_tile and writes into SLOT_IVAR are refused. */
int d3d_robust_begin(d3d_ctx *ctx, int nu, int every, int64_t start, int64_t accumulate_from);
/* One draw now, as the one after sweep `sweep_number` (the run's numbering) would be, from the
 * residual of the current parameters (lib/run.py:317-334; pending updates written back first):
 * for tests, and for a resumed run, which re-makes the last due draw of the checkpointed run. */
int d3d_robust_step(d3d_ctx *ctx, int64_t sweep_number);
/* (D,H,W) arrays: the current weights SLOT_IVAR / base (1 before the first draw) and the running
 * mean of the accumulated draws (0 before the first), NaN where the voxel carries no information
 * (base 1/variance 0: lib/run.py:423-424's nansum skips it); *count the accumulated draws.  Any
 * pointer may be NULL. */
int d3d_robust_get(d3d_ctx *ctx, double *weights, double *weight_mean, int64_t *count);
/* Disarm: the base cube goes back into SLOT_IVAR bit for bit, d3d_variance_is_uniform answers as
 * before d3d_robust_begin, the two cubes are freed: the Gaussian chain of lib/run.py:171-192's
 * variance again (d3d_ctx_destroy does it too). */
int d3d_robust_end(d3d_ctx *ctx);

/* ---- pointwise predictive accuracy: lppd and WAIC per voxel ---------------- */
/* The reference scores one state of the chain (lib/run.py:407-426 is its chi2 over a window,
 * lib/run.py:423 the sum d3d_chi2_map maps): that neither scores the posterior nor penalises
 * flexibility, and under d3d_robust_begin it is the conditional Gaussian's, not the Student-t's.
 * These entries keep, over the samples of the posterior moments (d3d_post_*), what the widely
 * applicable information criterion needs of every voxel v:
 *     lppd_v = log mean_s p(y_v | theta_s)        p_v = var_s log p(y_v | theta_s)
 * elpd = sum_v (lppd_v - p_v), WAIC = -2 elpd.  With r the residual (SLOT_ERR) and i0 the base
 * 1/variance (d3d_set_data's SLOT_IVAR; under d3d_robust_begin the copy the weights keep, never the
 * reweighted slot) log p = k_v + q_sv, k_v constant over the chain:
 *     Gaussian      q = -1/2 (r r) i0                      k = 1/2 log(i0) - 1/2 log(2 pi)
 *     Student-t     q = -((nu + 1)/2) log1p((r r) i0 / nu)
 *                   k = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) + 1/2 log(i0)
 * (the Student-t marginal: the weight integrated out).  Only q is accumulated, into four cubes:
 * M = max_s q, S = sum_s exp(q - M), and Welford's mean and M2 of q; with n samples
 *     lppd_v = (k_v + M_v) + log(S_v / n)         p_v = M2_v / (n - 1)   (NaN for n < 2).
 * The update of sample number n, in fp64 without contraction (the first sample sets M = q, S = 1):
 *     d = q - M;  e = exp(-fabs(d));
 *     S = (d <= 0) ? S + e : S * e + 1;   M = (d <= 0) ? M : q;   then Welford's step of (mean, M2).
 * No term of S exceeds 1, whatever the order of good and bad samples.  A voxel counts iff i0 != 0,
 * at masked spaxels too (the set d3d_chi2_map sums); NaN voxels and the pad channel never do.  Off
 * until begun: a ctx that never calls d3d_pred_begin allocates and launches nothing for it. */

/* Arm (lib/run.py:407-426's likelihood, per voxel): four zeroed cubes of device memory; the moments
 * start afresh (as d3d_hist_begin) and from then on every sample of theirs -- d3d_post_accumulate, the
 * sweeps of d3d_post_schedule -- is also one of these, made from the residual of the sample's state
 * (rebuilt when not valid, pending updates written back first).  The likelihood is the one in force
 * now: Student-t with d3d_robust_begin's nu when the weights are armed (arm them first), else
 * Gaussian; a sample after the weights were armed, disarmed or given another nu is D3D_ERR_STATE.
 * D3D_ERR_STATE: d3d_post_begin not called.  D3D_ERR_UNSUPPORTED: a tile ctx (d3d_set_tile).
 * D3D_ERR_HIP: the four cubes do not fit; the ctx stays usable.  d3d_post_begin / d3d_post_end free
 * them, d3d_set_data zeroes them with the moments. */
int d3d_pred_begin(d3d_ctx *ctx);
/* Samples accumulated (lib/run.py:407-426 evaluated that many times per voxel): d3d_post_count's
 * number, 0 when not begun. */
int d3d_pred_count(d3d_ctx *ctx, int64_t *n);
/* The raw accumulators of q (lib/run.py:407-426 without its constants) as (D,H,W) arrays, 0 where
 * the voxel is not counted; chains are pooled from these (M = max M_r, S = sum S_r exp(M_r - M),
 * Chan's merge of mean and M2).  Any pointer may be NULL. */
int d3d_pred_get(d3d_ctx *ctx, double *M, double *S, double *mean, double *m2);
/* maps (H,W,4) = {sum_z lppd_v, sum_z p_v, counted voxels, sum_z (lppd_v - p_v)^2} of every spaxel
 * (per spectrum, as lib/run.py:407-426 sums its chi2), folded on the device in a fixed order: lane l of
 * 64 takes the channel pairs l, l + 64, ..., then the lanes fold by halves -- the same bits on every
 * call.  The standard error of elpd is sqrt(N var_v(lppd_v - p_v)) from the first, second and last. */
int d3d_pred_maps(d3d_ctx *ctx, double *maps);
/* lppd_v and p_v as (D,H,W) arrays, NaN where the voxel is not counted (the nansum of
 * lib/run.py:407-426 skips it); through SLOT_TMP0.  Either pointer may be NULL. */
int d3d_pred_cubes(d3d_ctx *ctx, double *lppd, double *p);
/* Free the four cubes; the moments go on (lib/run.py:407-426's chain is untouched throughout). */
int d3d_pred_end(d3d_ctx *ctx);

/* ---- noise-scale inference: variance factors of channel groups ------------- */
/* The reference takes the variance as known (lib/run.py:171-200: the given cube, or one constant
 * from a corner of the data) and sums r^2 / variance over every window (lib/run.py:407-426).  Here
 * every channel z belongs to a group group[z] in 0 .. G-1 (-1: never rescaled) and the variance of
 * its voxels is s_g variance_v, s_g ~ InvGamma(shape a0, rate b0) (a0 = b0 = 0: Jeffreys' 1/s).
 * With i0_v the base 1/variance (what d3d_set_data left in SLOT_IVAR), a voxel counts iff i0_v != 0,
 * group[z] >= 0 and its spaxel is in the 0/1 map `spaxels` (NULL: every spaxel, masked ones too: the
 * set d3d_pred_begin counts).  N_g the counted voxels and Q_g = sum (r_v r_v) i0_v over them,
 *     tau_g = 1 / s_g | r ~ Gamma(shape a0 + N_g / 2, rate b0 + Q_g / 2),
 * an exact Gibbs step, after which SLOT_IVAR[v] = i0_v tau_group[z] -- always from the base cube,
 * never in place -- and the sweep kernels run unchanged.  Channels of group -1 and groups with
 * N_g < 2 keep tau = 1 (the latter are reported as NaN); a rate of exactly 0 keeps the previous tau.
 *
 * The sums, in fp64 without contraction, in one fixed order whatever the chip, the launch geometry,
 * the options and the padding: stream j of 1024 adds, per channel, the counted terms of the spaxels
 * j, j + 1024, ... (spaxel = y W + x) one after the other from 0; the 1024 partials of a channel are
 * added in index order from 0; the channels of a group in increasing z from 0.
 * The draw (Marsaglia and Tsang), alpha = a0 + 0.5 N_g, d = alpha - 1/3, c = 1 / sqrt(9 d): attempt
 * t = 0 .. 15 takes (u1, u2) = the two uniforms of Philox4x32-10 block 2t and u3 = the first of block
 * 2t + 1, key d3d_mh_config's seed, counter (g, sweep number, block, 0x4E4F4953), the sweep number in
 * the run's numbering (d3d_mh_set_sweep_origin);
 *     x = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2);  v = 1 + c x;  rejected when v <= 0;
 *     v = v v v;  accepted iff log(u3) < 0.5 x x + d - d v + d log(v);  then gamma = d v,
 * and gamma = d when no attempt of the 16 is accepted (probability below 1e-20 for alpha >= 1);
 *     tau_g = gamma / (b0 + 0.5 Q_g).
 * Off until begun: a ctx that never calls d3d_noise_begin allocates and launches nothing for it. */

/* Arm (lib/run.py:171-200's variance becomes the base of a scaled one; lib/run.py:407-426's sums
 * run on the scaled one): a copy of SLOT_IVAR as the base cube, 1024 x Dp partials and a series of
 * `capacity` rows of G scales on the device.  From then on d3d_mh_sweeps / d3d_mh_sweeps_batch redraw
 * after every sweep s (the run's numbering) with s >= start and (s - start) % every == 0 -- last,
 * after the snapshot, the posterior sample, the adaptation step and the from-scratch residual, with
 * the pending residual updates written back first -- on the context's stream, no host round trip.
 * d3d_variance_is_uniform answers 0 while armed.  d3d_chi2_map and the log ratios are those of the
 * conditional Gaussian under the current scales.  Calling it again starts afresh from the base cube.
 * Refused before any allocation -- D3D_ERR_UNSUPPORTED: a tile ctx, d3d_robust_begin or
 * d3d_pred_begin armed, a member of a tempering group; D3D_ERR_INVALID: G < 1, a label outside
 * -1 .. G-1, a negative shape, rate or start, every < 1, capacity < 1; D3D_ERR_STATE: no data.
 * A due draw with the series full fails with D3D_ERR_STATE.  While armed d3d_set_data, d3d_set_tile,
 * d3d_robust_begin, d3d_pred_begin, d3d_temper_create and writes into SLOT_IVAR are refused. */
int d3d_noise_begin(d3d_ctx *ctx, const int32_t *group /*D*/, int G, const uint8_t *spaxels /*H*W or NULL*/,
                    double shape, double rate, int every, int64_t start, int64_t capacity);
/* One draw now, as the one after sweep `sweep_number` (the run's numbering) would be, from the
 * residual as it is (lib/run.py:407-426's r; rebuilt when not valid, pending updates written back
 * first; the variance lib/run.py:171-200 set up is its base), one more row of the series; then
 * synchronises.  For tests, and for a resumed run, which re-makes the last due draw. */
int d3d_noise_step(d3d_ctx *ctx, int64_t sweep_number);
/* Rows of the series so far (draws of the variance factor of lib/run.py:171-200's variance, summed
 * as lib/run.py:407-426 does). */
int d3d_noise_count(d3d_ctx *ctx, int64_t *draws);
/* series (draws, G): the scales s_g = 1 / tau_g of every draw (NaN: N_g < 2); sweeps (draws): the
 * sweep number of every row; voxels (G) and last_sum (G): N_g and Q_g of the last draw (the sums of
 * lib/run.py:407-426 per group, on the base variance of lib/run.py:171-200); tau (D): the factor
 * SLOT_IVAR carries in every channel now.  Any pointer may be NULL. */
int d3d_noise_get(d3d_ctx *ctx, double *series /*draws*G*/, int64_t *sweeps /*draws*/, double *voxels /*G*/,
                  double *last_sum /*G*/, double *tau /*D*/);
/* Disarm: the base cube goes back into SLOT_IVAR bit for bit, d3d_variance_is_uniform answers as
 * before d3d_noise_begin, the buffers are freed: the chain of lib/run.py:171-200's variance again,
 * summed as in lib/run.py:407-426 (d3d_ctx_destroy frees them too). */
int d3d_noise_end(d3d_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DECONV3D_HIP_H */
