"""
Every kernel variant the dispatcher of the MH sweep can pick in the default build (d3d_mh.hip:
launch_mh_ws, launch_mh_small, launch_mh_zb_t, launch_mh_batch_t, launch_mh_defer, launch_mh), on
the smallest cube that reaches it.  One table, ROWS: a row gives a geometry, a depth, options, and
the fields of the read-only option `mh_path` (family, NS, U, M, K and the flags NTV, UV, prior,
multi: include/deconv3d_hip.h, D3D_MH_*) the row must produce.  Every row

  * runs SWEEPS sweeps and compares them update by update with the oracle, which is fed the
    device's initial residual, with the tolerances of tests/test_gpu_full_size_oracle.py
    (parameters and the log-ratio map rel 1e-9, carried residual 1e-11 of its peak, accepted
    counts equal).  The oracle run of a problem is shared by the rows that differ only in the
    kernel they ask for;
  * asserts the decoded `mh_path`, the pending-layer counts the launches found
    (`mh_path_layers`) and `mh_strips_on`;
  * where the project promises identity -- the beyond-cache policy (NTV) against the default one
    of the same row, and 1, 2 and 3 pending layers at Dp <= 160 -- compares the chains bit for bit.

Which side of the chip-filling threshold a geometry lies on is computed here, from the device's
number of compute units (the read-only option `device_cus`: what the dispatcher itself asked the
runtime for when the context was made): a colour launch
"fills the chip" from 2 workgroups per CU on, the windows of its colour class, virtual positions
(up to one period outside the cube) included -- times the 256-channel blocks for the z-blocked
kernels, times the chains for a batched launch.  A row states the side it was made for (`fill`:
True, False, or "mixed" -- the colour with the most windows fills the chip, the LAST colour of a
sweep does not); a geometry that lies elsewhere fails the row: change the shape.

Geometries (the numbers assume the 256 CUs of an MI355X, threshold 512):
  fill   69 x 69, 3 x 3 taps:  23 .. 24 lattice points per axis, 529 .. 576 windows per colour
  few    30 x 30, 5 x 5 taps:  6 .. 7 per axis, 36 .. 49 windows
  zfill  42 x 42, 3 x 3 taps:  196 .. 225 windows; 514 channels = 3 blocks: 588 .. 675 workgroups,
         770 channels = 4 blocks: 784 .. 900
  b48    48 x 48, 3 x 3 taps:  256 .. 289 windows; two chains: 512 .. 578
  b72    72 x 72, 5 x 5 taps:  15, 15, 15, 16, 15 lattice points per axis by residue; two chains: colour
         (3, 3) has 512 workgroups -- the batch takes two layers -- and the last colour, (4, 4), 450: `few`
Depths: 15 (a padding channel), 16, 160 | 162 (the staged G rows move from two registers to four),
256 | 258 (256 streaming threads become 512), 512 | 514 (k_mh_ws gives way to the z-blocked form).

Provenance: the window counts above and every expected path were DERIVED from the code
(build_colour_lists, launch_mh_*); the rows' paths, `mh_strips_on` values and the agreement with
the oracle were then MEASURED on an MI355X (256 CUs) -- see the table in DESIGN.md section 3.

`mh_path` holds the LAST launch of a run, so two rows are shaped for their last launch: `batch_mixed_16`
(k_mh_ws<4, 2, 2, BATCH>: the few arm of a two-layer batch, geometry b72) and, of an EXPERIMENTS build,
`x_pair` (ONE sweep from a cleared state: colour 0 alone, then the pairs (1,2) .. (7,8); in a second
sweep the last colour would be launched alone).
"""
import functools

import numpy as np
import pytest

from deconv3d_amd import _lib, tiling
from oracle import deconv3d_oracle as O
from tests import prior_oracle
from tests.test_gpu_multiplet import multiplet
from tests.tiling_oracle import part_order

pytestmark = pytest.mark.gpu

SWEEPS = 2
SEED = 77
LAM = (4.0, 0.5, 2.0)                      # d3d_prior_begin, as tests/test_gpu_sweep_strips.py
DOUBLET = ((0., 3.8), (1., 1.4))           # tests/test_gpu_multiplet.py: SHAPES["doublet"]
GEOM = {"fill": (69, 69, 3), "few": (30, 30, 5), "zfill": (42, 42, 3), "b48": (48, 48, 3), "b72": (72, 72, 5)}


@functools.lru_cache(maxsize=None)
def compute_units():
    """CUs of the device the contexts run on (read-only option device_cus)."""
    with _lib.Engine((2, 3, 3), (1, 1)) as eng:
        n = eng.get_option("device_cus")
    assert n > 0
    return n


def windows_per_colour(H, W, f):
    """(fewest, most, last) windows of a colour launch: the lattice points y = cy + f i with
    -fhh <= y < H + fhh, times the same along x (build_colour_lists); last: of colour (f-1, f-1), the
    last launch of a sweep (run_part walks col = cy * fw + cx upwards)."""
    fhh = (f - 1) // 2

    def along(n):
        return [len([y for y in range(c - f, n + f, f) if -fhh <= y < n + fhh]) for c in range(f)]
    ys, xs = along(H), along(W)
    return min(ys) * min(xs), max(ys) * max(xs), ys[-1] * xs[-1]


def row(rid, geom, D, family, NS, U, M, K, fill, opts=None, uv=False, ntv=False, prior=False, multi=False,
        parts=None, chains=1, same_bits_as=(), experiments=False, sweeps=SWEEPS, layers=None):
    return dict(sweeps=sweeps, layers=layers, id=rid, geom=geom, D=D, family=family, NS=NS, U=U, M=M, K=K, fill=fill, opts=dict(opts or {}),
                uv=uv, ntv=ntv, prior=prior, multi=multi, parts=parts, chains=chains,
                same_bits_as=tuple(same_bits_as), experiments=experiments)


L1, L2, L3 = {"mh_layers": 1}, {"mh_layers": 2}, {"mh_layers": 3}
NOSMALL = {"mh_small": 0}
NT = {"mh_nt_ivar": 1}


def opts(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


ROWS = [
    # ---- k_mh_ws, 256 streaming threads ------------------------------------------------------------
    # one layer: <1,1,4> chip-filling; <4,1,4> few (and uniform variance, whose launches count as small)
    row("ws_fill_16_L1", "fill", 16, "ws", 256, 1, 1, 4, True, L1),
    row("ws_fill_16_L1_uv", "fill", 16, "ws", 256, 4, 1, 4, True, L1, uv=True),
    row("ws_few_128_L1", "few", 128, "ws", 256, 4, 1, 4, False, NOSMALL),
    row("ws_few_128_L1_uv", "few", 128, "ws", 256, 4, 1, 4, False, NOSMALL, uv=True),
    # two layers: <2,2,2> / <4,2,2> up to Dp = 160, <2,2,4> / <4,2,4> above
    row("ws_fill_16_L2", "fill", 16, "ws", 256, 2, 2, 2, True, same_bits_as=["ws_fill_16_L1"]),
    row("ws_fill_16_L2_uv", "fill", 16, "ws", 256, 4, 2, 2, True, uv=True),
    row("ws_fill_15_L2", "fill", 15, "ws", 256, 2, 2, 2, True),
    row("ws_fill_160_L2", "fill", 160, "ws", 256, 2, 2, 2, True),
    row("ws_fill_162_L2", "fill", 162, "ws", 256, 2, 2, 4, True),
    row("ws_fill_162_L2_uv", "fill", 162, "ws", 256, 4, 2, 4, True, uv=True),
    row("ws_fill_256_L2", "fill", 256, "ws", 256, 2, 2, 4, True),
    row("ws_few_128_L2", "few", 128, "ws", 256, 4, 2, 2, False, opts(L2, NOSMALL)),
    row("ws_few_160_L2", "few", 160, "ws", 256, 4, 2, 2, False, opts(L2, NOSMALL)),
    row("ws_few_162_L2", "few", 162, "ws", 256, 4, 2, 4, False, opts(L2, NOSMALL)),
    row("ws_few_256_L2", "few", 256, "ws", 256, 4, 2, 4, False, opts(L2, NOSMALL)),
    # three layers (Dp <= 160): <2,3,2> / <4,3,2>; beyond 160 channels the option falls back to two
    row("ws_fill_16_L3", "fill", 16, "ws", 256, 2, 3, 2, True, L3, same_bits_as=["ws_fill_16_L2"]),
    row("ws_fill_160_L3", "fill", 160, "ws", 256, 2, 3, 2, True, L3, same_bits_as=["ws_fill_160_L2"]),
    row("ws_fill_16_L3_uv", "fill", 16, "ws", 256, 4, 3, 2, True, L3, uv=True),
    row("ws_few_128_L3", "few", 128, "ws", 256, 4, 3, 2, False, opts(L3, NOSMALL), same_bits_as=["ws_few_128_L2"]),
    row("ws_fill_162_L3_is_L2", "fill", 162, "ws", 256, 2, 2, 4, True, L3, same_bits_as=["ws_fill_162_L2"]),
    # non-temporal 1/variance, write-through residual: chip-filling launches with per-voxel variance
    row("ws_fill_16_L1_nt", "fill", 16, "ws", 256, 1, 1, 4, True, opts(L1, NT), ntv=True,
        same_bits_as=["ws_fill_16_L1"]),
    row("ws_fill_16_L2_nt", "fill", 16, "ws", 256, 2, 2, 2, True, NT, ntv=True, same_bits_as=["ws_fill_16_L2"]),
    row("ws_fill_162_L2_nt", "fill", 162, "ws", 256, 2, 2, 4, True, NT, ntv=True,
        same_bits_as=["ws_fill_162_L2"]),
    row("ws_fill_16_L3_nt", "fill", 16, "ws", 256, 2, 3, 2, True, opts(L3, NT), ntv=True,
        same_bits_as=["ws_fill_16_L3"]),
    # ... and NOT the launches that do not fill the chip, nor the uniform-variance kernels
    row("ws_few_128_L2_nt_is_not_ntv", "few", 128, "ws", 256, 4, 2, 2, False, opts(L2, NOSMALL, NT),
        same_bits_as=["ws_few_128_L2"]),
    row("ws_fill_16_L2_uv_nt_is_not_ntv", "fill", 16, "ws", 256, 4, 2, 2, True, NT, uv=True),
    # ---- k_mh_ws, 512 streaming threads (258 .. 512 channels) ------------------------------------------
    row("ws512_few_258_L2", "few", 258, "ws", 512, 4, 2, 4, False, L2),
    row("ws512_fill_258_L2", "fill", 258, "ws", 512, 4, 2, 4, True),
    row("ws512_fill_258_L2_nt", "fill", 258, "ws", 512, 4, 2, 4, True, NT, ntv=True,
        same_bits_as=["ws512_fill_258_L2"]),
    row("ws512_fill_258_L2_uv", "fill", 258, "ws", 512, 4, 2, 4, True, uv=True),
    row("ws512_fill_512_L2", "fill", 512, "ws", 512, 4, 2, 4, True),
    row("ws512_fill_512_L2_nt", "fill", 512, "ws", 512, 4, 2, 4, True, NT, ntv=True,
        same_bits_as=["ws512_fill_512_L2"]),
    row("ws512_few_258_L1", "few", 258, "ws", 512, 4, 1, 4, False),
    row("ws512_few_512_L1", "few", 512, "ws", 512, 4, 1, 4, False),
    row("ws512_few_258_L1_uv", "few", 258, "ws", 512, 4, 1, 4, False, uv=True),
    row("ws512_fill_258_L1", "fill", 258, "ws", 512, 1, 1, 4, True, L1),
    row("ws512_fill_258_L1_nt", "fill", 258, "ws", 512, 1, 1, 4, True, opts(L1, NT), ntv=True,
        same_bits_as=["ws512_fill_258_L1"]),
    # (the 512-thread branch asks `few`, not `UV || few`: uniform variance keeps one position in flight)
    row("ws512_fill_258_L1_uv", "fill", 258, "ws", 512, 1, 1, 4, True, L1, uv=True),
    # ---- the wide forms: the small launches of a partitioned context at 128 channels -------------------
    row("small_wide_128", "few", 128, "small wide", 704, 6, 1, 1, False, parts="2x1"),
    row("small_wide_128_uv", "few", 128, "small wide", 704, 6, 1, 1, False, parts="2x1", uv=True),
    row("ws_wide_128", "few", 128, "ws", 704, 1, 1, 1, False, NOSMALL, parts="2x1"),
    row("ws_wide_128_uv", "few", 128, "ws", 704, 1, 1, 1, False, NOSMALL, parts="2x1", uv=True),
    # ---- k_mh_small: K = 1, 2, 4 registers per staged row ----------------------------------------------
    row("small_16", "few", 16, "small", 256, 8, 1, 1, False),
    row("small_16_uv", "few", 16, "small", 256, 8, 1, 1, False, uv=True),
    row("small_64", "few", 64, "small", 256, 8, 1, 1, False),
    row("small_66", "few", 66, "small", 256, 8, 1, 2, False),
    row("small_128", "few", 128, "small", 256, 8, 1, 2, False),
    row("small_128_uv", "few", 128, "small", 256, 8, 1, 2, False, uv=True),
    row("small_130", "few", 130, "small", 256, 8, 1, 4, False),
    row("small_256", "few", 256, "small", 256, 8, 1, 4, False),
    row("small_256_uv", "few", 256, "small", 256, 8, 1, 4, False, uv=True),
    # ---- the z-blocked form beyond 512 channels ---------------------------------------------------------
    row("zb_few_514_L2", "few", 514, "zb", 256, 4, 2, 4, False, L2),
    row("zb_few_514_L2_uv", "few", 514, "zb", 256, 4, 2, 4, False, L2, uv=True),
    row("zb_fill_514_L2", "zfill", 514, "zb", 256, 2, 2, 4, True),
    row("zb_fill_514_L2_nt", "zfill", 514, "zb", 256, 2, 2, 4, True, NT, ntv=True, same_bits_as=["zb_fill_514_L2"]),
    row("zb_fill_514_L2_uv", "zfill", 514, "zb", 256, 2, 2, 4, True, uv=True),
    row("zb_fill_770_L2", "zfill", 770, "zb", 256, 2, 2, 4, True),
    row("zb_few_514_L1", "few", 514, "zb", 256, 4, 1, 4, False),
    row("zb_few_514_L1_uv", "few", 514, "zb", 256, 4, 1, 4, False, uv=True),
    row("zb_fill_514_L1", "zfill", 514, "zb", 256, 4, 1, 4, True, L1),
    # ---- batched chains: one launch per colour for two contexts ------------------------------------------
    row("batch_fill_16", "b48", 16, "batch ws", 256, 2, 2, 2, True, chains=2),
    row("batch_fill_160", "b48", 160, "batch ws", 256, 2, 2, 2, True, chains=2),
    row("batch_fill_16_uv", "b48", 16, "batch ws", 256, 2, 2, 2, True, chains=2, uv=True),
    # (two layers because ONE colour of the batch fills the chip; the last colour's launch does not: the few arm)
    row("batch_mixed_16", "b72", 16, "batch ws", 256, 4, 2, 2, "mixed", chains=2),
    row("batch_few_128_ws", "few", 128, "batch ws", 256, 4, 1, 4, False, NOSMALL, chains=2),
    row("batch_few_128_ws_uv", "few", 128, "batch ws", 256, 4, 1, 4, False, NOSMALL, chains=2, uv=True),
    row("batch_small_16", "few", 16, "batch small", 256, 8, 1, 1, False, chains=2),
    row("batch_small_128", "few", 128, "batch small", 256, 8, 1, 2, False, chains=2),
    row("batch_small_256", "few", 256, "batch small", 256, 8, 1, 4, False, chains=2),
    row("batch_small_16_uv", "few", 16, "batch small", 256, 8, 1, 1, False, chains=2, uv=True),
    row("batch_small_128_uv", "few", 128, "batch small", 256, 8, 1, 2, False, chains=2, uv=True),
    row("batch_small_256_uv", "few", 256, "batch small", 256, 8, 1, 4, False, chains=2, uv=True),
    # ---- the plain deferred kernel (mh_defer = 2) at every workgroup size ---------------------------------
    row("defer_nt128", "few", 16, "defer", 128, 0, 1, 0, False, {"mh_defer": 2, "mh_nt": 128}),
    row("defer_nt256", "few", 16, "defer", 256, 0, 1, 0, False, {"mh_defer": 2, "mh_nt": 256}),
    row("defer_nt512", "few", 16, "defer", 512, 0, 1, 0, False, {"mh_defer": 2, "mh_nt": 512}),
    row("defer_nt1024", "few", 128, "defer", 1024, 0, 1, 0, False, {"mh_defer": 2, "mh_nt": 1024}),
    row("defer_514_without_zblocks", "few", 514, "defer", 1024, 0, 1, 0, False, {"mh_zblocks": 0}),
    # ---- immediate write-back, and cubes beyond 1024 channels without the z-blocks -----------------------
    row("immediate_16", "few", 16, "immediate", 256, 0, 0, 0, False, {"mh_defer": 0}),
    row("immediate_258", "few", 258, "immediate", 512, 0, 0, 0, False, {"mh_defer": 0}),
    row("immediate_514", "few", 514, "immediate", 1024, 0, 0, 0, False, {"mh_defer": 0}),
    row("immediate_nt128", "few", 16, "immediate", 128, 0, 0, 0, False, {"mh_defer": 0, "mh_nt": 128}),
    row("deep_1030", "few", 1030, "deep", 1024, 0, 0, 0, False, {"mh_zblocks": 0}),
    # ---- every family once more with the smoothness prior (refused on a context of several parts: the
    # wide forms on ONE part that is the whole cube, d3d_set_parts) ------------------------------------------
    row("prior_ws_fill", "fill", 16, "ws", 256, 2, 2, 2, True, prior=True),
    row("prior_ws512_fill", "fill", 258, "ws", 512, 4, 2, 4, True, prior=True),
    row("prior_small", "few", 128, "small", 256, 8, 1, 2, False, prior=True),
    row("prior_small_wide", "few", 128, "small wide", 704, 6, 1, 1, False, parts="one", prior=True),
    row("prior_ws_wide", "few", 128, "ws", 704, 1, 1, 1, False, NOSMALL, parts="one", prior=True),
    row("prior_zb_fill", "zfill", 514, "zb", 256, 2, 2, 4, True, prior=True),
    row("prior_batch_ws", "b48", 16, "batch ws", 256, 2, 2, 2, True, chains=2, prior=True),
    row("prior_batch_small", "few", 128, "batch small", 256, 8, 1, 2, False, chains=2, prior=True),
    row("prior_defer", "few", 16, "defer", 256, 0, 1, 0, False, {"mh_defer": 2}, prior=True),
    row("prior_immediate", "few", 16, "immediate", 256, 0, 0, 0, False, {"mh_defer": 0}, prior=True),
    row("prior_deep", "few", 1030, "deep", 1024, 0, 0, 0, False, {"mh_zblocks": 0}, prior=True),
    # ---- ... and once with a doublet ---------------------------------------------------------------------
    row("doublet_ws_fill", "fill", 16, "ws", 256, 2, 2, 2, True, multi=True),
    row("doublet_ws_fill_nt", "fill", 16, "ws", 256, 2, 2, 2, True, NT, ntv=True, multi=True,
        same_bits_as=["doublet_ws_fill"]),
    row("doublet_ws512_fill", "fill", 258, "ws", 512, 4, 2, 4, True, multi=True),
    row("doublet_small", "few", 128, "small", 256, 8, 1, 2, False, multi=True),
    row("doublet_small_wide", "few", 128, "small wide", 704, 6, 1, 1, False, parts="2x1", multi=True),
    row("doublet_ws_wide", "few", 128, "ws", 704, 1, 1, 1, False, NOSMALL, parts="2x1", multi=True),
    row("doublet_zb_fill", "zfill", 514, "zb", 256, 2, 2, 4, True, multi=True),
    row("doublet_batch_ws", "b48", 16, "batch ws", 256, 2, 2, 2, True, chains=2, multi=True),
    row("doublet_batch_small", "few", 128, "batch small", 256, 8, 1, 2, False, chains=2, multi=True),
    row("doublet_defer", "few", 16, "defer", 256, 0, 1, 0, False, {"mh_defer": 2}, multi=True),
    row("doublet_immediate", "few", 16, "immediate", 256, 0, 0, 0, False, {"mh_defer": 0}, multi=True),
    row("doublet_deep", "few", 1030, "deep", 1024, 0, 0, 0, False, {"mh_zblocks": 0}, multi=True),
    # ---- the families of a `make EXPERIMENTS=1` build ----------------------------------------------------
    row("x_small_full_L2", "fill", 16, "small full", 256, 2, 2, 4, True, {"mh_small": 2}, experiments=True),
    row("x_small_full_L1", "fill", 16, "small full", 256, 2, 1, 4, True, opts(L1, {"mh_small": 2}), experiments=True),
    row("x_small_full_L2_nt", "fill", 16, "small full", 256, 2, 2, 4, True, opts(NT, {"mh_small": 2}), ntv=True,
        experiments=True),
    # (one sweep from a cleared state: colour 0 alone, then four pair launches, each finding one layer)
    row("x_pair", "fill", 16, "pair", 256, 2, 2, 2, True, {"mh_pair": 1}, experiments=True, sweeps=1, layers=(0, 1)),
    row("x_pair_uv", "fill", 16, "pair", 256, 4, 2, 2, True, {"mh_pair": 1}, uv=True, experiments=True, sweeps=1,
        layers=(0, 1)),
    row("x_flow", "few", 16, "flow", 256, 0, 1, 0, False, {"mh_flow": 1}, experiments=True),
    row("x_chain", "few", 16, "chain", 5 * 8, 0, 1, 0, False, {"mh_chain": 1}, experiments=True),
]
ROW = {r["id"]: r for r in ROWS}
assert len(ROW) == len(ROWS)


def gaussian_taps(f, sigma=1.1):
    y = np.exp(-0.5 * ((np.arange(f) - (f - 1) / 2.0) / sigma) ** 2)
    x = np.exp(-0.5 * ((np.arange(f) - (f - 1) / 2.0) / (1.2 * sigma)) ** 2)
    t = np.outer(y, x)
    return t / t.sum()


@functools.lru_cache(maxsize=6)
def problem(geom, D, uv):
    """Inputs of a (geometry, depth, variance kind): noise around a faint line, two masked spaxels,
    a MUSE-like LSF (taps within +-8 channels: the z-blocked kernels take it)."""
    H, W, f = GEOM[geom]
    rng = np.random.default_rng([9100, H, W, f, D])
    truth = np.dstack((1.0 + 9.0 * rng.random((H, W)), D * (0.2 + 0.6 * rng.random((H, W))),
                       0.6 + 2.0 * rng.random((H, W))))
    mask = np.ones((H, W))
    mask[H // 3, W // 2] = mask[H - 1, 0] = 0
    data = rng.normal(0.0, 0.3, size=(D, H, W)) + truth[..., 0][None] * 0.05
    var = np.full((D, H, W), 0.09) if uv else 0.09 * (0.5 + rng.random((D, H, W)))
    init = truth * (0.8 + 0.4 * rng.random((H, W, 3)))
    p = dict(dims=(D, H, W), fsf=gaussian_taps(f), lsf=O.muse_like_lsf(D), data=data, var=var, mask=mask,
             init=init, mn=np.array([0.0, 0.0, 0.3]), mx=np.array([30.0, D - 1.0, 6.0]), ra=900.0,
             layout=tiling.TileLayout(H, W, f, f, 2, 1))
    for a in (data, var, mask, init):
        a.setflags(write=False)
    return p


def make_engine(r, p, seed):
    eng = _lib.Engine(p["dims"], p["fsf"].shape, options=r["opts"])
    try:
        eng.set_taps(p["fsf"], p["lsf"])
        if r["uv"]:
            eng.set_data(p["data"], None, var_scalar=0.09, mask=p["mask"])
        else:
            eng.set_data(p["data"], p["var"], mask=p["mask"])
        assert eng.variance_is_uniform() == r["uv"]
        if r["multi"]:
            eng.set_line_shape(*DOUBLET)
        if r["parts"] == "2x1":
            tiling.apply_parts(eng, p["layout"])
        elif r["parts"] == "one":       # one part, the whole cube: partitioned, and the prior is not refused
            eng.set_parts([(0, p["dims"][1], 0, p["dims"][2])], [0])
        eng.set_params(p["init"])
        eng.mh_config(p["mn"], p["mx"], 0.1, p["ra"], seed=seed, refresh_every=0)
        if r["prior"]:
            eng.prior_begin(LAM)
    except Exception:
        eng.close()
        raise
    return eng


KEPT = {}
REFERENCED = {other for r in ROWS for other in r["same_bits_as"]}


def device_run(rid):
    """device_run_once, kept for the rows that another row is compared with bit for bit."""
    if rid not in KEPT:
        out = device_run_once(rid)
        if rid not in REFERENCED:
            return out
        KEPT[rid] = out
    return KEPT[rid]


def device_run_once(rid):
    """The row on the device: per chain (err0, params, dlog, accepted, err), and what the context
    reports -- read before anything else is launched; `mh_path_launches` last, it clears the record."""
    r = ROW[rid]
    p = problem(r["geom"], r["D"], r["uv"])
    engs = [make_engine(r, p, SEED + k) for k in range(r["chains"])]
    try:
        assert [e.get_option("mh_path") for e in engs] == [0] * len(engs)       # d3d_mh_config cleared it
        err0 = [e.residual() for e in engs]
        if len(engs) > 1:
            acc = _lib.mh_sweeps_batch(engs, r["sweeps"], first_sweep=1)
        else:
            acc = [engs[0].mh_sweeps(r["sweeps"], 1)]
        lead = engs[0]
        report = dict(path=_lib.mh_path_fields(lead.get_option("mh_path")),
                      layers=_lib.mh_layers_seen(lead.get_option("mh_path_layers")),
                      launches=lead.get_option("mh_path_launches"),
                      strips=lead.get_option("mh_strips_on"),
                      batch_layers=lead.get_option("batch_layers"),
                      nt_on=lead.get_option("mh_nt_ivar_on"))
        assert lead.get_option("mh_path") == 0 and lead.get_option("mh_path_launches") == 0     # cleared by the read
        chains = []
        for e, a, e0 in zip(engs, acc, err0):
            out = (e0, e.get_params(), e.get_dlog(), np.int64(a), e.download_slot(_lib.SLOT_ERR))
            for x in out[:3] + out[4:]:
                x.setflags(write=False)
            chains.append(out)
        return chains, report
    finally:
        for e in engs:
            e.close()


ORACLE = {}


def oracle_run(r, p, seed, err0):
    """The oracle's sweeps of the row from the device's initial residual; shared by the rows of one problem,
    line shape, prior, scan order and seed (the caller has patched the oracle's line for a doublet)."""
    key = (r["geom"], r["D"], r["uv"], r["prior"], r["multi"], r["parts"], seed, r["sweeps"])
    hit = ORACLE.get(key)
    if hit is not None and np.array_equal(hit[0], err0):
        return hit[1]
    st = O.MHState(p["data"], p["var"], p["mask"], p["fsf"], p["lsf"], p["init"], p["mn"], p["mx"], 0.1, p["ra"],
                   seed, err=err0)
    f = p["fsf"].shape[0]
    for s in range(1, r["sweeps"] + 1):
        if r["parts"] == "2x1":     # the scan order of a partitioned context: phase by phase, part by part
            lay = p["layout"]
            order = [yx for ph in lay.phases for yx in part_order(lay.all_parts(), ph, st.mask, f, f)]
        else:
            order = list(O.colour_order(st.mask, f, f))
        if r["prior"]:
            prior_oracle.mh_sweep(st, s, LAM, order=order)
        else:
            O.mh_sweep(st, s, order=order)
    st.data = st.var = None     # (kept: the state after the sweeps alone)
    ORACLE[key] = (err0, st)
    return st


def expected_layers(r):
    if r["layers"] is not None:
        return r["layers"]
    if r["family"] in ("immediate", "deep"):
        return (0,)
    if r["family"] == "chain":      # (one launch for the whole call, the pending layers written back before it)
        return (0,)
    return tuple(range(r["M"] + 1))


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_dispatched_variant_matches_the_oracle_and_reports_its_path(rid, monkeypatch):
    r = ROW[rid]
    if r["experiments"] and not _lib.has_experiments():
        pytest.skip("a kernel family of a `make EXPERIMENTS=1` build")
    p = problem(r["geom"], r["D"], r["uv"])
    D, H, W = p["dims"]

    # the side of the chip-filling threshold the row was made for, from the device's CU count
    threshold = 2 * compute_units()
    blocks = ((D + 1) // 2 * 2 + 255) // 256 if r["family"] == "zb" else 1     # workgroups per window
    fewest, most, last = [n * blocks * r["chains"] for n in windows_per_colour(*GEOM[r["geom"]])]
    print("%s: %d CUs, threshold %d, %d .. %d workgroups per colour launch, %d in the last" % (
        rid, compute_units(), threshold, fewest, most, last))
    if r["fill"] == "mixed":
        assert last < threshold <= most, "geometry %s is not mixed on this chip: change the shape" % r["geom"]
    elif r["fill"]:
        assert fewest >= threshold, "geometry %s does not fill this chip: change the shape" % r["geom"]
    else:
        assert most < threshold, "geometry %s fills this chip: change the shape" % r["geom"]

    chains, report = device_run(rid)
    print(rid, report)

    # 1. the path
    want = dict(family=r["family"], NS=r["NS"], U=r["U"], M=r["M"], K=r["K"], NTV=r["ntv"], UV=r["uv"],
                prior=r["prior"], multi=r["multi"])
    assert report["path"] == want
    assert report["layers"] == expected_layers(r)
    assert report["launches"] > 0
    deferred_ws = r["family"] in ("ws", "zb") and r["chains"] == 1 and not r["parts"]
    assert report["strips"] == (2 if (r["fill"] is True and not r["uv"] and deferred_ws) else 0)
    assert report["nt_on"] == int(r["opts"].get("mh_nt_ivar", 0))
    if r["chains"] > 1:
        assert report["batch_layers"] == r["M"]

    # 2. the chain, update by update
    if r["multi"]:
        monkeypatch.setattr(O, "gaussian_line", multiplet(*DOUBLET))
    live = p["mask"] == 1
    for k, (err0, params, dlog, accepted, err) in enumerate(chains):
        st = oracle_run(r, p, SEED + k, err0)
        np.testing.assert_allclose(params[live], st.params[live], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(params[~live], p["init"][~live])
        np.testing.assert_allclose(dlog[live], st.dlog[live], rtol=1e-9, atol=1e-9 * np.abs(st.dlog[live]).max())
        assert accepted == st.accepted and 0 < accepted < r["sweeps"] * int(live.sum())
        assert np.max(np.abs(err - st.err)) <= 1e-11 * np.max(np.abs(st.err))

    # 3. bit for bit, where the project promises it
    for other in r["same_bits_as"]:
        ref, _ = device_run(other)
        for mine, theirs in zip(chains, ref):
            for a, b in zip(mine, theirs):
                np.testing.assert_array_equal(np.atleast_1d(a).view(np.uint64), np.atleast_1d(b).view(np.uint64))
