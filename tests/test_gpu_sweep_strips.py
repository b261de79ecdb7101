"""
Lattice-row strips of a colour row (option mh_strips): the strips of a colour
row run the colour's kernel on ranges of its work list, on streams of their own between one fork
and one join per colour row.  The same workgroup does the same arithmetic on the same window, so a
chain run in 2, 3 or 4 strips is the unsplit chain (mh_strips = 1) BIT FOR BIT -- parameters, log
ratios, accepted count and the carried residual, compared as 64-bit patterns -- and two equal runs
of the 3-strip chain are equal: a race between strips shows up as a difference there.

Each problem is the smallest that still has what can go wrong (see PROBLEMS).  Unless a problem
says otherwise mh_layers = 2 and mh_small = 0 are forced, so that the small cubes take the k_mh_ws
variants the strips apply to, and `mh_strips_on` is asserted -- and, after the sweeps, the kernel
variant that ran (read-only option `mh_path`, PATHS: a strip takes its colour's variant, so the path is
the unsplit chain's).  The unsplit reference of a problem is computed once and shared.

The chip-filling problems (69 x 69 and 42 x 42 with 3 x 3 taps) assume the 256 compute units of an
MI355X: 529 or more windows per colour, or 196 or more windows in three 256-channel blocks, against
a threshold of 2 workgroups per CU.  tests/test_gpu_mh_dispatch.py computes that threshold from the
device; here a path assertion fails where it does not hold.

What is sampled at the end of a sweep (posterior moments, histograms, regions, predictive accuracy,
jump-scale adaptation, Student-t weights, noise scales) runs on the context's stream after the last
colour row's join: FEATURES compares every accumulator of a 3-strip run with the unsplit run's.
"""
import functools

import numpy as np
import pytest

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O

pytestmark = pytest.mark.gpu

SWEEPS = 3
FORCE = {"mh_layers": 2, "mh_small": 0}


def gaussian_taps(fh, fw, sigma=1.1):
    y = np.exp(-0.5 * ((np.arange(fh) - (fh - 1) / 2.0) / sigma) ** 2)
    x = np.exp(-0.5 * ((np.arange(fw) - (fw - 1) / 2.0) / (1.2 * sigma)) ** 2)
    t = np.outer(y, x)
    return t / t.sum()


def masked_30x30(rng):
    """30 % masked at random; cube rows 0 .. 4 -- lattice row 0 of EVERY colour row of a 5 x 5 FSF --
    fully masked: with four strips strip 0 (the virtual row above the cube and lattice row 0) holds
    only virtual positions; colour (2, 3) fully masked: colour row 2 has an inactive colour."""
    mask = (rng.random((30, 30)) >= 0.3).astype(np.float64)
    mask[0:5, :] = 0
    mask[2::5, 3::5] = 0
    return mask


@functools.lru_cache(maxsize=None)
def problem(name):
    """dims, taps, data, variance (cube or scalar), mask, start, options, and what else is on."""
    base = {"options": dict(FORCE), "prior": None, "refresh_every": 0, "streamed": False, "var_scalar": None,
            "line": None}
    seed = {"c16": 1, "c16_default_small": 1, "odd": 2, "masked": 3, "masked_uniform": 3, "masked_nt": 3,
            "zb": 4, "prior": 5, "refresh": 5, "streamed": 5, "too_few_rows": 6, "c16_nt": 1, "c16_one_layer": 1,
            "c16_three_layers": 1, "doublet": 1, "c162_nt": 7, "c258": 8, "c258_nt": 8, "zb_full": 9,
            "zb_full_nt": 9}[name]
    rng = np.random.default_rng(9000 + seed)
    if name in ("c16", "c16_default_small", "c16_nt", "c16_one_layer", "c16_three_layers", "doublet", "c162_nt",
                "c258", "c258_nt"):
        # 23 x 23 = 529 windows per colour: fills the chip (>= 512 workgroups) without forcing
        D, H, W, fh, fw = 16, 69, 69, 3, 3
        if name == "c16_default_small":
            base["options"] = {"mh_layers": 2}
        if name == "c16_one_layer":
            base["options"] = {"mh_layers": 1, "mh_small": 0}
        if name == "c16_three_layers":
            base["options"] = {"mh_layers": 3, "mh_small": 0}
        if name == "doublet":
            base["line"] = ([0., 3.8], [1., 1.4])
        if name == "c162_nt":
            D = 162                             # the staged G rows in four registers
        if name.startswith("c258"):
            D = 258                             # 512 streaming threads
        if name.endswith("_nt"):
            base["options"]["mh_nt_ivar"] = 1  # non-temporal 1/variance, write-through stores: the launches fill the chip
    elif name in ("zb_full", "zb_full_nt"):
        # 14 .. 15 lattice points per axis: 196 .. 225 windows x 3 blocks of 256 channels fill the chip
        D, H, W, fh, fw = 514, 42, 42, 3, 3
        if name == "zb_full_nt":
            base["options"]["mh_nt_ivar"] = 1
    elif name == "odd":
        # odd depth (a padding channel), FSF not square, H and W no multiples of the period,
        # virtual rows outside the cube
        D, H, W, fh, fw = 15, 40, 45, 3, 7
    elif name.startswith("masked"):
        D, H, W, fh, fw = 128, 30, 30, 5, 5
        if name == "masked_uniform":
            base["var_scalar"] = 0.09
        if name == "masked_nt":
            # the option alone: at most 49 windows per colour do not fill the chip, and only the chip-filling
            # launches have the non-temporal / write-through variant -- this runs masked's kernel, <4, 2, 2>
            base["options"]["mh_nt_ivar"] = 1
    elif name == "zb":
        D, H, W, fh, fw = 640, 12, 12, 3, 3    # the z-blocked form + k_mh_zdecide
    elif name in ("prior", "refresh", "streamed"):
        D, H, W, fh, fw = 128, 30, 30, 5, 5
        if name == "prior":
            base["prior"] = [4.0, 0.5, 2.0]
        if name == "refresh":
            base["refresh_every"] = 2           # a from-scratch residual mid-run
        if name == "streamed":
            base["streamed"] = True
    elif name == "too_few_rows":
        D, H, W, fh, fw = 128, 12, 30, 5, 5    # lattice rows -1 .. 2: four strips would hold one each
    else:
        raise KeyError(name)
    fsf = gaussian_taps(fh, fw)
    lsf = O.muse_like_lsf(D)
    truth = np.dstack((1.0 + 9.0 * rng.random((H, W)), D * (0.2 + 0.6 * rng.random((H, W))),
                       0.6 + 2.0 * rng.random((H, W))))
    if name.startswith("masked"):
        mask = masked_30x30(rng)
    else:
        mask = np.ones((H, W))
        mask[H // 3, W // 2] = mask[H - 1, 0] = 0
    data = rng.normal(0.0, 0.3, size=(D, H, W)) + truth[..., 0][None] * 0.05
    var = 0.09 * (0.5 + rng.random((D, H, W)))
    init = truth * (0.8 + 0.4 * rng.random((H, W, 3)))
    base.update(dims=(D, H, W), fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, init=init,
                mn=np.array([0.0, 0.0, 0.3]), mx=np.array([30.0, D - 1.0, 6.0]))
    return base


def engine(p, strips, seed=77):
    eng = _lib.Engine(p["dims"], p["fsf"].shape, options=dict(p["options"], mh_strips=strips))
    eng.set_taps(p["fsf"], p["lsf"])
    if p["var_scalar"] is not None:
        eng.set_data(p["data"], None, var_scalar=p["var_scalar"], mask=p["mask"])
    else:
        eng.set_data(p["data"], p["var"], mask=p["mask"])
    if p["line"] is not None:
        eng.set_line_shape(*p["line"])
    eng.set_params(p["init"])
    eng.mh_config(p["mn"], p["mx"], 0.1, 900.0, seed=seed, refresh_every=p["refresh_every"])
    if p["prior"] is not None:
        eng.prior_begin(p["prior"])
    return eng


def path(family="ws", NS=256, U=4, M=2, K=2, **flags):
    out = dict(family=family, NS=NS, U=U, M=M, K=K, NTV=False, UV=False, prior=False, multi=False)
    out.update(flags)
    return out


# the kernel variant of every problem's last launch (_lib.mh_path_fields): two positions in flight where the
# launches fill the chip, four where they do not (and with uniform variance)
PATHS = {
    "c16": path(U=2), "c16_default_small": path(U=2), "odd": path(), "masked": path(), "masked_uniform": path(UV=True),
    "masked_nt": path(), "prior": path(prior=True), "refresh": path(), "streamed": path(), "too_few_rows": path(),
    "zb": path("zb", K=4),
    "c16_nt": path(U=2, NTV=True), "c16_one_layer": path(U=1, M=1, K=4), "c16_three_layers": path(U=2, M=3),
    "c162_nt": path(U=2, K=4, NTV=True), "c258": path(NS=512, K=4), "c258_nt": path(NS=512, K=4, NTV=True),
    "zb_full": path("zb", U=2, K=4), "zb_full_nt": path("zb", U=2, K=4, NTV=True), "doublet": path(U=2, multi=True),
}


def state(eng, acc, extra=()):
    return (eng.get_params(), eng.get_dlog(), np.array([acc], dtype=np.int64),
            eng.download_slot(_lib.SLOT_ERR)) + tuple(extra)


def chain(name, strips, expect_on=None):
    """SWEEPS sweeps from first_sweep = 1; the state afterwards (and the streamed arrays)."""
    p = problem(name)
    with engine(p, strips) as eng:
        if expect_on is None:
            expect_on = strips if strips > 1 else 0
        assert eng.get_option("mh_strips_on") == expect_on
        extra = ()
        if p["streamed"]:
            H, W = p["dims"][1:]
            ch, dl = np.zeros((SWEEPS + 1, H, W, 3)), np.zeros((SWEEPS + 1, H, W))
            acc = eng.mh_sweeps(SWEEPS, 1, keep_one_in=1, chain=ch, dlog=dl)
            extra = (ch, dl)
        else:
            acc = eng.mh_sweeps(SWEEPS, 1)
        assert _lib.mh_path_fields(eng.get_option("mh_path")) == PATHS[name]
        return state(eng, acc, extra)


@functools.lru_cache(maxsize=None)
def unsplit(name):
    out = chain(name, 1)
    for a in out:
        a.setflags(write=False)
    assert np.isfinite(out[0]).all() and out[2][0] > 0   # a chain that moves
    return out


def assert_same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint64 if g.itemsize == 8 else np.uint8),
                                      np.ascontiguousarray(w).view(np.uint64 if w.itemsize == 8 else np.uint8))


PROBLEMS = ["c16", "c16_default_small", "odd", "masked", "masked_uniform", "masked_nt", "prior", "refresh",
            "streamed", "c16_nt", "c16_one_layer", "c16_three_layers", "c162_nt", "c258", "c258_nt", "zb_full",
            "zb_full_nt", "doublet"]


@pytest.mark.parametrize("strips", [2, 3, 4])
@pytest.mark.parametrize("name", PROBLEMS)
def test_stripped_chain_is_the_unsplit_chain_bit_for_bit(name, strips):
    assert_same_bits(chain(name, strips), unsplit(name))


@pytest.mark.parametrize("name", PROBLEMS + ["zb"])
def test_two_equal_stripped_runs_are_equal(name):
    """Two runs in one process: a race between strips is a difference between equal runs."""
    strips = 2 if name == "zb" else 3     # (12 rows, 3 x 3 taps: lattice rows -1 .. 4 hold two strips of three)
    first = chain(name, strips)
    assert_same_bits(chain(name, strips), first)
    assert_same_bits(first, unsplit(name))


def test_z_blocked_form_in_two_strips():
    """640 channels: k_mh_ws<..., ZBK> on (window, block) workgroups + k_mh_zdecide, every strip its
    share of the blocks' wave sums."""
    p = problem("zb")
    with engine(p, 2) as eng:
        assert eng.get_option("mh_zblocks") == 1 and eng.get_option("lsf_fits") == 1
    assert_same_bits(chain("zb", 2), unsplit("zb"))


def labels_69():
    """Three regions of the 69 x 69 map that straddle the boundaries of three strips."""
    lab = np.zeros((69, 69), dtype=np.int32)
    lab[5:40, 3:30] = 1
    lab[20:66, 35:60] = 2
    lab[60:69, 0:20] = 3
    return lab


FEATURE_SWEEPS = 5

# what is sampled at the end of a sweep: how to arm it, and its accumulators as a tuple of arrays
FEATURES = {
    "post": (lambda e: (e.post_begin(), e.post_schedule(1, 1)),
             lambda e: sum((e.post_get(w) for w in (_lib.POST_PARAMETERS, _lib.POST_CLEAN_CUBE,
                                                    _lib.POST_CONVOLVED_CUBE)), ())),
    "hist": (lambda e: (e.post_begin(_lib.POST_CLEAN), e.hist_begin(pilot=2, span=4.0), e.post_schedule(1, 1)),
             lambda e: e.hist_get() + e.post_get(_lib.POST_PARAMETERS)),
    "region": (lambda e: (e.post_begin(_lib.POST_CLEAN), e.region_begin(labels_69(), capacity=FEATURE_SWEEPS),
                          e.post_schedule(1, 1)),
               lambda e: e.region_get()),
    "pred": (lambda e: (e.post_begin(_lib.POST_CLEAN), e.pred_begin(), e.post_schedule(1, 1)),
             lambda e: e.pred_get()),
    "adapt": (lambda e: e.adapt_begin(target=0.25, window=2, last_sweep=FEATURE_SWEEPS),
              lambda e: tuple(np.asarray(a) for a in e.adapt_get())),
    "robust": (lambda e: e.robust_begin(4, every=1, start=1, accumulate_from=2),
               lambda e: tuple(np.asarray(a) for a in e.robust_get())),
    "noise": (lambda e: e.noise_begin(np.arange(16) // 4, every=1, start=1, capacity=FEATURE_SWEEPS),
              lambda e: e.noise_get()),
}


def feature_run(feature, strips):
    arm, get = FEATURES[feature]
    with engine(problem("c16"), strips) as eng:
        assert eng.get_option("mh_strips_on") == (strips if strips > 1 else 0)
        arm(eng)
        acc = eng.mh_sweeps(FEATURE_SWEEPS, 1)
        assert _lib.mh_path_fields(eng.get_option("mh_path")) == PATHS["c16"]
        got = tuple(np.ascontiguousarray(a) for a in get(eng))
        if feature in ("post", "hist", "region", "pred"):
            assert eng.post_count() == FEATURE_SWEEPS
        return got, state(eng, acc)


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_features_sampled_at_the_end_of_a_sweep_see_the_joined_strips(feature):
    """On c16 in three strips against the unsplit chain: the downloaded accumulators and the chain
    state, bit for bit.  A feature that sampled before the last colour row's join would read a
    residual or parameters that a strip is still writing."""
    got, chain_state = feature_run(feature, 3)
    want, want_state = feature_run(feature, 1)
    assert len(got) == len(want) and len(got) >= 2
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8))
    assert_same_bits(chain_state, want_state)
    if feature == "adapt":
        assert int(got[3][0]) == FEATURE_SWEEPS // 2 and np.unique(got[0]).size > 1     # the scales moved
    if feature == "hist":
        assert got[0].sum() > 0                                                     # samples were binned


def test_unforced_strips_need_a_chip_filling_launch():
    """Automatic (mh_strips = 0): never on a latency-bound problem, whatever the build's default is."""
    with engine(problem("masked"), 0) as eng:
        assert eng.get_option("mh_strips_on") == 0


def test_too_few_lattice_rows_fall_back_to_whole_launches():
    """5 x 5 taps on 12 rows: lattice rows -1 .. 2.  Four strips would hold one row each: refused
    (mh_strips_on == 0), the chain is the unsplit one; two strips of two rows run."""
    assert_same_bits(chain("too_few_rows", 4, expect_on=0), unsplit("too_few_rows"))
    assert_same_bits(chain("too_few_rows", 2), unsplit("too_few_rows"))


def test_untouched_paths_read_the_strip_major_lists():
    """After a stripped run: one colour class through d3d_mh_colour (k_mh on the REAL spaxels of the
    list) and a d3d_mh_sweeps_batch of two contexts (the whole list in one launch) equal the
    unsplit contexts'."""
    p = problem("masked")
    outs = {}
    for strips in (1, 3):
        engs = [engine(p, strips, seed=77 + r) for r in range(2)]
        try:
            accs = [e.mh_sweeps(SWEEPS, 1) for e in engs]
            assert engs[0].get_option("mh_strips_on") == (strips if strips > 1 else 0)
            for col in (0, 7, 13, 24):      # (13 = colour (2, 3): fully masked, nothing to do)
                engs[0].mh_colour(col, SWEEPS + 1)
            after_colour = state(engs[0], accs[0])
            engs[0].mh_phase(0, SWEEPS + 1)     # stepping by phase: whole colour launches
            after_colour += state(engs[0], accs[0])
            accs = _lib.mh_sweeps_batch(engs, 2, first_sweep=SWEEPS + 2)
            outs[strips] = after_colour + state(engs[0], accs[0]) + state(engs[1], accs[1])
        finally:
            for e in engs:
                e.close()
    assert_same_bits(outs[3], outs[1])
