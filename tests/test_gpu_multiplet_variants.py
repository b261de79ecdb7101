"""
The multiplet line shape (d3d_set_line_shape, K > 1) on every kernel VARIANT, not only on the
default selection of each shape (tests/test_gpu_multiplet.py): each launcher picks between a
MULTI = false and a MULTI = true instantiation with `line.K > 1`, and the MULTI = true ones are
machine code of their own.  Here the tests that force a non-default single-Gaussian variant run
again with a shape set -- their bodies, shared through helpers that take `line_shape` -- and one
variant of every family is tied to the oracle with its line patched to the multiplet
(O.gaussian_line, as tests/test_gpu_multiplet.py does).  DESIGN.md section 5 ("multiplet
variants") lists the test that reaches each instantiation.

Tolerances are the project's: cubes 1e-12 of the peak, chain parameters
rtol = atol = 1e-9, carried residual 1e-11 of its peak, accepted counts equal, line cubes
1e-14 / 1e-13 of the peak; "bit for bit" is assert_array_equal.
"""
import ctypes as C

import numpy as np
import pytest

from deconv3d_amd import _lib, ensemble
from oracle import deconv3d_oracle as O
from tests.cases import make_case
from tests.test_gpu_edges import check_512_thread_schemes, check_z_blocked_against_plain
from tests.test_gpu_full_size_oracle import check_beyond_cache_policy
from tests.test_gpu_lines import DEPTHS, line_cubes, line_problem
from tests.test_gpu_multiplet import (QUAD, SHAPES, assert_cube_close, chain_against_oracle,
                                      depth_chain_against_oracle, multiplet)
from tests.test_gpu_parity import check_uniform_variance_variant, check_write_back_schemes, engine_for

pytestmark = pytest.mark.gpu

LINE_SHAPES = dict(SHAPES, quad=QUAD)


# ---- a. write-back schemes ------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["doublet", "quad"])
@pytest.mark.parametrize("name", ["c1", "odd_depth", "big_fsf", "tiny"])
def test_write_back_schemes_are_bit_identical_with_a_multiplet(name, shape, monkeypatch):
    """k_mh_ws<..., true> with one, two and three pending layers, with and without the sweep's
    proposal table, k_mh_defer<..., true> (mh_defer = 2), k_mh<..., true> as a sweep kernel
    (mh_defer = 0) and k_mh_small on a multiplet line table against k_mh_ws (mh_small = 0): the
    same bits.  The walk without zig-zag is another scan order: against its own mh_small = 0
    twin.  And the first variant against the patched oracle, three sweeps -- a bug shared by all
    MULTI = true kernels would pass the bit-identity legs."""
    ls = LINE_SHAPES[shape]
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    case = make_case(name)
    check_write_back_schemes(case, line_shape=ls, more_variants=[{"mh_small": 0}])
    check_write_back_schemes(case, line_shape=ls, variants=[{"mh_zigzag": 0}, {"mh_zigzag": 0, "mh_small": 0}])
    with engine_for(case, options={"mh_defer": 1}, line_shape=ls) as eng:
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             case["init"], case["min_b"], case["max_b"], 3, 777)


# ---- b. uniform variance ----------------------------------------------------------------------

@pytest.mark.parametrize("name,how,shape", [("c1", "scalar", "quad"), ("c1", "constant cube", "doublet"),
                                            ("odd_depth", "scalar", "doublet"),
                                            ("odd_depth", "constant cube", "quad"),
                                            ("big_fsf", "scalar", "quad"),
                                            ("big_fsf", "constant cube", "doublet")])
def test_uniform_variance_variant_is_bit_identical_with_a_multiplet(name, how, shape, monkeypatch):
    """The UV instantiations (1/var from a register) against the general ones (uniform_ivar = 0),
    bit for bit, and against the patched oracle."""
    ls = LINE_SHAPES[shape]
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    check_uniform_variance_variant(make_case(name), how, line_shape=ls)


# ---- c. depth classes (K = 3) -------------------------------------------------------------------

@pytest.mark.parametrize("D", [300, 512])
def test_512_thread_kernel_schemes_are_bit_identical_with_a_triplet(D):
    """257 .. 512 channels: k_mh_ws<512, ..., true> with one and two pending layers,
    k_mh_defer<512, true>, k_mh<512, 0, true>.  (The default of these depths meets the oracle in
    test_every_default_mh_kernel_depth_matches_the_multiplet_oracle.)"""
    check_512_thread_schemes(D, line_shape=SHAPES["triplet"])


@pytest.mark.parametrize("D,uniform", [(600, False), (1030, True)])
def test_z_blocked_sweep_kernels_against_the_plain_ones_with_a_triplet(D, uniform):
    """k_mh_ws<..., ZBK, true> with one and two pending layers bit for bit; against
    mh_zblocks = 0 (k_mh_defer<1024, true> at 600 channels, k_mh_deep<true> at 1030) to
    rounding."""
    check_z_blocked_against_plain(D, uniform, line_shape=SHAPES["triplet"])


@pytest.mark.parametrize("D", [600, 1000, 1025, 2048])
def test_plain_deep_kernels_match_the_triplet_oracle(D, monkeypatch):
    """A Gaussian LSF's long tail does not fit +-8 channels (lsf_fits == 0), so the default
    beyond 512 channels is k_mh_defer<1024, true> (600, 1000) and beyond 1024 k_mh_deep<true>
    with k_lines_deep<true> (1025, 2048): forward model and two sweeps against the oracle."""
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES["triplet"]))
    depth_chain_against_oracle(D, "gauss", SHAPES["triplet"], lsf_fits=0)


# ---- d. beyond-cache policy, launches that fill the chip ------------------------------------------

def test_beyond_cache_policy_is_bit_identical_and_matches_the_doublet_oracle(monkeypatch):
    """k_mh_ws<..., NTV, true> (mh_nt_ivar = 1) on the 16 x 300 x 300 problem: bit-identical to
    the default policy, `mh_nt_ivar_on` reports it, and one sweep against the oracle fed the
    device's initial residual."""
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES["doublet"]))
    check_beyond_cache_policy(line_shape=SHAPES["doublet"], sweeps=1)


# ---- e. the batched form that fills the chip --------------------------------------------------------

def batch_problem():
    """32 channels, 3 x 3 FSF, 60 x 60 spaxels: 400 windows per colour class -- alone a small
    launch (k_mh_small), four chains together 1600 workgroups: k_mh_ws<..., BATCH> with two
    pending layers (d3d_mh_sweeps_batch: Dp <= 160 and most * R >= half the flow grid)."""
    D, H, W = 32, 60, 60
    fsf = np.outer([0.25, 0.5, 0.25], [0.2, 0.5, 0.3])
    lsf = O.muse_like_lsf(D)
    rng = np.random.default_rng(411)
    truth = np.dstack((1.0 + 9.0 * rng.random((H, W)), D * (0.2 + 0.6 * rng.random((H, W))),
                       0.6 + 2.0 * rng.random((H, W))))
    mask = np.ones((H, W))
    mask[7, 11] = mask[40, 3] = 0
    data = rng.normal(0.0, 0.3, size=(D, H, W)) + truth[..., 0][None] * 0.05
    var = 0.09 * (0.5 + rng.random((D, H, W)))
    init = truth * (0.8 + 0.4 * rng.random((H, W, 3)))
    return (D, H, W), fsf, lsf, data, var, mask, init


def test_chip_filling_batched_form_is_the_chains_alone_with_a_doublet():
    R = 4
    ls = SHAPES["doublet"]
    dims, fsf, lsf, data, var, mask, init = batch_problem()
    assert fsf.shape == (3, 3)
    mn, mx = np.array([0.0, 0.0, 0.3]), np.array([30.0, dims[0] - 1.0, 6.0])

    def make(r, shape=ls):
        eng = _lib.Engine(dims, fsf.shape)
        eng.set_taps(fsf, lsf)
        eng.set_data(data * (1.0 + 0.1 * r), var * (1.0 + 0.05 * r), mask=mask)
        eng.set_line_shape(*shape)
        start = init.copy()
        start[..., 2] = np.clip(start[..., 2] + 0.05 * r, 0.3, 6.0)
        eng.set_params(start)
        eng.mh_config(mn, mx, 0.1, 900.0, seed=21 + r, refresh_every=0)
        return eng

    alone = []
    for r in range(R):
        with make(r) as eng:
            assert eng.mh_layers() == 1 and eng.get_option("small_parts") == 1   # alone: k_mh_small
            acc = eng.mh_sweeps(2, 1) + eng.mh_sweeps(2, 3)
            alone.append((eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(), acc))
    engs = [make(r) for r in range(R)]
    try:
        a1 = ensemble.sweep_chains_batched(engs, 2, 1)
        # (d3d_mh_layers reports a context's own depth -- 1 here; the depth of the joint launch
        #  is the read-only option batch_layers: 2 = k_mh_ws<..., BATCH>, not k_mh_small)
        assert [e.get_option("batch_layers") for e in engs] == [2] * R
        a2 = ensemble.sweep_chains_batched(engs, 2, 3)
        for r, eng in enumerate(engs):
            np.testing.assert_array_equal(eng.get_params(), alone[r][0])
            np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_ERR), alone[r][1])
            np.testing.assert_array_equal(eng.get_dlog(), alone[r][2])
            assert a1[r] + a2[r] == alone[r][3]
    finally:
        for e in engs:
            e.close()
    # contexts that differ in line shape share no launch
    engs = [make(0), make(1, SHAPES["triplet"])]
    try:
        with pytest.raises(ValueError, match="line shape"):
            ensemble.sweep_chains_batched(engs, 1, 1)
        rc = _lib.load().d3d_mh_sweeps_batch((C.c_void_p * 2)(*[e._ctx.value for e in engs]), 2, 1, 1, 1,
                                             None, None, (C.c_int64 * 2)())
        assert rc == _lib.ERR_INVALID
    finally:
        for e in engs:
            e.close()


def test_the_chain_alone_of_the_batched_problem_matches_the_doublet_oracle(monkeypatch):
    """Ties the batched test's reference (chain 0 alone) to the oracle: one sweep."""
    ls = SHAPES["doublet"]
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    dims, fsf, lsf, data, var, mask, init = batch_problem()
    mn, mx = np.array([0.0, 0.0, 0.3]), np.array([30.0, dims[0] - 1.0, 6.0])
    with _lib.Engine(dims, fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        eng.set_data(data, var, mask=mask)
        eng.set_line_shape(*ls)
        chain_against_oracle(eng, data, var, mask, fsf, lsf, init, mn, mx, 1, 21)


# ---- f. line cube kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["doublet", "quad"])
@pytest.mark.parametrize("D,lsf_kind", DEPTHS)
def test_line_cube_kernels_with_a_multiplet(D, lsf_kind, shape, monkeypatch):
    """k_lines<256 / 512 / 1024, true> (lines_dense = 0) and k_lines_dense<false, true>
    (everywhere: the test value 3; one, three and eight spaxel rounds per wavefront): clean and
    LSF-convolved cubes bit-identical, and within tests/test_gpu_lines.py's tolerances of the
    oracle (the w == 0 spaxel excluded: the reference divides 0 / 0 there)."""
    ls = LINE_SHAPES[shape]
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    H, W, lsf, params, mask = line_problem(D, lsf_kind)
    clean0, conv0 = line_cubes(D, H, W, lsf, params, mask, 0, line_shape=ls)
    for dense in (0, 1):
        for rounds in (0, 3, 8):
            clean_r, conv_r = line_cubes(D, H, W, lsf, params, mask, dense, rounds, line_shape=ls)
            np.testing.assert_array_equal(clean_r, clean0)
            np.testing.assert_array_equal(conv_r, conv0)
    single, _ = line_cubes(D, H, W, lsf, params, mask, 0)
    assert not np.array_equal(single, clean0)
    assert np.isfinite(clean0).all() and np.isfinite(conv0).all()
    assert (clean0[:, mask == 0] == 0).all() and (conv0[:, mask == 0] == 0).all()
    scale = np.max(np.abs(clean0))
    want_clean = O.simulate_clean((D, H, W), params, mask)
    want = O.lsf_lines((D, H, W), params, mask, lsf) if lsf is not None else want_clean
    ok = np.ones((H, W), dtype=bool)
    ok[1, 0] = False
    assert np.max(np.abs(clean0 - want_clean)[:, ok]) <= 1e-14 * scale
    assert np.max(np.abs(conv0 - want)[:, ok]) <= 1e-13 * scale


# ---- g. edges of the shape -------------------------------------------------------------------------------

def test_zero_width_multiplet_is_deltas_not_nan():
    """unit_line's delta rule per component: w == 0, c = 10, offsets 0, 3, -4, 2.5 with ratios
    1, 0.5, 2, 1 and amplitude 3 is exactly 3, 1.5, 6 at channels 10, 13, 6 (the half-integer
    component meets no channel).  Expected vector by hand: numpy gives 0 / 0 here."""
    D, H, W = 16, 4, 4
    fsf = np.ones((1, 1))
    params = np.zeros((H, W, 3))
    params[..., 2] = 1.0
    params[1, 2] = [3.0, 10.0, 0.0]
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, None)
        eng.set_data(np.ones((D, H, W)), None, 1.0)
        eng.set_line_shape([0., 3., -4., 2.5], [1., 0.5, 2., 1.])
        eng.set_params(params)
        clean = eng.build_clean()
    assert np.isfinite(clean).all()
    want = np.zeros(D)
    want[10], want[13], want[6] = 3.0, 1.5, 6.0
    np.testing.assert_array_equal(clean[:, 1, 2], want)


@pytest.mark.parametrize("side", ["above", "below"])
def test_secondary_components_wholly_outside_the_cube(side, monkeypatch):
    """Every spaxel's centre on the bound of c (D - 1 with offsets +40 and +55.5; 0 with -40 and
    -55.5 on 32 channels): the secondary components contribute rounding-level tails or exact
    zeros, nothing NaN; forward model and one sweep equal the oracle."""
    sign = 1. if side == "above" else -1.
    ls = ([0., sign * 40., sign * 55.5], [1., 0.7, 2.0])
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    case = make_case("c1")
    dims = (case["D"], case["H"], case["W"])
    start = case["init"].copy()
    start[..., 1] = case["max_b"][1] if side == "above" else case["min_b"][1]
    with engine_for(case, line_shape=ls) as eng:
        eng.set_params(start)
        sim = eng.forward()
        assert np.isfinite(sim).all()
        assert_cube_close(sim, O.forward_full(dims, start, case["mask"], case["fsf"], case["lsf"]), "forward")
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             start, case["min_b"], case["max_b"], 1, 777)
        assert np.isfinite(eng.get_params()).all() and np.isfinite(eng.download_slot(_lib.SLOT_ERR)).all()


def test_component_centred_on_the_padded_channel_of_an_odd_depth(monkeypatch):
    """D = 21 is stored with a zero 22nd channel.  A component centred exactly there (c = 17,
    offset 4: c + offset = 21.0) must leave it zero: the (D, H, W) downloads of the model and of
    the residual equal the oracle, and the chi2 map equals the oracle's half_chi2 per spaxel --
    a leak into the pad channel would be summed there."""
    ls = ([0., 4.0], [1., 1.4])
    monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
    case = make_case("odd_depth")
    D, H, W = dims = (case["D"], case["H"], case["W"])
    assert D == 21
    params = case["init"].copy()
    params[..., 1] = 17.0
    params[..., 2] = np.minimum(params[..., 2], 2.0)
    with engine_for(case, line_shape=ls) as eng:
        eng.set_params(params)
        eng.forward(fetch=False)
        sim = eng.download_slot(_lib.SLOT_SIM)
        want = O.forward_full(dims, params, case["mask"], case["fsf"], case["lsf"])
        assert_cube_close(sim, want, "SLOT_SIM")
        err = eng.residual()
        want_err = O.compute_error_in_one_step(case["data"], params, case["mask"], case["fsf"], case["lsf"])
        assert_cube_close(err, want_err, "residual")
        assert_cube_close(eng.download_slot(_lib.SLOT_ERR), want_err, "SLOT_ERR")
        cmap, total = eng.chi2_map()
        ref = np.array([[O.half_chi2(want_err[:, y, x], case["var"][:, y, x]) for x in range(W)]
                        for y in range(H)])
        np.testing.assert_allclose(cmap, ref, rtol=1e-10, atol=1e-12 * ref.sum())
        np.testing.assert_allclose(total, ref.sum(), rtol=1e-10)


# ---- h. changing the shape in the middle of a chain ---------------------------------------------------------

def test_changing_the_line_shape_mid_chain_equals_a_fresh_context(monkeypatch):
    """Default options on `moffat` (a pending layer in play at every switch): two sweeps with the
    doublet, the triplet, then the single Gaussian.  d3d_set_line_shape writes the pending layer
    back with the OLD line and invalidates the residual and the sweep's tables, so each segment
    is, bit for bit, a fresh context given the previous segment's final parameters, the new
    shape and the same sweep numbers; and every segment's carried residual is the patched
    oracle's data - forward model of its parameters."""
    case = make_case("moffat")
    dims = (case["D"], case["H"], case["W"])
    segments = [SHAPES["doublet"], SHAPES["triplet"], ([0.], [1.])]

    def configure(eng, params):
        eng.set_params(params)
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)

    ends = []
    with engine_for(case) as eng:
        for k, ls in enumerate(segments):
            eng.set_line_shape(*ls)
            if k == 0:
                configure(eng, case["init"])
            acc = eng.mh_sweeps(2, 2 * k + 1)
            ends.append((eng.get_params(), eng.get_dlog(), acc))      # (no download: nothing flushed)
        last_err = eng.download_slot(_lib.SLOT_ERR)
    start = case["init"]
    for k, ls in enumerate(segments):
        with engine_for(case, line_shape=ls) as fresh:
            configure(fresh, start)
            acc = fresh.mh_sweeps(2, 2 * k + 1)
            np.testing.assert_array_equal(ends[k][0], fresh.get_params(), err_msg="segment %d" % k)
            np.testing.assert_array_equal(ends[k][1], fresh.get_dlog(), err_msg="segment %d" % k)
            assert ends[k][2] == acc
            err = fresh.download_slot(_lib.SLOT_ERR)
        assert acc > 0
        monkeypatch.setattr(O, "gaussian_line", multiplet(*ls))
        want = case["data"] - O.forward_full(dims, ends[k][0], case["mask"], case["fsf"], case["lsf"])
        assert np.max(np.abs(err - want)) <= 1e-11 * np.max(np.abs(want)), "segment %d" % k
        start = ends[k][0]
    np.testing.assert_array_equal(last_err, err)


# ---- i. the library's own refusals ------------------------------------------------------------------------------

def dbl(values):
    return (C.c_double * len(values))(*values)


BAD_SHAPES = [
    ("K = 0", 0, [0.], [1.]),
    ("K = 5", 5, [0., 1., 2., 3., 4.], [1., 1., 1., 1., 1.]),
    ("NaN offset", 2, [0., float("nan")], [1., 1.]),
    ("inf offset", 2, [0., float("inf")], [1., 1.]),
    ("NaN ratio", 2, [0., 2.], [1., float("nan")]),
    ("inf ratio", 3, [0., 2., 3.], [1., 1., float("inf")]),
    ("offsets[0] != 0", 2, [0.5, 2.], [1., 1.]),
    ("ratios[0] != 1", 2, [0., 2.], [0.9, 1.]),
    ("negative ratio", 3, [0., 2., 5.], [1., 1., -0.1]),
    ("duplicate offsets", 3, [0., 2., 2.], [1., 1., 1.]),
    ("duplicate of the first", 2, [0., 0.], [1., 1.]),
    ("NULL offsets", 2, None, [1., 1.]),
    ("NULL ratios", 2, [0., 2.], None),
]


def test_d3d_set_line_shape_refuses_invalid_shapes_and_keeps_the_old_one():
    """The library's own validation (Engine.set_line_shape and the Python model check first, so
    these branches are otherwise never reached): D3D_ERR_INVALID with a message, returned before
    anything is launched, and the context keeps the shape it had -- its cube is the same bits."""
    lib = _lib.load()
    case = make_case("c1")
    with engine_for(case, line_shape=SHAPES["triplet"]) as eng:
        before = eng.simulate(case["truth"], convolved=True)
        for what, K, off, rat in BAD_SHAPES:
            rc = lib.d3d_set_line_shape(eng._ctx, K, None if off is None else dbl(off),
                                        None if rat is None else dbl(rat))
            assert rc == _lib.ERR_INVALID, what
            assert lib.d3d_last_error(), what
            np.testing.assert_array_equal(eng.simulate(case["truth"], convolved=True), before, err_msg=what)
        assert lib.d3d_set_line_shape(None, 1, dbl([0.]), dbl([1.])) == _lib.ERR_INVALID
        # and a valid call still works
        assert lib.d3d_set_line_shape(eng._ctx, 2, dbl(SHAPES["doublet"][0]), dbl(SHAPES["doublet"][1])) == 0
        assert not np.array_equal(eng.simulate(case["truth"], convolved=True), before)


def unsupported(call):
    """The call is refused with D3D_ERR_UNSUPPORTED, which the binding raises as
    NotImplementedError (deconv3d_amd._lib._check; HipError is for HIP runtime failures)."""
    with pytest.raises(NotImplementedError, match="multiplet form") as info:
        call()
    assert not isinstance(info.value, _lib.HipError)


def test_options_without_a_multiplet_form_are_refused_not_ignored():
    """lines_dense = 2 (the line cube with its own exp) and, in an EXPERIMENTS build, mh_maxit,
    mh_flow, mh_pair and mh_chain have no MULTI = true kernel: with K > 1 they answer
    D3D_ERR_UNSUPPORTED -- a status code before any launch --, with K = 1 they work."""
    lib = _lib.load()
    case = make_case("c1")
    case["lsf"] = O.muse_like_lsf(case["D"])        # taps within +-8 channels: the dense line kernel applies
    with engine_for(case, options={"lines_dense": 2}) as eng:
        eng.set_params(case["truth"])
        single = eng.forward()                                        # K = 1: works
        assert np.isfinite(single).all()
        eng.set_line_shape(*SHAPES["doublet"])
        assert lib.d3d_forward(eng._ctx, None) == _lib.ERR_UNSUPPORTED
        assert b"lines_dense" in lib.d3d_last_error()
        unsupported(eng.forward)
        unsupported(eng.build_clean)
        unsupported(lambda: eng.simulate(case["truth"], convolved=False))
        eng.set_option("lines_dense", 1)                              # the option, not the context, is refused
        assert not np.array_equal(eng.forward(), single)
        eng.set_option("lines_dense", 2)
        eng.set_line_shape([0.], [1.])
        np.testing.assert_array_equal(eng.forward(), single)
    if _lib.has_experiments():
        for opts in ({"mh_defer": 0, "mh_maxit": 8}, {"mh_defer": 1, "mh_flow": 1},
                     {"mh_defer": 1, "mh_layers": 2, "mh_pair": 1}, {"mh_chain": 1}):
            with engine_for(case, options=opts) as eng:
                if "mh_chain" in opts:
                    assert eng.get_option("chain_parts") == 1
                eng.set_params(case["init"])
                eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)
                assert eng.mh_sweeps(1, 1) > 0                        # K = 1: works
                eng.set_line_shape(*SHAPES["doublet"])
                unsupported(lambda: eng.mh_sweeps(1, 2))
                assert np.isfinite(eng.get_params()).all()
