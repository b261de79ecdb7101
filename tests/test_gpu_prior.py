"""
GPU tests of the smoothness prior between neighbouring spaxels (d3d_prior_*, Run(smoothness=...)).

The device chain runs against tests/prior_oracle.py -- the oracle's update with the prior's two
terms -- sweep by sweep, on every kernel variant of the default build, with the tolerances
tests/test_gpu_chain.py applies to the same quantities without a prior: parameters
rtol = atol = 1e-9, dlog 1e-9 relative (and of its largest value), the carried residual 1e-11 of
its peak, accepted counts equal.  "Bit for bit" is assert_array_equal.
"""
import ctypes as C

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, ensemble
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import prior_oracle as PO
from tests.cases import make_case
from tests.test_gpu_multiplet import SHAPES, multiplet, run_inputs
from tests.test_gpu_multiplet_variants import batch_problem

pytestmark = pytest.mark.gpu

LAM = np.array([0.8, 1.5, 2.5])
SEED, RA, SWEEPS = 77, 35.0, 3

# the kernels of the default build that decide an update, as tests/test_gpu_parity.py's
# check_write_back_schemes and tests/test_gpu_multiplet_variants.py select them: k_mh_small (the
# default of these small cubes), k_mh_ws forced on them with one, two and three pending layers, with
# and without the sweep's proposal table, the walk without zig-zag, k_mh_defer, k_mh
VARIANTS = [{}, {"mh_props": 0}, {"mh_small": 0}, {"mh_small": 0, "mh_props": 0},
            {"mh_small": 0, "mh_layers": 1}, {"mh_small": 0, "mh_layers": 2}, {"mh_small": 0, "mh_layers": 3},
            {"mh_zigzag": 0}, {"mh_zigzag": 0, "mh_small": 0}, {"mh_defer": 2}, {"mh_defer": 0}]


def custom_case(D, H, W, fsf, lsf, mask, seed):
    """tests/cases.py's recipe for a shape, FSF and mask of the caller's."""
    rng = np.random.default_rng(seed)
    truth = np.dstack((1.0 + 9.0 * rng.random((H, W)), D * (0.25 + 0.5 * rng.random((H, W))),
                       0.8 + 2.0 * rng.random((H, W))))
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    sigma = 0.05 * np.max(clean) + 1e-3
    data = clean + rng.normal(0., sigma, size=(D, H, W))
    var = (sigma * (0.5 + rng.random((D, H, W)))) ** 2
    min_b = O.model_min_boundaries()
    max_b = O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, truth=truth, mask=mask, data=data, var=var,
                min_b=min_b, max_b=max_b, init=init)


def problem(name):
    """(case, lam, uniform variance or None, line shape or None)"""
    if name == "c1":                     # 32 x 16 x 16, the 9 x 9 FSF, all three weights
        return make_case("c1"), LAM, None, None
    if name == "odd_asym_masked":        # odd depth, asymmetric 5 x 3 FSF, a masked block, an isolated spaxel
        D, H, W = 21, 12, 10
        rng = np.random.default_rng(5)
        fsf = rng.random((5, 3))
        fsf /= fsf.sum()
        mask = np.ones((H, W))
        mask[2:5, 6:9] = 0               # a block
        for y, x in ((8, 3), (10, 3), (9, 2), (9, 4)):   # (9, 3): its four neighbours all masked
            mask[y, x] = 0
        assert PO.neighbours(mask, 9, 3) == [] and mask[9, 3] == 1
        return custom_case(D, H, W, fsf, O.gaussian_lsf_vector(D, 1.3), mask, 91), LAM, None, None
    if name == "fsf3":                   # the tightest colouring: every neighbour is of the adjacent class
        D, H, W = 32, 8, 8
        fsf = np.outer([0.25, 0.5, 0.25], [0.2, 0.5, 0.3])
        return custom_case(D, H, W, fsf, O.gaussian_lsf_vector(D, 0.9088), np.ones((H, W)), 92), LAM, None, None
    if name == "uniform":                # one constant variance: the UV instantiations
        case = make_case("c1")
        return case, np.array([0.5, 0., 4.]), float(np.median(case["var"])), None
    if name == "doublet":
        D, H, W = 32, 8, 8
        fsf = np.outer([0.25, 0.5, 0.25], [0.2, 0.5, 0.3])
        return custom_case(D, H, W, fsf, O.gaussian_lsf_vector(D, 0.9088), np.ones((H, W)), 93), LAM, None, SHAPES["doublet"]
    raise KeyError(name)


def engine_of(case, options=None, uniform=None, line=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    if uniform is not None:
        eng.set_data(case["data"], None, var_scalar=uniform, mask=case["mask"])
    else:
        eng.set_data(case["data"], case["var"], mask=case["mask"])
    if line is not None:
        eng.set_line_shape(*line)
    return eng


def oracle_sweeps(case, lam, uniform):
    """The state after each of SWEEPS sweeps: computed once per problem, shared by the variants."""
    var = case["var"] if uniform is None else np.full(case["data"].shape, uniform)
    st = O.MHState(case["data"], var, case["mask"], case["fsf"], case["lsf"], case["init"],
                   case["min_b"], case["max_b"], 0.1, RA, SEED)
    out = []
    for s in range(1, SWEEPS + 1):
        PO.mh_sweep(st, s, lam)
        out.append((st.params.copy(), st.err.copy(), st.dlog.copy(), st.accepted))
    return out


@pytest.mark.parametrize("name", ["c1", "odd_asym_masked", "fsf3", "uniform", "doublet"])
def test_chain_with_the_prior_matches_the_oracle_on_every_kernel_variant(name, monkeypatch):
    case, lam, uniform, line = problem(name)
    if line is not None:
        monkeypatch.setattr(O, "gaussian_line", multiplet(*line))
    want = oracle_sweeps(case, lam, uniform)
    live = case["mask"] == 1
    variants = list(VARIANTS)
    if uniform is not None:
        variants.append({"uniform_ivar": 0})
    first = None
    for opts in variants:
        with engine_of(case, opts, uniform, line) as eng:
            if uniform is not None:
                assert eng.variance_is_uniform() == (opts.get("uniform_ivar", 1) == 1)
            eng.set_params(case["init"])
            eng.mh_config(case["min_b"], case["max_b"], 0.1, RA, seed=SEED, refresh_every=0)
            eng.prior_begin(lam)
            acc = 0
            for s in range(1, SWEEPS + 1):
                acc += eng.mh_sweeps(1, s)
                params, dlog, err = eng.get_params(), eng.get_dlog(), eng.download_slot(_lib.SLOT_ERR)
                w_params, w_err, w_dlog, w_acc = want[s - 1]
                what = "%s %s sweep %d" % (name, opts, s)
                np.testing.assert_allclose(params[live], w_params[live], rtol=1e-9, atol=1e-9, err_msg=what)
                np.testing.assert_allclose(dlog[live], w_dlog[live], rtol=1e-9,
                                           atol=1e-9 * max(np.abs(w_dlog[live]).max(), 1e-300), err_msg=what)
                assert np.max(np.abs(err - w_err)) <= 1e-11 * np.max(np.abs(w_err)), what
                assert acc == w_acc, what
            if first is None:
                first = (params, acc)
            elif "mh_zigzag" not in opts:
                # the write-back schemes and kernel families are one arithmetic (tests/test_gpu_parity.py:
                # check_write_back_schemes), with the prior's terms too: the same bits
                np.testing.assert_array_equal(params, first[0], err_msg="%s %s" % (name, opts))
    # and the prior does something here: another chain than without it
    with engine_of(case, None, uniform, line) as eng:
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, RA, seed=SEED, refresh_every=0)
        eng.mh_sweeps(SWEEPS, 1)
        assert not np.array_equal(eng.get_params(), first[0])


def check_variants(name, case, lam, uniform, line, variants, sweeps=SWEEPS):
    """Every option set of `variants` against the oracle with the prior, sweep by sweep."""
    var = case["var"] if uniform is None else np.full(case["data"].shape, uniform)
    st = O.MHState(case["data"], var, case["mask"], case["fsf"], case["lsf"], case["init"],
                   case["min_b"], case["max_b"], 0.1, RA, SEED)
    want = []
    for s in range(1, sweeps + 1):
        PO.mh_sweep(st, s, lam)
        want.append((st.params.copy(), st.err.copy(), st.dlog.copy(), st.accepted))
    live = case["mask"] == 1
    for opts, expect in variants:
        with engine_of(case, opts, uniform, line) as eng:
            for key, value in expect.items():
                assert eng.get_option(key) == value, (name, opts, key)
            eng.set_params(case["init"])
            eng.mh_config(case["min_b"], case["max_b"], 0.1, RA, seed=SEED, refresh_every=0)
            eng.prior_begin(lam)
            acc = 0
            for s in range(1, sweeps + 1):
                acc += eng.mh_sweeps(1, s)
                params, dlog, err = eng.get_params(), eng.get_dlog(), eng.download_slot(_lib.SLOT_ERR)
                w_params, w_err, w_dlog, w_acc = want[s - 1]
                what = "%s %s sweep %d" % (name, opts, s)
                np.testing.assert_allclose(params[live], w_params[live], rtol=1e-9, atol=1e-9, err_msg=what)
                np.testing.assert_allclose(dlog[live], w_dlog[live], rtol=1e-9,
                                           atol=1e-9 * max(np.abs(w_dlog[live]).max(), 1e-300), err_msg=what)
                assert np.max(np.abs(err - w_err)) <= 1e-11 * np.max(np.abs(w_err)), what
                assert acc == w_acc, what


# the depth classes of tests/test_gpu_multiplet_variants.py: each selects another deciding kernel
DEPTHS = [
    (300, "gauss", False, [({}, {}), ({"mh_layers": 1}, {}), ({"mh_defer": 2}, {}), ({"mh_defer": 0}, {})]),
    (512, "gauss", True, [({}, {}), ({"uniform_ivar": 0}, {})]),        # k_mh_ws<512>, k_mh_defer<512>, k_mh<512>
    (600, "muse", False, [({}, {"lsf_fits": 1}), ({"mh_layers": 1}, {}),    # k_mh_ws<ZBK> + k_mh_zdecide
                          ({"mh_zblocks": 0}, {}), ({"mh_defer": 0}, {})]),  # k_mh_defer<1024>, k_mh<1024>
    (600, "gauss", True, [({}, {"lsf_fits": 0})]),                          # (the taps do not fit: k_mh_defer<1024>)
    (1030, "muse", True, [({}, {"lsf_fits": 1}), ({"mh_zblocks": 0}, {})]),  # z-blocked; k_mh_deep
    (1030, "gauss", False, [({}, {"lsf_fits": 0})]),                         # k_mh_deep
]


@pytest.mark.parametrize("D,lsf_kind,uniform,variants", DEPTHS,
                         ids=["%d-%s" % (d[0], d[1]) for d in DEPTHS])
def test_chain_with_the_prior_matches_the_oracle_in_every_depth_class(D, lsf_kind, uniform, variants):
    """The 5 x 6 problem of tests/test_gpu_multiplet.py's depth_chain_against_oracle (one spaxel
    masked) at the depths that select the 512-thread k_mh_ws, the z-blocked pair, k_mh_defer<1024>
    and k_mh_deep, with per-voxel and with uniform variance: two sweeps against the oracle."""
    H, W = 5, 6
    fsf = O.gaussian_fsf_image(1.6)
    lsf = O.gaussian_lsf_vector(D, 1.1) if lsf_kind == "gauss" else O.muse_like_lsf(D)
    mask = np.ones((H, W))
    mask[2, 3] = 0
    case = custom_case(D, H, W, fsf, lsf, mask, 1000 + D)
    case["init"][..., 2] = np.maximum(case["init"][..., 2], 0.5)
    check_variants("D=%d %s" % (D, lsf_kind), case, LAM, float(np.median(case["var"])) if uniform else None,
                   None, variants, sweeps=2)


# ---- off is off ------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [{}, {"mh_small": 0}, {"mh_defer": 0}])
def test_zero_weights_and_ending_the_prior_give_the_chain_without_it_bit_for_bit(opts):
    case = make_case("c1")

    def chain(prepare, mid=None):
        with engine_of(case, opts) as eng:
            eng.set_params(case["init"])
            eng.mh_config(case["min_b"], case["max_b"], 0.1, RA, seed=11, refresh_every=0)
            prepare(eng)
            acc = eng.mh_sweeps(2, 1)
            if mid is not None:
                mid(eng)
            acc += eng.mh_sweeps(2, 3)
            return acc, eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog()

    def same(a, b):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            np.testing.assert_array_equal(x, y)

    def begin_end(eng):
        eng.prior_begin(LAM)
        assert eng.prior_get()[1] and np.array_equal(eng.prior_get()[0], LAM)
        eng.prior_end()
        lam, on = eng.prior_get()
        assert not on and not lam.any()

    plain = chain(lambda eng: None)
    same(chain(lambda eng: eng.prior_begin(np.zeros(3))), plain)
    same(chain(begin_end), plain)
    # d3d_prior_end in the middle of a run restores it: the second half is what zero weights give
    with_prior = chain(lambda eng: eng.prior_begin(LAM), mid=lambda eng: eng.prior_end())
    same(chain(lambda eng: eng.prior_begin(LAM), mid=lambda eng: eng.prior_begin(np.zeros(3))), with_prior)
    kept = chain(lambda eng: eng.prior_begin(LAM))
    assert not np.array_equal(with_prior[1], plain[1]) and not np.array_equal(with_prior[1], kept[1])


def run_kw(var, **more):
    kw = dict(variance=var, seed=31, min_acceptance_rate=0.)
    kw.update(more)
    return kw


def test_run_without_the_keyword_is_the_run_it_was():
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=6)
    plain = d3d.Run(cube, inst, max_iterations=8, **run_kw(var))
    none = d3d.Run(cube, inst, max_iterations=8, smoothness=None, **run_kw(var))
    flat = d3d.Run(cube, inst, max_iterations=8, smoothness={}, **run_kw(var))   # all sigmas infinite
    np.testing.assert_array_equal(none.chain, plain.chain)
    np.testing.assert_array_equal(flat.chain, plain.chain)
    np.testing.assert_array_equal(flat.likelihoods, plain.likelihoods)
    assert plain.smoothness is None and flat.smoothness == (np.inf,) * 3
    assert not plain.engine.prior_get()[1] and flat.engine.prior_get()[1]


# ---- chains=R ---------------------------------------------------------------------------------

@pytest.mark.parametrize("batched", [True, False])
def test_run_chains_share_the_prior_and_keep_their_own_parameters(batched):
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=6)
    R = 3
    sm = dict(a=2., c=1., w=0.5)
    many = d3d.Run.__new__(d3d.Run)
    many._batched = batched                 # both transports of _sweep_chains
    many.__init__(cube, inst, chains=R, max_iterations=9, smoothness=sm, **run_kw(var))
    assert many._batched is batched and many.smoothness == (2., 1., 0.5)
    for r in range(R):
        one = d3d.Run(cube, inst, max_iterations=9, smoothness=sm, **run_kw(var, seed=31 + r))
        np.testing.assert_array_equal(one.chain, many.chains[r])
        np.testing.assert_array_equal(one.likelihoods, many.all_likelihoods[r])
    plain = d3d.Run(cube, inst, max_iterations=9, **run_kw(var))
    assert not np.array_equal(plain.chain, many.chains[0])


def test_chip_filling_batched_form_with_the_prior_is_the_chains_alone():
    """k_mh_ws<..., BATCH> with two pending layers (tests/test_gpu_multiplet_variants.py's batched
    problem): every chain its own weights and parameters."""
    R = 4
    dims, fsf, lsf, data, var, mask, init = batch_problem()
    mn, mx = np.array([0.0, 0.0, 0.3]), np.array([30.0, dims[0] - 1.0, 6.0])

    def make(r):
        eng = _lib.Engine(dims, fsf.shape)
        eng.set_taps(fsf, lsf)
        eng.set_data(data * (1.0 + 0.1 * r), var * (1.0 + 0.05 * r), mask=mask)
        eng.set_params(init)
        eng.mh_config(mn, mx, 0.1, 900.0, seed=21 + r, refresh_every=0)
        eng.prior_begin(LAM * (1. + r))
        return eng

    alone = []
    for r in range(R):
        with make(r) as eng:
            acc = eng.mh_sweeps(2, 1)
            alone.append((eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(), acc))
    engs = [make(r) for r in range(R)]
    try:
        acc = ensemble.sweep_chains_batched(engs, 2, 1)
        assert [e.get_option("batch_layers") for e in engs] == [2] * R
        for r, eng in enumerate(engs):
            np.testing.assert_array_equal(eng.get_params(), alone[r][0])
            np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_ERR), alone[r][1])
            np.testing.assert_array_equal(eng.get_dlog(), alone[r][2])
            assert acc[r] == alone[r][3]
    finally:
        for e in engs:
            e.close()
    assert not np.array_equal(alone[0][0], alone[1][0])


# ---- d3d_prior_energy ---------------------------------------------------------------------------

def energy_map(name):
    rng = np.random.default_rng(17)
    if name == "1x1":
        H, W, mask = 1, 1, None
    elif name == "1xW":
        H, W, mask = 1, 9, None
    elif name == "35x37 half masked":
        H, W = 35, 37
        mask = (rng.random((H, W)) < 0.5).astype(np.float64)
    elif name == "no pairs":
        H, W = 6, 7
        mask = (np.indices((H, W)).sum(axis=0) % 2).astype(np.float64)     # a chequerboard
    else:                               # 90 000 cells: more than one block's share (65 536), 352 blocks asked for
        H, W = 300, 300
        mask = np.ones((H, W))
        mask[100:103, :] = 0
    return H, W, mask, rng.normal(size=(H, W, 3)) * [10., 3., 1.] + [20., 16., 2.]


@pytest.mark.parametrize("name", ["1x1", "1xW", "35x37 half masked", "no pairs", "300x300"])
def test_prior_energy_matches_numpy_and_repeats_bit_for_bit(name):
    H, W, mask, params = energy_map(name)
    D = 2
    with _lib.Engine((D, H, W), (3, 3)) as eng:
        eng.set_taps(np.full((3, 3), 1. / 9.), None)
        eng.set_data(np.ones((D, H, W)), None, var_scalar=1.0, mask=mask)
        want = PO.energy(params, np.ones((H, W)) if mask is None else mask)
        got = eng.prior_energy(params)
        assert got[3] == want[3]
        if want[3] == 0:
            assert got == (0., 0., 0., 0)
        else:
            np.testing.assert_allclose(got[:3], want[:3], rtol=1e-12, atol=0.)
        assert eng.prior_energy(params) == got                    # the same bits
        eng.set_params(params)
        assert eng.prior_energy() == got                          # NULL: the context's parameters
        with pytest.raises(ValueError, match="shape"):
            eng.prior_energy(np.zeros((H + 1, W, 3)))
    if name in ("1x1", "no pairs"):
        assert want == (0., 0., 0., 0)


# ---- refusals -----------------------------------------------------------------------------------

def test_refusals_by_status_code_and_exception():
    case = make_case("c1")
    lib = _lib.load()
    dims = (case["D"], case["H"], case["W"])
    H, W = dims[1:]
    nan, inf = float("nan"), float("inf")
    three = C.c_double * 3

    def last():
        return lib.d3d_last_error().decode()

    with engine_of(case) as eng:
        ctx = eng._ctx
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=1, refresh_every=0)
        for bad in ((-1., 0., 0.), (0., nan, 0.), (0., 0., inf), (0., -1e-300, 0.)):
            assert lib.d3d_prior_begin(ctx, three(*bad)) == _lib.ERR_INVALID, bad
            assert not eng.prior_get()[1]
        assert lib.d3d_prior_begin(ctx, None) == _lib.ERR_INVALID
        with pytest.raises(ValueError, match="lam"):
            eng.prior_begin([1., -2., 0.])
        eng.prior_begin(LAM)
        with pytest.raises(NotImplementedError, match="tile"):                       # not while it is on
            eng.set_tile(0, 0, W, 0, H, 0, W)
        with pytest.raises(NotImplementedError, match="parts"):
            eng.set_parts([[0, H // 2, 0, W], [H // 2, H, 0, W]], [0, 1])
        # the host-evaluated models' entry point
        eng.residual(fetch=False)
        n, D = 1, dims[0]
        with pytest.raises(NotImplementedError, match="host-evaluated"):
            eng.mh_colour_lines(1, np.zeros(n, dtype=np.int32), np.array([[1., 0., -1.]]), np.zeros((n, 2, D)))
        if _lib.has_experiments():
            for key in ("mh_chain", "mh_flow", "mh_pair"):
                with pytest.raises(NotImplementedError, match=key):
                    eng.set_option(key, 1)
        # after the refusals the context still runs its chain, with the prior
        assert eng.mh_sweeps(1, 1) >= 0 and eng.prior_get()[1]
        # d3d_window_stats keeps returning the likelihood terms only
        p_new = case["init"][5, 7] + np.array([0., 0.4, -0.1])
        with_prior = eng.window_stats(5, 7, p_new)
        eng.prior_end()
        eng.prior_end()                                                              # twice is fine
        np.testing.assert_array_equal(eng.window_stats(5, 7, p_new), with_prior)
        eng.set_parts([[0, H // 2, 0, W], [H // 2, H, 0, W]], [0, 1])                # more than one part
        assert lib.d3d_prior_begin(ctx, three(*LAM)) == _lib.ERR_UNSUPPORTED
        assert "parts" in last()
        with pytest.raises(NotImplementedError):
            eng.prior_begin(LAM)
    with _lib.Engine(dims, case["fsf"].shape) as eng:                                # a tile
        eng.set_tile(0, 0, W, 0, H, 0, W)
        assert lib.d3d_prior_begin(eng._ctx, three(*LAM)) == _lib.ERR_UNSUPPORTED
        assert "tile" in last()
        with pytest.raises(NotImplementedError):
            eng.prior_begin(LAM)
    for shape in ((1, 5), (5, 1)):                                                   # a 1 x N FSF
        with _lib.Engine(dims, shape) as eng:
            assert lib.d3d_prior_begin(eng._ctx, three(*LAM)) == _lib.ERR_INVALID
            assert "colour class" in last()
            with pytest.raises(ValueError, match="FSF"):
                eng.prior_begin(LAM)
    if _lib.has_experiments():
        for key in ("mh_chain", "mh_flow", "mh_pair"):
            with _lib.Engine(dims, case["fsf"].shape, options={key: 1}) as eng:
                with pytest.raises(NotImplementedError, match=key):
                    eng.prior_begin(LAM)
    assert lib.d3d_prior_begin(None, three(*LAM)) == _lib.ERR_INVALID
    assert lib.d3d_prior_end(None) == _lib.ERR_INVALID
    assert lib.d3d_prior_energy(None, None, three(), None) == _lib.ERR_INVALID


def test_run_refusals():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7)
    with pytest.raises(NotImplementedError, match="Lorentzian"):
        d3d.Run(cube, inst, model=Lorentzian, max_iterations=8, smoothness=dict(c=1.), **run_kw(var))
    with pytest.raises(ValueError, match="smoothness"):
        d3d.Run(cube, inst, max_iterations=8, smoothness=dict(c=-1.), **run_kw(var))
    inst1, cube1, var1, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7, fsf=np.array([[0.25, 0.5, 0.25]]))
    with pytest.raises(ValueError, match="1 x 3 FSF"):
        d3d.Run(cube1, inst1, max_iterations=8, smoothness=dict(c=1.), **run_kw(var1))


# ---- it composes, and checkpoints -----------------------------------------------------------------

def test_run_composes_with_adaptation_moments_search_preparation_and_a_doublet():
    ls = SHAPES["doublet"]
    inst, cube, var, _ = run_inputs(32, 12, 12, ls[0], ls[1], seed=8)
    run = d3d.Run(cube, inst, model=d3d.GaussianMultipletLineModel(*ls), max_iterations=31,
                  smoothness=(None, 1., 0.5), adapt_sweeps=20, adapt_window=5, posterior_burn_in=20,
                  initial_search=True, prepare=True, seed=4, min_acceptance_rate=0.)
    assert run.smoothness == (np.inf, 1., 0.5) and run.adapted_until == 20 and run.posterior.count == 11
    assert np.isfinite(run.parameters).all()
    lam, on = run.engine.prior_get()
    assert on and np.array_equal(lam, [0., 1., 4.])
    rough = run.roughness()
    assert rough == run.engine.prior_energy(run.parameters)
    np.testing.assert_allclose(rough[:3], PO.energy(run.parameters, run.mask)[:3], rtol=1e-12)
    assert rough[3] == 2 * 12 * 11


@pytest.mark.parametrize("at", [7])
def test_resume_with_the_prior_is_bit_for_bit_and_other_sigmas_are_refused(at, tmp_path):
    """refresh_every = 6: the uninterrupted run rebuilds its residual from the parameters at the very
    sweep where the resumed one starts from them (tests/test_gpu_adapt.py)."""
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7)
    mask = np.ones((12, 12))
    mask[3, 4] = mask[11, 0] = 0
    name = str(tmp_path / "ck")
    kw = run_kw(var, refresh_every=6, mask=mask, seed=3, smoothness=dict(c=1., a=3.))
    whole = d3d.Run(cube, inst, max_iterations=19, **kw)
    first = d3d.Run(cube, inst, max_iterations=at, write_every=at, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    np.testing.assert_array_equal(state["smoothness_sigmas"], [3., 1., np.inf])
    second = d3d.Run(cube, inst, max_iterations=19 - (at - 1), initial_parameters=name + "_parameters.npy",
                     resume_state=name + "_state.npz", **kw)
    np.testing.assert_array_equal(first.chain, whole.chain[:at])
    np.testing.assert_array_equal(second.chain[1:], whole.chain[at:])
    for other in (dict(c=0.5, a=3.), None):
        with pytest.raises(ValueError, match="smoothness"):
            d3d.Run(cube, inst, max_iterations=5, initial_parameters=name + "_parameters.npy",
                    resume_state=name + "_state.npz", **dict(kw, smoothness=other))
    plain = d3d.Run(cube, inst, max_iterations=19, **dict(kw, smoothness=None))
    assert not np.array_equal(plain.chain, whole.chain)


# ---- does it help? ----------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [12345, 7])
def test_the_prior_halves_the_error_of_the_centre_map(seed):
    """tests/test_prior_cpu.py's ordering on the device: oracle.synthetic_case(32, 12, 12), Gaussian
    FSF FWHM 3, LSF sigma 0.9088, started at the truth, 160 iterations, mean of the last 100."""
    D, H, W = 32, 12, 12
    fsf = O.gaussian_fsf_image(3.0)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, truth, _, _, _ = O.synthetic_case(D, H, W, fsf, lsf, seed=seed)
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    kw = dict(variance=var, initial_parameters=truth, seed=seed, min_acceptance_rate=0., max_iterations=160,
              refresh_every=0)
    rms, rough = {}, {}
    for name, sm in (("without", None), ("with", dict(c=1.))):
        run = d3d.Run(cube, inst, smoothness=sm, **kw)
        mean = np.mean(run.chain[60:160], axis=0)
        rms[name] = float(np.sqrt(np.mean((mean[..., 1] - truth[..., 1]) ** 2)))
        rough[name] = run.roughness(mean)
        np.testing.assert_allclose(rough[name][:3], PO.energy(mean, mask)[:3], rtol=1e-12)
    print("seed %d: rms error of the mean c map without %.3f, with sigma_c = 1 %.3f; roughness of c %.1f, %.1f"
          % (seed, rms["without"], rms["with"], rough["without"][1], rough["with"][1]))
    assert rms["with"] < 0.5 * rms["without"]
    assert rough["with"][1] < rough["without"][1]
