"""
GPU tests of the per-spaxel jump scales (d3d_adapt_*, Run(adapt_sweeps=N)).

The oracle has one amplitude vector, read at every O.mh_update: a sweep with a scale map walks
O.colour_order itself and sets st.amp = [0, 0.1 s[y,x], 0.1 s[y,x]] before each update.
Tolerances are those of chain_against_oracle (tests/test_gpu_multiplet.py): parameters 1e-9,
dlog 1e-8 relative, the carried residual 1e-11 of its peak, accepted counts equal.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests.cases import make_case
from tests.test_gpu_multiplet import SHAPES, multiplet, run_inputs

pytestmark = pytest.mark.gpu

JUMP = 0.1


def scale_map(shape, seed, lo=-2., hi=2.):
    """Scales over 10^lo .. 10^hi, both ends present."""
    s = 10. ** np.random.default_rng(seed).uniform(lo, hi, size=shape)
    s.flat[0], s.flat[-1] = 10. ** lo, 10. ** hi
    return s


def oracle_sweep(st, sweep, scale, counts):
    """One sweep in device order with per-spaxel amplitudes; counts[y, x] += accepted."""
    for (y, x) in O.colour_order(st.mask, *st.fsf.shape):
        st.amp = np.array([0., JUMP * scale[y, x], JUMP * scale[y, x]])
        counts[y, x] += bool(O.mh_update(st, y, x, sweep))


def compare_sweeps(eng, st, scale, first, n_sweeps):
    """n_sweeps of the device from sweep `first`, update by update against the oracle driven with
    `scale`.  Returns (device accepted, oracle per-spaxel accept counts)."""
    H, W = st.mask.shape
    chain = np.full((first + n_sweeps, H, W, 3), np.nan)
    dlog = np.full((first + n_sweeps, H, W), np.nan)
    accepted = eng.mh_sweeps(n_sweeps, first, 1, chain, dlog)
    err_dev = eng.download_slot(_lib.SLOT_ERR)
    live = st.mask == 1
    counts = np.zeros((H, W), dtype=np.int64)
    before = st.accepted
    for s in range(first, first + n_sweeps):
        oracle_sweep(st, s, scale, counts)
        np.testing.assert_allclose(chain[s][live], st.params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="params after sweep %d" % s)
        top = np.max(np.abs(st.dlog[live])) + 1.0
        np.testing.assert_allclose(dlog[s][live], st.dlog[live], rtol=1e-8, atol=1e-10 * top,
                                   err_msg="dlog sweep %d" % s)
    assert accepted == st.accepted - before
    assert np.max(np.abs(err_dev - st.err)) <= 1e-11 * np.max(np.abs(st.err)), "carried residual"
    return accepted, counts


def fixed_map_against_oracle(eng, data, var, mask, fsf, lsf, init, min_b, max_b, seed, n_sweeps=3):
    """window = 0 with a random map over four decades: the chain, then the counters."""
    st = O.MHState(data, var, mask, fsf, lsf, init, min_b, max_b, jump_amplitude=JUMP, seed=seed)
    scale = scale_map(mask.shape, seed)
    eng.set_params(init)
    eng.mh_config(min_b, max_b, JUMP, st.ra, seed=seed, refresh_every=0)
    eng.adapt_begin(window=0)
    eng.adapt_set(scale=scale)
    accepted, counts = compare_sweeps(eng, st, scale, 1, n_sweeps)
    got_scale, got_acc, n_win, k = eng.adapt_get()
    np.testing.assert_array_equal(got_scale, scale)             # a fixed map never moves
    np.testing.assert_array_equal(got_acc, counts)              # exactly the oracle's accepts
    assert int(got_acc.sum()) == accepted and (n_win, k) == (n_sweeps, 0)
    assert not got_acc[mask != 1].any()


def engine_of(case, options=None, line=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    if line is not None:
        eng.set_line_shape(*line)
    return eng


# ---- 1, 2: a fixed map against the oracle, and the counters ---------------------------------

@pytest.mark.parametrize("mh_props", [0, 1])
@pytest.mark.parametrize("name", ["c1", "odd_depth", "asym", "nolsf", "tiny", "uniform"])
def test_fixed_scale_map_matches_the_oracle_update_by_update(name, mh_props):
    """"uniform": c1 with one constant variance (the uniform-variance kernels)."""
    case = make_case("c1" if name == "uniform" else name)
    if name == "uniform":
        case["var"] = np.full(case["var"].shape, float(np.median(case["var"])))
    with engine_of(case, options={"mh_props": mh_props}) as eng:
        assert eng.variance_is_uniform() == (name == "uniform")
        fixed_map_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                                 case["init"], case["min_b"], case["max_b"], 777)


@pytest.mark.parametrize("mh_props", [0, 1])
@pytest.mark.parametrize("D,lsf_kind", [(128, "gauss"), (512, "gauss"), (600, "muse"), (1025, "muse")])
def test_fixed_scale_map_on_every_default_kernel_family(D, lsf_kind, mh_props):
    """The 5 x 6 problem of depth_chain_against_oracle (tests/test_gpu_multiplet.py): k_mh_small /
    k_mh_ws with 256 and 512 streaming threads, the z-blocked form, the thread-looped deep kernels."""
    H, W = 5, 6
    fsf = O.gaussian_fsf_image(1.6)
    lsf = O.gaussian_lsf_vector(D, 1.1) if lsf_kind == "gauss" else O.muse_like_lsf(D)
    rng = np.random.default_rng(D)
    truth = np.dstack((1 + 5 * rng.random((H, W)), D * (0.3 + 0.4 * rng.random((H, W))),
                       1.0 + 2 * rng.random((H, W))))
    mask = np.ones((H, W))
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    sigma = 0.05 * clean.max()
    data = clean + rng.normal(0, sigma, clean.shape)
    var = np.full(clean.shape, sigma ** 2)
    min_b = O.model_min_boundaries()
    max_b = O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.5)
    with _lib.Engine((D, H, W), fsf.shape, options={"mh_props": mh_props}) as eng:
        eng.set_taps(fsf, lsf)
        eng.set_data(data, var, mask=mask)
        fixed_map_against_oracle(eng, data, var, mask, fsf, lsf, init, min_b, max_b, 3)


def test_fixed_scale_map_composes_with_a_doublet(monkeypatch):
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES["doublet"]))
    case = make_case("c1")
    with engine_of(case, line=SHAPES["doublet"]) as eng:
        fixed_map_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                                 case["init"], case["min_b"], case["max_b"], 777)


# ---- 3: the rule ---------------------------------------------------------------------------

TARGET, WINDOW, GAIN, RANGE = 0.25, 5, 2.0, (0.5, 2.0)
LAST = 22                 # adapts after sweeps 5, 10, 15, 20; the window ending at 25 lies beyond
SEED = 777


def adaptive_engine(case, last_sweep, start):
    """c1 with a start map over two decades (so that both clamps of RANGE are hit at step 1)."""
    eng = engine_of(case)
    eng.set_params(case["init"])
    eng.mh_config(case["min_b"], case["max_b"], JUMP, float(case["max_b"][0] ** 2), seed=SEED, refresh_every=0)
    eng.adapt_begin(TARGET, WINDOW, last_sweep, GAIN, RANGE)
    eng.adapt_set(scale=start)
    return eng


def test_the_rule_window_by_window_against_numpy_and_the_oracle():
    case = make_case("c1")
    live = case["mask"] == 1
    start = np.where(live, scale_map(case["mask"].shape, 5, -1., 1.), 1.0)
    st = O.MHState(case["data"], case["var"], case["mask"], case["fsf"], case["lsf"], case["init"],
                   case["min_b"], case["max_b"], jump_amplitude=JUMP, seed=SEED)
    with adaptive_engine(case, LAST, start) as eng:
        scale = start
        for j in range(1, 5):
            # a twin that adapts to the previous step only keeps window j's counters
            with adaptive_engine(case, WINDOW * (j - 1), start) as twin:
                twin.mh_sweeps(WINDOW * j, 1)
                t_scale, t_acc, t_n, t_k = twin.adapt_get()
                twin_params = twin.get_params()
            np.testing.assert_array_equal(t_scale, scale)
            assert (t_n, t_k) == (WINDOW, j - 1)
            # the sweeps of window j against the oracle driven with the map of step j - 1
            _, counts = compare_sweeps(eng, st, scale, WINDOW * (j - 1) + 1, WINDOW)
            np.testing.assert_array_equal(t_acc, counts)
            np.testing.assert_array_equal(eng.get_params(), twin_params)
            want = np.clip(scale * np.exp(GAIN / np.sqrt(j) * (t_acc / float(WINDOW) - TARGET)), *RANGE)
            want = np.where(live, want, scale)                   # masked spaxels keep theirs
            got, acc, n_win, k = eng.adapt_get()
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=0.)
            np.testing.assert_array_equal(got[~live], 1.0)
            assert not acc.any() and (n_win, k) == (0, j)
            if j == 1:
                assert (got[live] == RANGE[0]).any() and (got[live] == RANGE[1]).any(), "both clamps"
            assert RANGE[0] <= got.min() and got.max() <= RANGE[1]
            scale = got
        # beyond last_sweep: no step, the map stays, the counters go on counting
        total = 0
        for j in (5, 6):
            accepted, counts = compare_sweeps(eng, st, scale, WINDOW * (j - 1) + 1, WINDOW)
            total += accepted
            got, acc, n_win, k = eng.adapt_get()
            np.testing.assert_array_equal(got, scale)
            assert (n_win, k) == (WINDOW * (j - 4), 4) and int(acc.sum()) == total
        final = (eng.get_params(), got, acc)
    # one call of 30 sweeps is the six calls of 5, bit for bit
    with adaptive_engine(case, LAST, start) as whole:
        whole.mh_sweeps(6 * WINDOW, 1)
        w_scale, w_acc, w_n, w_k = whole.adapt_get()
        np.testing.assert_array_equal(whole.get_params(), final[0])
        np.testing.assert_array_equal(w_scale, final[1])
        np.testing.assert_array_equal(w_acc, final[2])
        assert (w_n, w_k) == (2 * WINDOW, 4)


# ---- 4: off is off ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["c1", "depth600"])
def test_off_is_off_bit_for_bit(name):
    """Never begun, begun and ended, and a map of ones that never adapts: one chain."""
    if name == "c1":
        case = make_case("c1")
    else:                                    # (the z-blocked kernels: k_mh_zdecide decides)
        case = make_case("tile_deep")
    ra = float(case["max_b"][0] ** 2)

    def chain(prepare):
        with engine_of(case) as eng:
            eng.set_params(case["init"])
            eng.mh_config(case["min_b"], case["max_b"], JUMP, ra, seed=11, refresh_every=0)
            prepare(eng)
            accepted = eng.mh_sweeps(4, 1)
            return accepted, eng.get_params(), eng.download_slot(_lib.SLOT_ERR)

    def begin_end(eng):
        eng.adapt_begin(TARGET, 2, 4, GAIN, RANGE)
        eng.adapt_end()

    plain = chain(lambda eng: None)
    for prepare in (begin_end, lambda eng: eng.adapt_begin(window=0)):
        got = chain(prepare)
        assert got[0] == plain[0]
        np.testing.assert_array_equal(got[1], plain[1])
        np.testing.assert_array_equal(got[2], plain[2])
    # (and the scales do matter)
    moved = chain(lambda eng: eng.adapt_begin(TARGET, 2, 4, GAIN, RANGE))
    assert not np.array_equal(moved[1], plain[1])


# ---- 5, 6: Run -- chains=R, checkpoints ------------------------------------------------------

def adapt_kw(var, **more):
    kw = dict(variance=var, seed=31, min_acceptance_rate=0., adapt_sweeps=20, adapt_window=5)
    kw.update(more)
    return kw


@pytest.mark.parametrize("batched", [True, False])
def test_run_chains_adapt_from_their_own_counters(batched):
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=6)
    R = 3
    many = d3d.Run.__new__(d3d.Run)
    many._batched = batched                 # both transports of _sweep_chains
    many.__init__(cube, inst, chains=R, max_iterations=31, **adapt_kw(var))
    assert many._batched is batched and many.adapted_until == 20
    for r in range(R):
        one = d3d.Run(cube, inst, max_iterations=31, **adapt_kw(var, seed=31 + r))
        np.testing.assert_array_equal(one.chain, many.chains[r])
        np.testing.assert_array_equal(one.jump_scale, many.jump_scales[r])
        np.testing.assert_array_equal(one.acceptance_map, many.acceptance_maps[r])
        assert one.adapted_until == 20 and one.jump_scales == [one.jump_scale]
    assert not np.array_equal(many.jump_scales[0], many.jump_scales[1])
    rate = many.acceptance_map
    assert rate.shape == (12, 12) and np.all((rate >= 0.) & (rate <= 1.))
    # the counted sweeps are the ten after the freeze
    np.testing.assert_allclose(rate * 10., np.round(rate * 10.), rtol=0., atol=1e-12)
    plain = d3d.Run(cube, inst, variance=var, seed=31, min_acceptance_rate=0., max_iterations=31)
    assert plain.jump_scale is None and plain.acceptance_map is None and plain.adapted_until is None
    assert not np.array_equal(plain.chain, many.chains[0])


@pytest.mark.parametrize("at", [7, 25])
def test_resume_inside_and_after_the_adaptation_is_bit_for_bit(at, tmp_path):
    """A checkpoint after sweep 6 (inside window 2) and after sweep 24 (frozen).  refresh_every = 6:
    the uninterrupted run rebuilds its residual from the parameters at the very sweeps where the
    resumed one starts from them, so that the two can agree to the last bit at all."""
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7)
    mask = np.ones((12, 12))
    mask[3, 4] = mask[11, 0] = 0
    name = str(tmp_path / "ck")
    kw = adapt_kw(var, refresh_every=6, mask=mask, seed=3)
    whole = d3d.Run(cube, inst, max_iterations=31, **kw)
    first = d3d.Run(cube, inst, max_iterations=at, write_every=at, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    assert int(state["iteration"]) == at
    np.testing.assert_array_equal(state["adapt_keywords"], [20, 5, 0.25, 2.0, 1e-3, 1e3])
    assert state["adapt_scale"].shape == (1, 12, 12) and state["adapt_accepted"].dtype == np.uint32
    assert (int(state["adapt_n_win"][0]), int(state["adapt_k"][0])) == ((1, 1) if at == 7 else (4, 4))
    second = d3d.Run(cube, inst, max_iterations=31 - (at - 1), initial_parameters=name + "_parameters.npy",
                     resume_state=name + "_state.npz", **kw)
    np.testing.assert_array_equal(first.chain, whole.chain[:at])
    np.testing.assert_array_equal(second.chain[1:], whole.chain[at:])
    np.testing.assert_array_equal(second.jump_scale, whole.jump_scale)
    np.testing.assert_array_equal(second.acceptance_map, whole.acceptance_map)
    assert second.adapted_until == whole.adapted_until == 20
    assert np.isnan(whole.acceptance_map[mask == 0]).all() and np.isfinite(whole.acceptance_map[mask == 1]).all()
    np.testing.assert_array_equal(whole.jump_scale[mask == 0], 1.0)
    with pytest.raises(ValueError, match="adapt_window"):
        d3d.Run(cube, inst, max_iterations=5, initial_parameters=name + "_parameters.npy",
                resume_state=name + "_state.npz", **dict(kw, adapt_window=4))


def test_save_adds_the_maps(tmp_path):
    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7)
    run = d3d.Run(cube, inst, max_iterations=12, **adapt_kw(var, adapt_sweeps=6, adapt_window=3))
    run.save(str(tmp_path / "out"), clobber=True)
    z = np.load(str(tmp_path / "out_result.npz"))
    np.testing.assert_array_equal(z["jump_scale"], run.jump_scale)
    np.testing.assert_array_equal(z["acceptance_map"], run.acceptance_map)


# ---- 7: refusals -------------------------------------------------------------------------------

def test_refusals_by_status_code_and_exception():
    case = make_case("c1")
    lib = _lib.load()
    dims = (case["D"], case["H"], case["W"])
    nan, inf = float("nan"), float("inf")

    def last():
        return lib.d3d_last_error().decode()

    with engine_of(case) as eng:
        ctx = eng._ctx
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], JUMP, 50.0, seed=1, refresh_every=0)
        assert lib.d3d_adapt_get(ctx, None, None, None, None) == _lib.ERR_STATE      # not begun
        assert lib.d3d_adapt_set(ctx, None, None, 0, 0) == _lib.ERR_STATE
        bad = [(0., 5, 10, 2., 1e-3, 1e3), (1., 5, 10, 2., 1e-3, 1e3), (nan, 5, 10, 2., 1e-3, 1e3),
               (.25, -1, 10, 2., 1e-3, 1e3), (.25, 5, 10, 0., 1e-3, 1e3), (.25, 5, 10, -2., 1e-3, 1e3),
               (.25, 5, 10, nan, 1e-3, 1e3), (.25, 5, 10, 2., 0., 1e3), (.25, 5, 10, 2., 1e-3, inf),
               (.25, 5, 10, 2., nan, 1e3), (.25, 5, 10, 2., -1., 1.), (.25, 5, 10, 2., 2., 1.)]
        for args in bad:
            assert lib.d3d_adapt_begin(ctx, *args) == _lib.ERR_INVALID, args
            assert lib.d3d_adapt_get(ctx, None, None, None, None) == _lib.ERR_STATE  # nothing begun
        with pytest.raises(ValueError, match="target"):
            eng.adapt_begin(target=1.5)
        eng.adapt_begin(window=0)
        for v in (0., -1., nan, inf):
            m = np.ones(dims[1:])
            m[2, 3] = v
            with pytest.raises(ValueError, match=r"spaxel \(2, 3\)"):
                eng.adapt_set(scale=m)
        with pytest.raises(ValueError):
            eng.adapt_set(n_win=-1)
        with pytest.raises(ValueError, match="shape"):
            eng.adapt_set(scale=np.ones((3, 3)))
        np.testing.assert_array_equal(eng.adapt_get()[0], 1.0)                       # nothing installed
        assert lib.d3d_adapt_get(ctx, None, None, None, None) == 0                   # any pointer may be NULL
        with pytest.raises(NotImplementedError, match="tile"):                       # not while it is on
            eng.set_tile(0, 0, case["W"], 0, case["H"], 0, case["W"])
        if _lib.has_experiments():
            for key in ("mh_chain", "mh_flow", "mh_pair"):
                with pytest.raises(NotImplementedError, match=key):
                    eng.set_option(key, 1)
        # after the refusals the context still runs its chain
        plain = eng.mh_sweeps(2, 1)
        assert plain > 0 and int(eng.adapt_get()[1].sum()) == plain
        eng.adapt_end()
        eng.adapt_end()                                                              # twice is fine
        assert lib.d3d_adapt_get(ctx, None, None, None, None) == _lib.ERR_STATE
        assert eng.mh_sweeps(1, 3) >= 0
    with _lib.Engine(dims, case["fsf"].shape) as eng:                                # a tile
        eng.set_tile(0, 0, case["W"], 0, case["H"], 0, case["W"])
        assert lib.d3d_adapt_begin(eng._ctx, .25, 5, 10, 2., 1e-3, 1e3) == _lib.ERR_UNSUPPORTED
        assert "tile" in last()
        with pytest.raises(NotImplementedError):
            eng.adapt_begin()
    if _lib.has_experiments():
        for key in ("mh_chain", "mh_flow", "mh_pair"):
            with _lib.Engine(dims, case["fsf"].shape, options={key: 1}) as eng:
                with pytest.raises(NotImplementedError, match=key):
                    eng.adapt_begin()
    assert lib.d3d_adapt_begin(None, .25, 5, 10, 2., 1e-3, 1e3) == _lib.ERR_INVALID
    assert lib.d3d_adapt_end(None) == _lib.ERR_INVALID


def test_run_refusals_leave_nothing_behind():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    inst, cube, var, _ = run_inputs(16, 12, 12, [0.], [1.], seed=7)
    with pytest.raises(NotImplementedError, match="Lorentzian"):
        d3d.Run(cube, inst, model=Lorentzian, max_iterations=8, **adapt_kw(var, adapt_sweeps=6, adapt_window=3))
    with pytest.raises(ValueError, match="posterior_burn_in"):
        d3d.Run(cube, inst, max_iterations=31, posterior_burn_in=10, **adapt_kw(var))
    run = d3d.Run(cube, inst, max_iterations=31, posterior_burn_in=20, **adapt_kw(var))
    assert run.posterior.count == 11 and run.adapted_until == 20


# ---- 8: it helps -------------------------------------------------------------------------------

def test_adaptation_brings_the_acceptance_rates_to_the_target():
    """32x16x16, amplitudes over two decades (O.synthetic_case with A0 = 100 and a seeded
    per-spaxel dimming): after 20 adapted sweeps (windows of 5) more spaxels accept between half
    and twice the target over the next 40 sweeps than with every scale pinned at 1 (the same
    chain as without the keyword, counted alike), and the median distance from the target is
    smaller.  The CPU oracle, same rule and counts: shares 0.445 against 0.168 of 256 spaxels
    (binomial standard errors 0.031 and 0.023), medians 0.200 against 0.700."""
    D, H, W = 32, 16, 16
    fsf = O.gaussian_fsf_image(3.0)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    dim = 10. ** (-2. * np.random.default_rng(31).random((H, W)))

    def forward(truth):
        t = truth.copy()
        t[..., 0] = 100. * dim
        return O.forward_full((D, H, W), t, np.ones((H, W)), fsf, lsf)

    data, var, mask, _, init, _, _ = O.synthetic_case(D, H, W, fsf, lsf, seed=31, A0=100., fast_forward=forward)
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    kw = dict(variance=var, initial_parameters=init, seed=5, min_acceptance_rate=0., max_iterations=61,
              refresh_every=0, adapt_sweeps=20, adapt_window=5)
    adapted = d3d.Run(cube, inst, **kw)
    pinned = d3d.Run(cube, inst, adapt_scale_range=(1., 1.), **kw)
    plain = d3d.Run(cube, inst, **{k: v for k, v in kw.items() if not k.startswith("adapt_")})
    np.testing.assert_array_equal(pinned.chain, plain.chain)
    np.testing.assert_array_equal(pinned.jump_scale, 1.0)
    target = 0.25
    shares, medians = [], []
    for run in (adapted, pinned):
        rate = run.acceptance_map[mask == 1]
        shares.append(np.mean((rate >= target / 2.) & (rate <= 2. * target)))
        medians.append(np.median(np.abs(rate - target)))
    print("share in [target/2, 2 target]: adapted %.4f, pinned %.4f; median |rate - target|: %.4f, %.4f"
          % (shares[0], shares[1], medians[0], medians[1]))
    assert shares[0] > shares[1]
    assert medians[0] < medians[1]
