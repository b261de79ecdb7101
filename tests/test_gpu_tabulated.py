"""
GPU tests of the tabulated line model (TabulatedLineModel, d3d_set_line_table): every line build
of the device -- forward model, simulate, window statistics, the MH kernels of every depth class
and write-back scheme, batched chains, posterior moments and histograms, the search bank, Run
with its keywords, checkpoints -- against the oracle with its line patched to the independent
restatement of the interpolant (tests/tabulated_oracle.py; every oracle function builds its
lines through O.gaussian_line).

Profiles: (G) Gaussian, n = 2049, support 8; (S) skewed, n = 1025, support 6 -- a mirrored u or
a flipped table fails on it; (L) Lorentzian, n = 4097, support 40 -- reaches past both cube
edges and past the support; (C) 8 coarse samples with negative lobes, support 3.5.

Tolerances are the multiplet and chain tests' (tests/test_gpu_multiplet.py): cubes 1e-12 of the
peak, chain parameters rtol = atol = 1e-9, carried residual 1e-11 of its peak, accepted counts
equal; "bit for bit" is assert_array_equal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, ensemble, tiling
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import line_search_oracle as LS
from tests import tabulated_oracle as TO
from tests.cases import make_case
from tests.test_gpu_multiplet import assert_cube_close, chain_against_oracle
from tests.test_gpu_multiplet_variants import batch_problem
from tests.test_gpu_posterior import MAP_RTOL, close
from tests.test_gpu_tiling import compare

pytestmark = pytest.mark.gpu

DOUBLET = ([0., 3.8], [1., 1.4])


@functools.lru_cache(maxsize=None)
def model_of(key, doublet=False):
    tab, sup = TO.PROFILES[key]()
    if doublet:
        return d3d.TabulatedLineModel(tab, sup, offsets=DOUBLET[0], ratios=DOUBLET[1])
    return d3d.TabulatedLineModel(tab, sup)


def oracle_line(key, doublet=False):
    tab, sup = TO.PROFILES[key]()
    return TO.line(tab, sup, *(DOUBLET if doublet else ([0.], [1.])))


def set_model(eng, model):
    eng.set_line_shape(model.offsets, model.ratios)
    eng.set_line_table(model.table, model.support, model.table_integral)


def engine_for(case, model=None, options=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    if model is not None:
        set_model(eng, model)
    return eng


# ---- forward model ------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["S", "L", "C"])
@pytest.mark.parametrize("name", ["c1", "odd_depth", "d30", "nolsf", "tiny", "asym"])
def test_forward_simulate_and_residual_match_the_patched_oracle(name, key, monkeypatch):
    case = make_case(name)
    monkeypatch.setattr(O, "gaussian_line", oracle_line(key))
    dims = (case["D"], case["H"], case["W"])
    with engine_for(case, model_of(key)) as eng:
        eng.set_params(case["truth"])
        assert_cube_close(eng.forward(), O.forward_full(dims, case["truth"], case["mask"], case["fsf"],
                                                        case["lsf"]), "forward")
        clean = eng.simulate(case["init"], convolved=False)
        assert_cube_close(clean, O.simulate_clean(dims, case["init"], case["mask"]), "simulate clean")
        conv = eng.simulate(case["init"], convolved=True)
        assert_cube_close(conv, O.forward_full(dims, case["init"], case["mask"], case["fsf"], case["lsf"]),
                          "simulate convolved")
        eng.set_params(case["init"])
        ref_err = O.compute_error_in_one_step(case["data"], case["init"], case["mask"], case["fsf"], case["lsf"])
        assert_cube_close(eng.residual(), ref_err, "residual")
    with engine_for(case) as gauss:
        assert not np.allclose(gauss.simulate(case["init"], convolved=True), conv)


@pytest.mark.parametrize("name,key", [("c1", "S"), ("odd_depth", "L"), ("d30", "C"), ("nolsf", "S"),
                                      ("tiny", "C"), ("asym", "L")])
def test_window_stats_probe(name, key, monkeypatch):
    case = make_case(name)
    monkeypatch.setattr(O, "gaussian_line", oracle_line(key))
    rng = case["rng"]
    H, W = case["H"], case["W"]
    with engine_for(case, model_of(key)) as eng:
        eng.set_params(case["init"])
        err = eng.residual()
        spaxels = [(0, 0), (H - 1, W - 1), (0, W - 1), (H // 2, W // 2)]
        spaxels += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(6)]
        for (y, x) in spaxels:
            p_old = case["init"][y, x]
            p_new = p_old + np.array([0., 1., 0.3]) * np.tan(np.pi * (rng.random(3) - 0.5)) * 0.5
            p_new[2] = abs(p_new[2]) + 0.2
            got = eng.window_stats(y, x, p_new)
            ref = O.window_stats(err, case["var"], p_old, p_new, y, x, case["fsf"], case["lsf"])
            floor = 1e-12 * max(ref[0], ref[1])
            np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-10, atol=floor, err_msg="chi2 at %s" % ((y, x),))
            np.testing.assert_allclose(got[3:], ref[3:], rtol=1e-10, atol=1e-12 * max(abs(ref[3]), abs(ref[4])),
                                       err_msg="gibbs moments at %s" % ((y, x),))


def test_a_zero_width_line_is_a_delta_of_the_tables_centre_value():
    """w == 0: phi(0) at the channel d == 0, nothing elsewhere and nothing NaN, per component."""
    D, H, W = 16, 4, 4
    params = np.zeros((H, W, 3))
    params[..., 2] = 1.0
    params[1, 2] = [3.0, 10.0, 0.0]
    model = d3d.TabulatedLineModel([0., -0.3, 0.2, 1., 0.6, 0.1, -0.1, 0., 0.], 4.,       # phi(0) = 0.6
                                   offsets=[0., 3., 2.5], ratios=[1., 0.5, 1.])
    with _lib.Engine((D, H, W), (1, 1)) as eng:
        eng.set_taps(np.ones((1, 1)), None)
        eng.set_data(np.ones((D, H, W)), None, 1.0)
        set_model(eng, model)
        eng.set_params(params)
        clean = eng.build_clean()
    assert np.isfinite(clean).all()
    want = np.zeros(D)
    want[10], want[13] = 3.0 * 0.6, 3.0 * (0.5 * 0.6)
    np.testing.assert_array_equal(clean[:, 1, 2], want)
    np.testing.assert_array_equal(clean[:, 1, 2], model.modelize(None, np.arange(16.), params[1, 2]))


# ---- the chain against the oracle -----------------------------------------------------------------

@pytest.mark.parametrize("name,key,doublet", [("c1", "S", False), ("odd_depth", "L", False), ("d30", "C", True),
                                              ("uniform", "S", False)])
def test_mh_chain_matches_the_patched_oracle_update_by_update(name, key, doublet, monkeypatch):
    """"uniform": c1 with one constant variance (the uniform-variance kernels)."""
    monkeypatch.setattr(O, "gaussian_line", oracle_line(key, doublet))
    case = make_case("c1" if name == "uniform" else name)
    if name == "uniform":
        case["var"] = np.full(case["var"].shape, float(np.median(case["var"])))
    with engine_for(case, model_of(key, doublet)) as eng:
        if name == "uniform":
            assert eng.variance_is_uniform()
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             case["init"], case["min_b"], case["max_b"], 3, 777)


# ---- kernel variants of the default build ---------------------------------------------------------

def run_variant(case, model, opts, sweeps=3):
    with engine_for(case, model, options=opts) as eng:
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)
        acc = eng.mh_sweeps(sweeps - 1, 1)
        mid = eng.download_slot(_lib.SLOT_ERR)          # flushes the pending colour
        acc += eng.mh_sweeps(1, sweeps)                 # and the chain continues consistently
        return eng.get_params(), mid, eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(), np.int64(acc)


def assert_same_bits(a, b, what):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v, err_msg=what)


SCHEMES = [{"mh_defer": d, "mh_small": s} for d in (1, 0, 2) for s in (1, 0)]


@pytest.mark.parametrize("name,key,doublet", [("c1", "S", False), ("odd_depth", "C", True), ("tiny", "L", False)])
def test_write_back_schemes_are_bit_identical_with_a_table(name, key, doublet, monkeypatch):
    """mh_defer = 1 (k_mh_ws<..., true>, or k_mh_small on a line table of the tabulated line),
    2 (k_mh_defer<..., true>) and 0 (k_mh<..., true>), each with and without k_mh_small: the same
    bits; and the first against the patched oracle."""
    case = make_case(name)
    model = model_of(key, doublet)
    outs = [run_variant(case, model, opts) for opts in SCHEMES]
    for opts, other in zip(SCHEMES[1:], outs[1:]):
        assert_same_bits(outs[0], other, str(opts))
    monkeypatch.setattr(O, "gaussian_line", oracle_line(key, doublet))
    with engine_for(case, model, options=SCHEMES[0]) as eng:
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             case["init"], case["min_b"], case["max_b"], 3, 777)


def depth_case(D):
    """The 5 x 6 problem of tests/test_gpu_multiplet.py::depth_chain_against_oracle at depth D
    (Gaussian LSF up to 512 channels, the MUSE-like one -- taps within +-8 channels, what the
    z-blocked kernels take -- beyond), its data simulated with single Gaussians."""
    H, W = 5, 6
    fsf = O.gaussian_fsf_image(1.6)
    lsf = O.gaussian_lsf_vector(D, 1.1) if D <= 512 else O.muse_like_lsf(D)
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
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, truth=truth, mask=mask, data=data, var=var,
                min_b=min_b, max_b=max_b, init=init)


@pytest.mark.parametrize("D,key,doublet", [(300, "S", False), (512, "C", True), (600, "L", False),
                                           (1030, "S", True)])
def test_every_depth_class_with_a_table(D, key, doublet, monkeypatch):
    """300 and 512 channels: k_mh_ws<512, ..., true>, k_mh_defer<512, true> and k_mh<512, 0, true>,
    the same bits.  600 and 1030 channels: the z-blocked k_mh_ws with k_mh_zdecide (one and two
    pending layers, bit for bit) against the plain kernels (mh_zblocks = 0: k_mh_defer<1024, true>
    at 600, k_mh_deep<true> at 1030) -- another grouping of the channel sums, so to rounding, as
    tests/test_gpu_edges.py holds them.  The forward model and the first variant's chain against
    the patched oracle."""
    case = depth_case(D)
    model = model_of(key, doublet)
    live = case["mask"] == 1
    if D <= 512:
        outs = [run_variant(case, model, opts) for opts in SCHEMES]
        for opts, other in zip(SCHEMES[1:], outs[1:]):
            assert_same_bits(outs[0], other, str(opts))
        first = SCHEMES[0]
    else:
        zb = [{"mh_zblocks": 1}, {"mh_zblocks": 1, "mh_small": 0}, {"mh_zblocks": 1, "mh_layers": 2}]
        outs = [run_variant(case, model, opts) for opts in zb]
        for opts, other in zip(zb[1:], outs[1:]):
            assert_same_bits(outs[0], other, str(opts))
        plain = run_variant(case, model, {"mh_zblocks": 0})
        np.testing.assert_allclose(outs[0][0][live], plain[0][live], rtol=1e-9, atol=1e-9)
        assert np.max(np.abs(outs[0][2] - plain[2])) <= 1e-11 * np.max(np.abs(plain[2]))
        assert outs[0][4] == plain[4]
        first = zb[0]
    monkeypatch.setattr(O, "gaussian_line", oracle_line(key, doublet))
    dims = (case["D"], case["H"], case["W"])
    with engine_for(case, model, options=first) as eng:
        eng.set_params(case["truth"])
        assert_cube_close(eng.forward(), O.forward_full(dims, case["truth"], case["mask"], case["fsf"],
                                                        case["lsf"]), "forward")
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             case["init"], case["min_b"], case["max_b"], 2, 3)


# ---- batched chains ---------------------------------------------------------------------------------

def test_batched_chains_are_the_chains_alone_and_share_one_table():
    R = 3
    model = model_of("S", True)
    dims, fsf, lsf, data, var, mask, init = batch_problem()
    mn, mx = np.array([0.0, 0.0, 0.3]), np.array([30.0, dims[0] - 1.0, 6.0])

    def make(r, m=model):
        eng = _lib.Engine(dims, fsf.shape)
        eng.set_taps(fsf, lsf)
        eng.set_data(data * (1.0 + 0.1 * r), var * (1.0 + 0.05 * r), mask=mask)
        if m is not None:
            set_model(eng, m)
        start = init.copy()
        start[..., 2] = np.clip(start[..., 2] + 0.05 * r, 0.3, 6.0)
        eng.set_params(start)
        eng.mh_config(mn, mx, 0.1, 900.0, seed=21 + r, refresh_every=0)
        return eng

    alone = []
    for r in range(R):
        with make(r) as eng:
            acc = eng.mh_sweeps(2, 1) + eng.mh_sweeps(1, 3)
            alone.append((eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(), acc))
    engs = [make(r) for r in range(R)]
    try:
        a1 = ensemble.sweep_chains_batched(engs, 2, 1)
        a2 = ensemble.sweep_chains_batched(engs, 1, 3)
        for r, eng in enumerate(engs):
            np.testing.assert_array_equal(eng.get_params(), alone[r][0])
            np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_ERR), alone[r][1])
            np.testing.assert_array_equal(eng.get_dlog(), alone[r][2])
            assert a1[r] + a2[r] == alone[r][3]
    finally:
        for e in engs:
            e.close()
    # contexts that differ in the table -- one sample, the support, or table against none -- share no launch
    tab, sup = TO.profile_S()
    other = tab.copy()
    other[500] *= 1.001
    for m in (d3d.TabulatedLineModel(other, sup, *DOUBLET), d3d.TabulatedLineModel(tab, sup + 0.5, *DOUBLET),
              d3d.GaussianMultipletLineModel(*DOUBLET)):
        engs = [make(0), make(1, None)]
        try:
            engs[1].set_line_shape(m.offsets, m.ratios)
            if isinstance(m, d3d.TabulatedLineModel):
                engs[1].set_line_table(m.table, m.support, m.table_integral)
            with pytest.raises(ValueError, match="line shape"):
                ensemble.sweep_chains_batched(engs, 1, 1)
            rc = _lib.load().d3d_mh_sweeps_batch((C.c_void_p * 2)(*[e._ctx.value for e in engs]), 2, 1, 1, 1,
                                                 None, None, (C.c_int64 * 2)())
            assert rc == _lib.ERR_INVALID
        finally:
            for e in engs:
                e.close()


# ---- tiled and partitioned chains ---------------------------------------------------------------------

def test_tiled_chain_with_a_table_is_the_partitioned_single_context(monkeypatch):
    """tiling.make_tile_engine(line_table=...): every tile builds the tabulated doublet -- its own
    windows and the neighbours' replayed updates (k_apply_updates<..., true>) --, so the tiled
    chain is the partitioned single context's bit for bit."""
    model = model_of("S", True)
    case = make_case("tile_a")
    fh, fw = case["fsf"].shape
    ra, seed, sweeps = 35.0, 77, 3
    lay = tiling.TileLayout(case["H"], case["W"], fh, fw, 2, 2)
    with engine_for(case, model) as ref:
        tiling.apply_parts(ref, lay)
        ref.set_params(case["init"])
        ref.mh_config(case["min_b"], case["max_b"], 0.1, ra, seed=seed, refresh_every=0)
        err0 = ref.residual()
        accepted = ref.mh_sweeps(sweeps, 1)
        ref_params, ref_err = ref.get_params(), ref.download_slot(_lib.SLOT_ERR)
    assert accepted > 0
    engines = [tiling.make_tile_engine(lay, r, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                                       case["init"], case["min_b"], case["max_b"], 0.1, ra, seed, err=err0,
                                       line_shape=(model.offsets, model.ratios),
                                       line_table=(model.table, model.support, model.table_integral))
               for r in range(lay.n)]
    try:
        tables = [tiling.plan_tables(lay, r) for r in range(lay.n)]
        for s in range(1, sweeps + 1):
            tiling.sweep_loopback(engines, lay, tables, s, device_copy=True)
        compare(case, lay, engines, ref_params, ref_err)
        assert sum(e.mh_accepted() for e in engines) == accepted
    finally:
        for e in engines:
            e.close()


# ---- (G) against the analytic Gaussian ----------------------------------------------------------------

def test_the_gaussian_table_is_the_gaussian_model_to_the_interpolation_error():
    """|forward(table G) - forward(Gaussian)| <= 2 a_max e, e the largest difference between the
    restated interpolant and exp(-u^2/2) on a dense grid of u (the factor 2 covers the LSF and
    FSF sums of absolute taps, 1 each for normalised non-negative taps)."""
    tab, sup = TO.profile_G()
    model = model_of("G")
    u = np.concatenate((np.linspace(-9., 9., 40001), np.random.default_rng(1).uniform(-8., 8., 20000)))
    tabn = TO.normalised(tab)
    e = max(abs(TO.phi_scalar(tabn, sup, float(v), 1.) - np.exp(-v * v / 2.)) for v in u)
    print("largest |interpolant - exp(-u^2/2)| = %.3e" % e)
    assert 0. < e < 1e-6
    case = make_case("c1")
    assert (case["fsf"] >= 0).all() and abs(case["fsf"].sum() - 1.) < 1e-12 and (case["lsf"] >= 0).all()
    a_max = float(np.max(case["truth"][..., 0]))
    with engine_for(case, model) as eng:
        eng.set_params(case["truth"])
        got = eng.forward()
    with engine_for(case) as eng:
        eng.set_params(case["truth"])
        want = eng.forward()
    d = float(np.max(np.abs(got - want)))
    print("forward: max|table - Gaussian| = %.3e, bound %.3e" % (d, 2. * a_max * e))
    assert 0. < d <= 2. * a_max * e


# ---- setting, clearing, switching ----------------------------------------------------------------------

def test_a_cleared_table_leaves_a_fresh_context():
    case = make_case("c1")

    def go(eng):
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)
        acc = eng.mh_sweeps(2, 1)
        return eng.simulate(case["truth"], convolved=True), eng.get_params(), eng.download_slot(_lib.SLOT_ERR), acc

    with engine_for(case) as fresh:
        want = go(fresh)
    with engine_for(case, model_of("S")) as eng:
        with_table = eng.simulate(case["truth"], convolved=True)
        eng.set_line_table(None)
        got = go(eng)
    assert not np.array_equal(with_table, want[0])
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_setting_a_table_mid_chain_flushes_the_pending_layers(monkeypatch):
    """Default options on c1 (a pending layer in play at the switch): two sweeps of Gaussians, the
    table (S), two more sweeps.  The second segment is, bit for bit, a fresh context given the
    first segment's final parameters; its carried residual is data - forward model."""
    case = make_case("c1")
    dims = (case["D"], case["H"], case["W"])
    model = model_of("S")

    def configure(eng, params):
        eng.set_params(params)
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)

    with engine_for(case) as eng:
        configure(eng, case["init"])
        eng.mh_sweeps(2, 1)
        mid = eng.get_params()                        # (no download of the residual: nothing flushed)
        set_model(eng, model)
        acc = eng.mh_sweeps(2, 3)
        end, err = eng.get_params(), eng.download_slot(_lib.SLOT_ERR)
    with engine_for(case, model) as fresh:
        configure(fresh, mid)
        assert fresh.mh_sweeps(2, 3) == acc
        np.testing.assert_array_equal(fresh.get_params(), end)
        np.testing.assert_array_equal(fresh.download_slot(_lib.SLOT_ERR), err)
    monkeypatch.setattr(O, "gaussian_line", oracle_line("S"))
    want = case["data"] - O.forward_full(dims, end, case["mask"], case["fsf"], case["lsf"])
    assert np.max(np.abs(err - want)) <= 1e-11 * np.max(np.abs(want))


def dbl(values):
    return (C.c_double * len(values))(*values)


def test_d3d_set_line_table_refuses_invalid_tables_and_keeps_the_old_one():
    lib = _lib.load()
    case = make_case("c1")
    good = [0., 0.2, 0.6, 1., 0.5, 0.2, 0.1, 0.]
    bad = [
        ("n = 7", 7, 3., good[:7]),
        ("n = 65538", 65538, 3., [1.] * 65538),
        ("support 0", 8, 0., good),
        ("support NaN", 8, float("nan"), good),
        ("support < 0", 8, -3., good),
        ("support inf", 8, float("inf"), good),
        ("NaN sample", 8, 3., good[:5] + [float("nan")] + good[6:]),
        ("all zero", 8, 3., [0.] * 8),
        ("peak not 1", 8, 3., [2. * v for v in good]),
        ("negative peak", 8, 3., [-v for v in good]),
        ("NULL table", 8, 3., None),
        ("negative n", -1, 3., good),
    ]
    with engine_for(case, model_of("S")) as eng:
        before = eng.simulate(case["truth"], convolved=True)
        for what, n, support, tab in bad:
            rc = lib.d3d_set_line_table(eng._ctx, n, support, None if tab is None else dbl(tab), 1.)
            assert rc == _lib.ERR_INVALID, what
            assert lib.d3d_last_error(), what
            np.testing.assert_array_equal(eng.simulate(case["truth"], convolved=True), before, err_msg=what)
        assert lib.d3d_set_line_table(None, 8, 3., dbl(good), 1.) == _lib.ERR_INVALID
        assert lib.d3d_set_line_table(None, 0, 0., None, 0.) == _lib.ERR_INVALID
        # d3d_set_line_shape leaves the table alone
        eng.set_line_shape([0.], [1.])
        np.testing.assert_array_equal(eng.simulate(case["truth"], convolved=True), before)
        # and a valid call still works
        assert lib.d3d_set_line_table(eng._ctx, 8, 3., dbl(good), 1.) == 0
        assert not np.array_equal(eng.simulate(case["truth"], convolved=True), before)


def test_options_without_a_tabulated_form_are_refused_not_ignored():
    case = make_case("c1")
    case["lsf"] = O.muse_like_lsf(case["D"])        # taps within +-8 channels: the dense line kernel applies
    with engine_for(case, options={"lines_dense": 2}) as eng:
        eng.set_params(case["truth"])
        single = eng.forward()
        set_model(eng, model_of("S"))
        with pytest.raises(NotImplementedError, match="tabulated form"):
            eng.forward()
        eng.set_option("lines_dense", 1)
        assert not np.array_equal(eng.forward(), single)
        eng.set_option("lines_dense", 2)
        eng.set_line_table(None)
        np.testing.assert_array_equal(eng.forward(), single)


# ---- posterior ------------------------------------------------------------------------------------------

def tab_run_inputs(D, H, W, key, doublet, seed, noise=0.05, fsf=None):
    """A Run()-ready cube whose lines are the table's (tests/test_gpu_multiplet.py::run_inputs)."""
    fsf = O.moffat_cropped(11, 3.0, 2.5) if fsf is None else fsf
    lsf = O.muse_like_lsf(D)
    rng = np.random.default_rng(seed)
    y, x = np.indices((H, W))
    r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
    truth = np.dstack((10. * np.exp(-r2 / (2. * (H / 4.) ** 2)) + 0.5,
                       D / 2.5 + 2. * np.tanh((x - W / 2.) / (W / 4.)),
                       rng.uniform(1.4, 2.2, size=(H, W))))
    clean = np.zeros((D, H, W))
    line = oracle_line(key, doublet)
    for (yy, xx) in zip(y.ravel(), x.ravel()):
        clean[:, yy, xx] = O.spectral_convolve(line(np.arange(D), *truth[yy, xx]), lsf)
    clean = O.spatial_convolve(clean, fsf)
    sigma = noise * clean.max()
    data = clean + rng.normal(0., sigma, clean.shape)
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    return inst, cube, np.full(data.shape, sigma ** 2), truth


def test_posterior_flux_takes_the_tables_factor():
    model = model_of("S", True)
    inst, cube, var, _ = tab_run_inputs(32, 16, 16, "S", True, seed=5)
    run = d3d.Run(cube, inst, model=model, variance=var, max_iterations=12, seed=31, min_acceptance_rate=0.,
                  keep_one_in=1, posterior_burn_in=4)
    assert not run._host_model
    slots = run.chain[4:]
    pm = run.posterior
    assert pm.count == len(slots) == 8
    assert abs(model.flux_factor - 2.4 * TO.trapezoid(*TO.profile_S())) < 1e-12
    close(pm.flux_mean, np.mean(slots[..., 0] * slots[..., 2], axis=0) * model.flux_factor, MAP_RTOL, "flux mean")
    close(pm.parameters_mean, slots.mean(axis=0), MAP_RTOL, "parameters mean")
    cubes = np.stack([run.simulate_convolved(cube.data.shape, s) for s in slots])
    close(pm.convolved_mean, cubes.mean(axis=0), 1e-12, "convolved mean")


def test_histogram_flux_bounds_take_the_tables_factor():
    case = make_case("c1")
    model = model_of("L")
    with engine_for(case, model) as eng:
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)
        eng.post_begin()
        eng.post_schedule(1, 1)
        eng.hist_begin(3, 1e12)          # (a span beyond every bound: the frozen ranges are the bounds)
        eng.mh_sweeps(5, 1)
        bins, tails, rng = eng.hist_get()
    live = case["mask"] == 1
    top = float(np.max(rng[live][:, 3, 1]))
    want = case["max_b"][0] * case["max_b"][2] * model.flux_factor
    assert abs(top - want) <= 1e-14 * want, (top, want)
    assert abs(model.flux_factor - np.sqrt(2. * np.pi)) > 0.3          # (not the Gaussian's factor)
    assert float(np.min(rng[live][:, 3, 0])) == 0.


# ---- search, Run ----------------------------------------------------------------------------------------

def test_line_search_builds_its_bank_from_the_table():
    model = model_of("S")
    D, H, W = 32, 16, 16
    fsf = O.gaussian_fsf_image(3.0)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask = O.synthetic_case(D, H, W, fsf, lsf, seed=4242)[:3]
    centres, widths = LS.default_grid(D)
    bank = LS.template_bank(D, lsf, centres, widths, model)
    want_best, want_stat, gap = LS.statistic(data, var, mask, bank, centres.size)
    assert gap >= 1e-7
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    found = d3d.line_search(d3d.MUSE().build_cube(data), inst, variance=var, mask=mask, model=model)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        eng.set_data(data, var, mask=mask)
        set_model(eng, model)
        best, stat = eng.line_search(centres, widths)
        eng.set_line_table(None)
        gauss_best, _ = eng.line_search(centres, widths)
    np.testing.assert_array_equal(best, want_best)
    det = want_best >= 0
    assert det.any() and (stat[~det] == 0.).all()
    np.testing.assert_allclose(stat[det][:, :2], want_stat[det][:, :2], rtol=1e-10, atol=0.)
    assert not np.array_equal(gauss_best, best)
    np.testing.assert_array_equal(found.detected, det)
    np.testing.assert_array_equal(found.best_index, want_best)


def test_run_takes_every_keyword_with_a_table_and_refuses_them_for_a_host_model():
    model = model_of("S")
    inst, cube, var, _ = tab_run_inputs(32, 16, 16, "S", False, seed=6)
    kw = dict(variance=var, max_iterations=30, seed=3, min_acceptance_rate=0., initial_search=True,
              adapt_sweeps=10, adapt_window=5, smoothness=dict(c=1.), posterior_burn_in=20, chains=2)
    run = d3d.Run(cube, inst, model=model, **kw)
    assert not run._host_model and run.search is not None
    assert len(run.posteriors) == 2 and run.posteriors[0].count == 10
    assert np.isfinite(run.chains[0]).all() and np.isfinite(run.chains[1]).all()
    assert not np.array_equal(run.chains[0][-1], run.chains[1][-1])

    class Host(d3d.TabulatedLineModel):
        def modelize(self, runner, x, parameters):
            return d3d.TabulatedLineModel.modelize(self, runner, x, parameters)

    with pytest.raises(NotImplementedError, match="evaluated on the host"):
        d3d.Run(cube, inst, model=Host(*TO.profile_S()), **kw)


def test_checkpoint_and_resume_with_a_table(tmp_path):
    model = model_of("S", True)
    inst, cube, var, _ = tab_run_inputs(32, 12, 12, "S", True, seed=7)
    name = str(tmp_path / "ck")
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, model=model)
    whole = d3d.Run(cube, inst, max_iterations=13, **kw)
    first = d3d.Run(cube, inst, max_iterations=7, write_every=7, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    assert str(state["line_table_digest"]) == model.digest()
    np.testing.assert_array_equal(state["line_offsets"], DOUBLET[0])
    resume = dict(max_iterations=7, initial_parameters=name + "_parameters.npy", resume_state=name + "_state.npz")
    second = d3d.Run(cube, inst, **resume, **kw)
    again = d3d.Run(cube, inst, **resume, **kw)
    np.testing.assert_array_equal(first.chain[-1], np.load(name + "_parameters.npy"))
    np.testing.assert_array_equal(second.chain, again.chain)            # the same table: the same continuation
    # (the resumed run rebuilds the residual from the parameters: rounding-level differences)
    np.testing.assert_allclose(second.chain[-1], whole.chain[-1], rtol=1e-8, atol=1e-8)
    tab, sup = TO.profile_S()
    other = tab.copy()
    other[500] = np.nextafter(other[500], 0.)
    for bad in (d3d.TabulatedLineModel(other, sup, *DOUBLET), d3d.GaussianMultipletLineModel(*DOUBLET)):
        with pytest.raises(ValueError, match="line table"):
            d3d.Run(cube, inst, **resume, **dict(kw, model=bad))


def test_the_skewed_table_fits_skewed_data_better_than_a_gaussian():
    """Data simulated with (S) on 32 x 12 x 12; the same number of sweeps from the same start: the
    total chi2 of the (S) fit lies below that of the single-Gaussian fit.  Only the order is
    asserted."""
    inst, cube, var, truth = tab_run_inputs(32, 12, 12, "S", False, seed=8, noise=0.02,
                                            fsf=O.gaussian_fsf_image(1.0))
    kw = dict(variance=var, max_iterations=200, seed=21, min_acceptance_rate=0., initial_parameters=truth)
    fit = d3d.Run(cube, inst, model=model_of("S"), **kw)
    single = d3d.Run(cube, inst, model=d3d.SingleGaussianLineModel, **kw)

    def chi2(run):
        sim = run.simulate_convolved(cube.data.shape, run.chain[-1])
        return float(np.sum((cube.data - sim) ** 2 / var))

    print("chi2 of the last sample: table (S) %.1f, single Gaussian %.1f, %d voxels"
          % (chi2(fit), chi2(single), cube.data.size))
    assert chi2(fit) < chi2(single)
