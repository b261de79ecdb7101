"""
Pointwise predictive accuracy on the device (csrc/d3d_pred.hip, Run(predictive=...)): the four
accumulators k_pred_accum keeps are tests/predictive_oracle.py's from the device's own residual at
every shape, with NaN voxels, zero variances and the pad channel; the maps and cubes are the
oracle's extraction of them; one sample is the chi2 map and that state's log density; the Student-t
marginal uses the base variance; through Run the chain is untouched, chains pool exactly, tempering
follows rung 0; and the doublet that made a cube beats the single Gaussian on it.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import predictive_oracle as PO
from tests.cases import make_case
from tests.test_gpu_multiplet import multiplet
from tests.test_gpu_run import synthetic_cube

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RESIDUAL_BOUND = 1e-11        # the project's bound on a carried residual, in units of max|data|


def holed(case):
    """The case with NaN voxels and zero variances (tests/test_gpu_edges.py:
    test_nan_voxels_and_zero_variance); at least the first spaxel keeps a whole spectrum."""
    D, H, W = case["D"], case["H"], case["W"]
    data, var = case["data"].copy(), case["var"].copy()
    data[D // 3, 1 % H, 2 % W] = np.nan
    data[D - 1, H - 1, 1 % W] = np.nan            # (the last channel: beside the pad of an odd depth)
    var[0, 0, 0] = var[D // 2, H - 1, W - 1] = 0.0
    return dict(case, data=data, var=var)


def deep_case():
    """300 channels: 150 channel pairs, so every lane walks two or three of them."""
    D, H, W = 300, 4, 5
    fsf = O.gaussian_fsf_image(1.5)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, truth, init, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=31)
    var = var * (0.5 + np.random.default_rng(31).random(var.shape)) ** 2
    return dict(name="deep", D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, truth=truth,
                init=init, min_b=min_b, max_b=max_b)


def case_of(name):
    return holed(deep_case() if name == "deep" else make_case(name))


def engine_of(case, options=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    eng.set_params(case["init"])
    eng.mh_config(case["min_b"], case["max_b"], 0.1, 35.0, seed=77, refresh_every=0)
    return eng


def sequence(case):
    """Six samples of five maps: one far from the truth, first and last."""
    rng = np.random.default_rng(9)
    truth, far = case["truth"], case["init"]
    near = [np.clip(truth * (1. + 0.03 * rng.normal(size=truth.shape)), case["min_b"], case["max_b"])
            for _ in range(3)]
    return [far, truth, near[0], near[1], near[2], far]


def lppd_margin(i0, M, n, nu=0):
    """|device lppd - numpy lppd| where both take (k + M) + log(S / n) from the same accumulators:
    two logarithms of a few ulp each and two roundings of sums, 8 eps of the sum of the terms' sizes;
    the Student-t constant adds two lgamma values from two libraries, a few ulp of their own size."""
    import math
    gammas = math.lgamma(0.5 * (nu + 1.)) + math.lgamma(0.5 * nu) if nu else 0.
    with np.errstate(divide="ignore"):
        return 8. * EPS * (np.abs(np.log(np.where(i0 != 0., i0, 1.))) + np.abs(M) + np.log(max(n, 2)) + 1.
                           + abs(gammas))


def check_extraction(eng, n, i0, nu=0):
    """Maps and cubes against the oracle's extraction of the device's own accumulators."""
    M, S, mean, m2 = eng.pred_get()
    lppd, p = eng.pred_cubes()
    want_lppd, want_p = PO.extract(n, M, S, m2, i0, nu)
    live = i0 != 0.
    assert np.isnan(lppd[~live]).all() and np.isnan(p[~live]).all()          # NaN exactly where i0 == 0
    assert np.isfinite(lppd[live]).all()
    worst = np.max(np.abs(lppd - want_lppd)[live] / lppd_margin(i0, M, n, nu)[live])
    print("lppd cube: largest deviation in units of the margin", worst)
    assert worst <= 1.
    np.testing.assert_array_equal(p[live], want_p[live])                      # M2 / (n - 1): one division
    assert np.isnan(p[live]).all() == (n < 2)
    maps = eng.pred_maps()
    np.testing.assert_array_equal(maps, PO.fold_maps(lppd, p))                # the fold order is fixed
    np.testing.assert_array_equal(maps[..., 2], live.sum(0))
    np.testing.assert_array_equal(eng.pred_maps(), maps)
    return maps, lppd, p


# ---- 1. the accumulators through the C ABI ------------------------------------------------------

@pytest.mark.parametrize("name, post_nt", [("c1", 0), ("odd_depth", 0), ("d30", 0), ("tiny", 0), ("moffat", 0),
                                           ("deep", 0), ("odd_depth", 1), ("deep", 1)])
def test_accumulators_are_the_oracles_from_the_devices_residual(name, post_nt):
    """(post_nt 1: the non-temporal form of the accumulators' loads and stores)"""
    case = case_of(name)
    i0 = PO.base_ivar(case["data"], case["var"])
    live = i0 != 0.
    assert (~live).sum() == 2 and (i0 == 1e-12).sum() == 2
    acc = PO.Accum(i0.shape)
    with engine_of(case, {"post_nt": post_nt}) as eng:
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), i0)
        with pytest.raises(RuntimeError, match="posterior moments not begun"):
            eng.pred_begin()
        eng.post_begin()
        eng.pred_begin()
        assert eng.pred_count() == 0
        biggest = 0.
        for params in sequence(case):
            eng.set_params(params)
            eng.post_accumulate()
            err = eng.download_slot(_lib.SLOT_ERR)
            q = PO.q_of(err, i0)
            biggest = max(biggest, np.max(np.abs(q[live])))
            acc.add(q, live)
        n = eng.pred_count()
        assert n == eng.post_count() == acc.n == 6
        M, S, mean, m2 = eng.pred_get()
        np.testing.assert_array_equal(M, acc.M)
        np.testing.assert_array_equal(mean, acc.mean)
        np.testing.assert_array_equal(m2, acc.m2)
        # every term of S lies in (0, 1] and S >= 1: n exp calls of a few ulp each
        assert np.all(S[live] >= 1.) and np.all(S[live] <= n) and np.all(S[~live] == 0.)
        print(name, "max|q|", biggest, "S: max rel deviation", np.max(np.abs(S[live] / acc.S[live] - 1.)))
        np.testing.assert_allclose(S, acc.S, rtol=1e-13, atol=0.)
        maps, lppd, p = check_extraction(eng, n, i0)
        # a masked spaxel's voxels count: the model predicts them through its neighbours
        masked = case["mask"] == 0
        if masked.any():
            assert np.all(maps[..., 2][masked] > 0) and np.isfinite(maps[..., 0][masked]).all()
        # d3d_pred_end frees, the moments go on
        eng.pred_end()
        with pytest.raises(RuntimeError, match="not begun"):
            eng.pred_get()
        assert eng.pred_count() == 0 and eng.post_count() == 6


def test_far_samples_do_not_overflow_in_either_order():
    """Data scaled so that the far map's q lies thousands below the near ones': beyond exp's range."""
    case = case_of("d30")
    case["var"] = case["var"] * 1e-4
    i0 = PO.base_ivar(case["data"], case["var"])
    live = i0 != 0.
    acc = PO.Accum(i0.shape)
    with engine_of(case) as eng:
        eng.post_begin(0)
        eng.pred_begin()
        qs = []
        for params in sequence(case):
            eng.set_params(params)
            eng.post_accumulate()
            qs.append(PO.q_of(eng.download_slot(_lib.SLOT_ERR), i0))
            acc.add(qs[-1], live)
        jump = np.max(np.abs(qs[1] - qs[0])[live])
        print("largest jump of q between the first two samples", jump)
        assert jump > 745.
        M, S, mean, m2 = eng.pred_get()
        assert np.isfinite(S).all() and np.isfinite(M).all()
        np.testing.assert_array_equal(M, acc.M)
        np.testing.assert_allclose(S, acc.S, rtol=1e-13, atol=0.)
        lppd = eng.pred_cubes()[0]
        assert np.isfinite(lppd[live]).all()


# ---- 2. one sample ---------------------------------------------------------------------------------

def test_one_sample_is_the_chi2_map_and_the_states_log_density():
    case = case_of("c1")
    i0 = PO.base_ivar(case["data"], case["var"])
    live = i0 != 0.
    with engine_of(case) as eng:
        eng.post_begin()
        eng.pred_begin()
        eng.set_params(case["truth"])
        eng.post_accumulate()
        chi2 = eng.chi2_map()[0]                       # 1/2 sum_z r^2 / var
        err = eng.download_slot(_lib.SLOT_ERR)
        M, S, mean, m2 = eng.pred_get()
        np.testing.assert_array_equal(M, mean)
        np.testing.assert_array_equal(S, live.astype(np.float64))
        np.testing.assert_allclose(-2. * M.sum(0), 2. * chi2, rtol=1e-10, atol=0.)
        maps, lppd, p = check_extraction(eng, 1, i0)
        want = PO.log_density(err, i0)
        np.testing.assert_allclose(lppd[live], want[live], rtol=0., atol=np.max(lppd_margin(i0, M, 1)))
        assert np.isnan(p).all() and np.isnan(maps[..., 1]).all() and np.isnan(maps[..., 3]).all()
        assert np.isfinite(maps[..., 0]).all()


# ---- 3. the Student-t marginal ------------------------------------------------------------------------

@pytest.mark.parametrize("nu", [4, 1, 30])
def test_student_t_uses_the_base_variance_and_the_marginal(nu):
    case = case_of("odd_depth")
    i0 = PO.base_ivar(case["data"], case["var"])
    live = i0 != 0.
    acc = PO.Accum(i0.shape)
    with engine_of(case) as eng:
        eng.post_begin(0)
        eng.robust_begin(nu)
        eng.pred_begin()
        biggest = 0.
        for j, params in enumerate(sequence(case)):
            eng.set_params(params)
            eng.post_accumulate()
            q = PO.q_of(eng.download_slot(_lib.SLOT_ERR), i0, nu)
            biggest = max(biggest, np.max(np.abs(q[live])))
            acc.add(q, live)
            eng.robust_step(j + 1)                     # SLOT_IVAR = weight * base from now on
            ivar = eng.download_slot(_lib.SLOT_IVAR)
            assert np.mean(ivar[live] != i0[live]) > 0.99
        M, S, mean, m2 = eng.pred_get()
        for name, got, want, scale in (("M", M, acc.M, biggest), ("mean", mean, acc.mean, biggest),
                                       ("S", S, acc.S, 1.), ("M2", m2, acc.m2, biggest * biggest)):
            print("nu", nu, name, "max deviation / scale", np.max(np.abs(got - want)) / scale)
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * scale, err_msg=name)
        maps, lppd, p = check_extraction(eng, 6, i0, nu)
        want = PO.extract(6, acc.M, acc.S, acc.m2, i0, nu)
        np.testing.assert_allclose(lppd[live], want[0][live], rtol=1e-10, atol=1e-10 * biggest)
        np.testing.assert_allclose(p[live], want[1][live], rtol=1e-10, atol=1e-10 * biggest * biggest)
        # the Gaussian q of the same residuals is another number: the marginal formula is in force
        assert not np.allclose(M[live], PO.q_of(eng.download_slot(_lib.SLOT_ERR), i0)[live], rtol=1e-3)
        # the weights disarmed: the next sample would mix two likelihoods
        eng.robust_end()
        with pytest.raises(RuntimeError, match="share a likelihood"):
            eng.post_accumulate()


# ---- 4. through Run ----------------------------------------------------------------------------------

def run_of_case(case, **kw):
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(case["lsf"]), fsf=ImageFieldSpreadFunction(case["fsf"]))
    cube = d3d.MUSE().build_cube(case["data"])
    return d3d.Run(cube, inst, variance=case["var"], mask=case["mask"], initial_parameters=case["init"],
                   min_acceptance_rate=0., refresh_every=0, **kw)


def oracle_of_chain(samples, data, var, mask, fsf, lsf):
    """(accumulators, per-voxel bound on |dq|): the oracle over the residuals its forward model gives
    the chain's samples; a carried residual lies within RESIDUAL_BOUND max|data| of those, and
    |dq| <= |r| i0 dr."""
    i0 = PO.base_ivar(data, var)
    dr = RESIDUAL_BOUND * np.nanmax(np.abs(data))
    acc, dq = PO.Accum(i0.shape), np.zeros(i0.shape)
    for params in samples:
        err = PO.residual(data, params, mask, fsf, lsf)
        acc.add(PO.q_of(err, i0), i0 != 0.)
        dq = np.maximum(dq, np.abs(err) * i0 * dr)
    return acc, dq, i0


def assert_maps_within_the_propagated_bound(pa, acc, dq, i0, what):
    """lppd_v is a log-mean-exp of the q: it moves by at most max_s |dq|.  M2 = sum (q - mean)^2 moves
    by at most 4 eps_q sqrt(n M2) (Cauchy-Schwarz), so p_v by 4 eps_q sqrt(n p_v / (n - 1)).  Summed
    per spaxel; the test allows ten times the bound."""
    n = acc.n
    lppd, p = PO.extract(n, acc.M, acc.S, acc.m2, i0)
    maps = PO.fold_maps(lppd, p)
    live = i0 != 0.
    b_lppd = np.where(live, dq, 0.).sum(0)
    b_p = np.where(live, 4. * dq * np.sqrt(n * np.where(live, p, 0.) / (n - 1.)), 0.).sum(0)
    d_lppd, d_p = np.abs(pa.lppd_map - maps[..., 0]), np.abs(pa.p_waic_map - maps[..., 1])
    print(what, "lppd map: max deviation %.3g, bound %.3g (worst ratio %.3g); p map: %.3g, %.3g (%.3g)"
          % (d_lppd.max(), b_lppd.max(), np.max(d_lppd / b_lppd), d_p.max(), b_p.max(), np.max(d_p / b_p)))
    assert np.all(d_lppd <= 10. * b_lppd), what
    assert np.all(d_p <= 10. * b_p), what
    np.testing.assert_array_equal(pa.voxels, live.sum(0))


def test_run_accumulates_the_chains_samples_and_leaves_the_chain_alone(tmp_path):
    case = make_case("c1")
    kw = dict(seed=77, max_iterations=40, posterior_burn_in=20, keep_one_in=1)
    run = run_of_case(case, predictive=True, **kw)
    plain = run_of_case(case, **kw)
    np.testing.assert_array_equal(run.chain, plain.chain)
    np.testing.assert_array_equal(run.likelihoods, plain.likelihoods)
    np.testing.assert_array_equal(run.parameters, plain.parameters)
    np.testing.assert_array_equal(run.posterior.convolved_mean, plain.posterior.convolved_mean)
    assert plain.posterior.predictive is None
    pa = run.posterior.predictive
    assert isinstance(pa, d3d.PredictiveAccuracy) and pa.nu == 0
    assert pa.count == run.posterior.count == 20
    acc, dq, i0 = oracle_of_chain(run.chain[20:40], case["data"], case["var"], case["mask"], case["fsf"], case["lsf"])
    assert_maps_within_the_propagated_bound(pa, acc, dq, i0, "c1")
    assert pa.lppd_cube.shape == case["data"].shape
    np.testing.assert_array_equal(PO.fold_maps(pa.lppd_cube, pa.p_waic_cube)[..., :2],
                                  np.dstack((pa.lppd_map, pa.p_waic_map)))
    np.testing.assert_allclose(pa.elpd, np.sum(pa.lppd_cube - pa.p_waic_cube), rtol=1e-12)
    assert pa.waic == -2. * pa.elpd and pa.se > 0.
    pointwise = (pa.lppd_cube - pa.p_waic_cube).ravel()
    np.testing.assert_allclose(pa.se, np.sqrt(pointwise.size * pointwise.var(ddof=1)), rtol=1e-9)
    assert pa.compare(pa) == (0., 0.)
    run.posterior.save(str(tmp_path / "r"), clobber=True)
    saved = np.load(str(tmp_path / "r_posterior_predictive.npz"))
    assert int(saved["count"]) == 20
    np.testing.assert_array_equal(saved["elpd_map"], pa.elpd_map)


def test_three_chains_keep_their_own_and_pool_exactly():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, min_acceptance_rate=0., refresh_every=0, max_iterations=12, posterior_burn_in=4,
              predictive=dict())
    three = d3d.Run(cube, inst, seed=21, chains=3, **kw)
    singles = [d3d.Run(cube, inst, seed=21 + r, **kw) for r in range(3)]
    for r in range(3):
        np.testing.assert_array_equal(three.chains[r], singles[r].chain)
        mine, single = three.posteriors[r].predictive, singles[r].posterior.predictive
        assert mine.count == single.count == 8
        np.testing.assert_array_equal(mine.lppd_cube, single.lppd_cube)
        np.testing.assert_array_equal(mine.p_waic_cube, single.p_waic_cube)
        np.testing.assert_array_equal(mine.lppd_map, single.lppd_map)
        np.testing.assert_array_equal(mine.p_waic_map, single.p_waic_map)
    pooled = three.posterior.predictive
    assert pooled.count == three.posterior.count == 24
    # the pooled accumulators are the oracle's merge of the device's, extracted as the oracle does
    i0 = PO.base_ivar(cube.data, var)
    n, M, S, mean, m2 = PO.merge([pm.predictive.accumulators() for pm in three.posteriors])
    want = PO.extract(n, M, S, m2, i0)
    np.testing.assert_array_equal(pooled.lppd_cube, want[0])
    np.testing.assert_array_equal(pooled.p_waic_cube, want[1])
    np.testing.assert_array_equal(pooled.lppd_map, PO.fold_maps(*want)[..., 0])
    # ... and those of the oracle over all 24 samples
    samples = [three.chains[r][s] for r in range(3) for s in range(4, 12)]
    acc, dq, i0 = oracle_of_chain(samples, cube.data, var, three.mask, three.fsf, three.lsf)
    assert_maps_within_the_propagated_bound(pooled, acc, dq, i0, "three chains")


def test_tempering_follows_rung_0():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, seed=5, min_acceptance_rate=0., refresh_every=0, max_iterations=13, posterior_burn_in=4,
              tempering=dict(betas=(1., 0.8), swap_every=3))
    run = d3d.Run(cube, inst, predictive=True, **kw)
    plain = d3d.Run(cube, inst, **kw)
    for r in range(2):                   # (the other rung writes its pending updates back with rung 0)
        np.testing.assert_array_equal(run.chains[r], plain.chains[r])
    pa = run.posterior.predictive
    assert len(run.posteriors) == 1 and pa.count == run.posterior.count == 9
    acc, dq, i0 = oracle_of_chain(run.chains[0][4:13], cube.data, var, run.mask, run.fsf, run.lsf)
    assert_maps_within_the_propagated_bound(pa, acc, dq, i0, "rung 0")


def test_robust_run_scores_the_student_t_marginal():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, max_iterations=12, posterior_burn_in=4)
    run = d3d.Run(cube, inst, robust=4, predictive=True, **kw)
    plain = d3d.Run(cube, inst, robust=4, **kw)
    np.testing.assert_array_equal(run.chain, plain.chain)
    pa = run.posterior.predictive
    assert pa.nu == 4 and pa.count == 8
    i0 = PO.base_ivar(cube.data, var)
    acc = PO.Accum(i0.shape)
    for s in range(4, 12):
        acc.add(PO.q_of(PO.residual(cube.data, run.chain[s], run.mask, run.fsf, run.lsf), i0, 4))
    want = PO.extract(8, acc.M, acc.S, acc.m2, i0, 4)
    np.testing.assert_allclose(pa.lppd_cube, want[0], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(pa.p_waic_cube, want[1], rtol=1e-6, atol=1e-8)


def test_refusals():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    with pytest.raises(ValueError, match="predictive= needs posterior_burn_in="):
        d3d.Run(cube, inst, variance=var, max_iterations=4, predictive=True)

    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="predictive=: the line model Lorentzian"):
        d3d.Run(cube, inst, variance=var, model=Lorentzian, max_iterations=4, posterior_burn_in=2, predictive=True)
    case = case_of("d30")
    with engine_of(case) as eng:
        for call in (eng.pred_get, eng.pred_maps, eng.pred_cubes):
            with pytest.raises(RuntimeError, match="not begun"):
                call()
        with pytest.raises(RuntimeError, match="d3d_post_begin"):
            eng.pred_begin()
        eng.post_begin(0)
        eng.set_tile(0, 0, case["W"], 0, case["H"], 0, case["W"])
        with pytest.raises(NotImplementedError, match="predictive accuracy on a tile"):
            eng.pred_begin()


# ---- 5. what it is for: is it a doublet here? ---------------------------------------------------------

DOUBLET = ([0., 6.0], [1., 0.8])      # separation in channels, flux ratio
DOUBLET_A0 = 30.0                     # peak amplitude of the blob, in units of the noise
SCIENCE_SWEEPS, SCIENCE_BURN = 300, 150


def doublet_cube():
    """16 channels x 10 x 10, Gaussian FSF of FWHM 2 px (7 x 7): a blob (sigma 3.5 px) of doublets
    of one centre and width, unit noise."""
    D, H, W = 16, 10, 10
    rng = np.random.default_rng(4711)
    fsf = O.gaussian_fsf_image(2.0)
    lsf = O.gaussian_lsf_vector(D, 0.6)
    y, x = np.indices((H, W))
    r2 = (y - (H - 1) / 2.) ** 2 + (x - (W - 1) / 2.) ** 2
    truth = np.dstack((DOUBLET_A0 * np.exp(-r2 / (2. * 3.5 ** 2)), np.full((H, W), 6.0), np.full((H, W), 1.1)))
    keep = O.gaussian_line
    O.gaussian_line = multiplet(*DOUBLET)
    try:
        clean = O.forward_full((D, H, W), truth, np.ones((H, W)), fsf, lsf)
    finally:
        O.gaussian_line = keep
    data = clean + rng.normal(0., 1.0, clean.shape)
    return fsf, lsf, truth, data, np.ones(clean.shape)


def test_the_doublet_beats_the_single_gaussian_where_the_flux_is():
    """Both models from the truth's map, 300 sweeps, the samples of sweeps 150 .. 299.  On the oracle's
    chains (tests/predictive_oracle.py over oracle.mh_sweep, seed 5) the doublet beats the single
    Gaussian by delta elpd = 887.9 with se_delta = 81.9, 10.8 se (9.2 at amplitude 20 and 200 sweeps,
    8.1 at 14): the test asks for 4 se, half of the 8 the case was chosen for, to cover chain-to-chain
    scatter.  The single Gaussian's gain map peaks at 0.73 to 1.0 of the peak flux in all six
    calibration runs and its mean over the brighter half of the spaxels is 2.3 to 4.4 times that over
    the fainter half: asserted as above 0.5 and above 1 times."""
    fsf, lsf, truth, data, var = doublet_cube()
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    kw = dict(variance=var, initial_parameters=truth, seed=5, min_acceptance_rate=0., max_iterations=SCIENCE_SWEEPS,
              posterior_burn_in=SCIENCE_BURN, predictive=True)
    doublet = d3d.Run(cube, inst, model=d3d.GaussianMultipletLineModel(*DOUBLET), **kw)
    single = d3d.Run(cube, inst, **kw)
    a, b = doublet.posterior.predictive, single.posterior.predictive
    delta, se = a.compare(b)
    print("doublet against single: delta elpd %.4g, se %.4g, ratio %.3g; elpd %.6g / %.6g, p_waic %.4g / %.4g"
          % (delta, se, delta / se, a.elpd, b.elpd, a.p_waic, b.p_waic))
    assert delta > 4. * se
    np.testing.assert_allclose(delta, a.elpd - b.elpd, rtol=1e-9)
    gain = a.elpd_map - b.elpd_map
    flux = truth[..., 0]
    upper = flux > np.median(flux)
    y, x = np.unravel_index(np.argmax(gain), gain.shape)
    print("mean gain per spaxel: brighter half %.4g, fainter half %.4g; largest at (%d, %d), %.2f of the peak flux"
          % (gain[upper].mean(), gain[~upper].mean(), y, x, flux[y, x] / flux.max()))
    assert gain[upper].mean() > max(gain[~upper].mean(), 0.)
    assert flux[y, x] > 0.5 * flux.max()
