"""
Student-t likelihood on the device (csrc/d3d_robust.hip, Run(robust=...)): the weights
d3d_robust_step draws are tests/robust_oracle.py's at every shape and nu, whatever the options; an
armed run that never draws is the Gaussian run bit for bit and d3d_robust_end restores the base
cube; the draws have their Gamma distribution; the chain follows the oracle's chain update by
update; chains=R, resume and the other Run keywords work with it; and it does what it is for on a
cube with spiked voxels.
"""
import numpy as np
import pytest
from scipy import stats

import deconv3d_amd as d3d
from deconv3d_amd import _lib, regions, tiling
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import composed_oracle as CO
from tests import robust_oracle as RO
from tests.cases import make_case
from tests.test_gpu_run import synthetic_cube

pytestmark = pytest.mark.gpu

FSF5 = np.outer([0.1, 0.2, 0.4, 0.2, 0.1], [0.15, 0.2, 0.3, 0.2, 0.15])
NEVER = 10 ** 9           # a start no run reaches: armed, no draw


def shape_case(shape, seed=31):
    """A synthetic case of that shape with NaN voxels (one whole spectrum too) and zero variances."""
    D, H, W = shape
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, truth, init, min_b, max_b = O.synthetic_case(D, H, W, FSF5, lsf, seed=seed)
    data, var = data.copy(), var * (0.5 + np.random.default_rng(seed).random(var.shape)) ** 2
    data[D // 3, 1, 2] = np.nan
    data[:, H - 1, 0] = np.nan
    data[D - 1, 2, 1] = np.nan                      # (the last channel: beside the pad of an odd depth)
    var[0, 0, 0] = var[D // 2, 2, 3] = 0.0
    return dict(D=D, H=H, W=W, fsf=FSF5, lsf=lsf, data=data, var=var, mask=mask, init=init,
                min_b=min_b, max_b=max_b)


def engine_of(case, options=None, var="cube"):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    if var == "cube":
        eng.set_data(case["data"], case["var"], mask=case["mask"])
    else:
        eng.set_data(case["data"], None, var_scalar=var, mask=case["mask"])
    eng.set_params(case["init"])
    eng.mh_config(case["min_b"], case["max_b"], 0.1, 35.0, seed=77, refresh_every=0)
    return eng


# ---- 1. the draw against the oracle ------------------------------------------------------------

@pytest.mark.parametrize("shape", [(13, 5, 7), (32, 6, 5), (21, 30, 24), (300, 4, 4)])
def test_step_draws_the_oracles_weights(shape):
    """One real sweep (pending layers to write back), then the draw: SLOT_IVAR = lambda * i0 of the
    oracle from the same residual at rtol 1e-12 (IEEE-identical arithmetic around two or three libm
    calls of a few ulp), exactly 0 where the voxel carries nothing."""
    case = shape_case(shape)
    i0 = RO.base_ivar(case["data"], case["var"])
    assert (i0 == 0).sum() >= case["D"] + 2 and (i0 == 1e-12).sum() == 2
    with engine_of(case) as eng:
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), i0)
        eng.robust_begin(1, 1, NEVER, 0)
        eng.mh_sweeps(1, 1)
        for nu in (1, 2, 3, 4, 6, 8):          # (2 and 6: an even nu whose m = (nu + 1) // 2 is odd)
            eng.robust_begin(nu, 1, NEVER, 0)          # (afresh: the base cube back first)
            np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), i0)
            eng.robust_step(1)
            ivar = eng.download_slot(_lib.SLOT_IVAR)
            err = eng.download_slot(_lib.SLOT_ERR)
            lam = RO.draw_weights(77, 1, nu, err, i0)
            want = np.where(i0 == 0., 0., lam * i0)
            live = i0 != 0.
            print(shape, "nu", nu, "max rel", np.max(np.abs(ivar[live] / want[live] - 1.)))
            np.testing.assert_allclose(ivar, want, rtol=1e-12, atol=0., err_msg="nu %d" % nu)
            assert np.all(ivar[~live] == 0.)
            weights, mean, count = eng.robust_get()
            assert count == 1 and np.isnan(weights[~live]).all() and np.isnan(mean[~live]).all()
            np.testing.assert_allclose(weights[live], lam[live], rtol=1e-12)
            np.testing.assert_allclose(mean[live], lam[live], rtol=1e-12)   # one draw: the mean is it


# ---- 2. the same draw whatever the options -------------------------------------------------------

def test_draw_is_bit_identical_across_options():
    case = shape_case((16, 16, 9), seed=8)
    case["data"] = np.nan_to_num(case["data"])       # (a NaN voxel would rule the uniform variant out)
    v0 = float(np.median(case["var"]))

    def one(options, parts=False):
        with engine_of(case, options, var=v0) as eng:
            if parts:
                tiling.apply_parts(eng, tiling.TileLayout(case["H"], case["W"], 5, 5, 2, 1))
            uniform = eng.variance_is_uniform()
            eng.robust_begin(4, 1, NEVER, 0)
            assert not eng.variance_is_uniform()
            eng.mh_sweeps(1, 1)
            eng.robust_step(1)
            return dict(ivar=eng.download_slot(_lib.SLOT_IVAR), err=eng.download_slot(_lib.SLOT_ERR),
                        params=eng.get_params(), uniform=uniform)

    ref = one(None)
    assert ref["uniform"]
    for options in ({"mh_layers": 1}, {"mh_layers": 2}, {"uniform_ivar": 0}, {"uniform_ivar": 1}):
        got = one(options)
        assert got["uniform"] == (options.get("uniform_ivar", 1) == 1)
        for k in ("params", "err", "ivar"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (options, k))
    # a partitioned context scans in another order: its own residual, the oracle's weights from it,
    # and the bits of an unpartitioned context given that residual
    got = one(None, parts=True)
    i0 = np.full(got["err"].shape, 1. / v0)
    np.testing.assert_allclose(got["ivar"], RO.draw_weights(77, 1, 4, got["err"], i0) * i0, rtol=1e-12)
    with engine_of(case, {"mh_layers": 1}, var=v0) as eng:
        eng.robust_begin(4, 1, NEVER, 0)
        eng.upload_slot(_lib.SLOT_ERR, got["err"])
        eng.robust_step(1)
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), got["ivar"])


def test_default_variance_equals_the_same_constant_as_a_cube():
    inst, cube, _, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(seed=3, min_acceptance_rate=0., refresh_every=0, max_iterations=9, robust=4)
    a = d3d.Run(cube, inst, variance=None, **kw)
    b = d3d.Run(cube, inst, variance=a.variance_cube.copy(), **kw)
    np.testing.assert_array_equal(a.chain, b.chain)
    np.testing.assert_array_equal(a.robust.weight_mean, b.robust.weight_mean)
    assert a.robust.count == b.robust.count == 8


# ---- 3. armed without a draw: the Gaussian chain --------------------------------------------------

@pytest.mark.parametrize("uniform", [True, False])
def test_a_start_never_reached_leaves_the_chain_and_end_restores_the_slot(uniform):
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    if not uniform:
        var = var * (0.5 + np.random.default_rng(1).random(var.shape))
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, max_iterations=12)
    plain = d3d.Run(cube, inst, **kw)
    armed = d3d.Run(cube, inst, robust=dict(nu=4, start=NEVER), **kw)
    np.testing.assert_array_equal(armed.chain, plain.chain)
    np.testing.assert_array_equal(armed.likelihoods, plain.likelihoods)
    assert armed.robust.count == 0 and np.isnan(armed.robust.weight_mean).all()
    np.testing.assert_array_equal(armed.robust.weights, np.ones(var.shape))
    assert plain.robust is None and plain.engine.variance_is_uniform() == uniform
    assert not armed.engine.variance_is_uniform()
    armed.engine.robust_step(5)
    assert not np.array_equal(armed.engine.download_slot(_lib.SLOT_IVAR), 1. / var)
    armed.engine.robust_end()
    np.testing.assert_array_equal(armed.engine.download_slot(_lib.SLOT_IVAR), 1. / var)
    assert armed.engine.variance_is_uniform() == uniform
    with pytest.raises(RuntimeError, match="not begun"):
        armed.engine.robust_get()


# ---- 4. the distribution of the device's draws -----------------------------------------------------

@pytest.mark.parametrize("nu", [3, 4])
def test_device_draws_are_gamma(nu):
    """Data equal to the model: r is 0 to rounding, lambda nu / 2 ~ Gamma((nu + 1) / 2)."""
    D, H, W = 32, 25, 25
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    _, var, mask, truth, _, min_b, max_b = O.synthetic_case(D, H, W, FSF5, lsf, seed=2)
    mask = np.ones((H, W))
    with _lib.Engine((D, H, W), FSF5.shape) as eng:
        eng.set_taps(FSF5, lsf)
        eng.set_params(truth)
        eng.set_data(eng.forward(), var, mask=mask)
        eng.mh_config(min_b, max_b, 0.1, 35.0, seed=123, refresh_every=0)
        assert np.max(np.abs(eng.residual()) / np.sqrt(var)) < 1e-9
        eng.robust_begin(nu)
        eng.robust_step(1)
        lam = eng.robust_get()[0]
    ks = stats.kstest(lam.ravel() * nu / 2., stats.gamma((nu + 1) / 2.).cdf)
    print("nu", nu, ks)
    assert ks.pvalue > 1e-3, ks


# ---- 5. the chain against the oracle's ---------------------------------------------------------------

def run_of_case(case, **kw):
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(case["lsf"]), fsf=ImageFieldSpreadFunction(case["fsf"]))
    cube = d3d.MUSE().build_cube(case["data"])
    return d3d.Run(cube, inst, variance=case["var"], mask=case["mask"], initial_parameters=case["init"],
                   min_acceptance_rate=0., refresh_every=0, **kw)


def test_chain_follows_the_oracles_update_by_update():
    """Five sweeps with every = 1 on c1: parameters after every sweep, the carried residual and the
    accepted count as tests/test_gpu_parity.py and tests/test_gpu_chain.py compare a device chain
    with the oracle's; the weight mean and its count at rtol 1e-12."""
    case = make_case("c1")
    run = run_of_case(case, seed=77, max_iterations=6, robust=dict(nu=4, every=1))
    st = O.MHState(case["data"], case["var"], case["mask"], case["fsf"], case["lsf"], case["init"],
                   run.min_boundaries, run.max_boundaries, 0.1, run.gibbs_apriori_variance, 77)
    chain = RO.RobustChain(st, 4)
    live = case["mask"] == 1
    for s in range(1, 6):
        chain.sweep(s)
        np.testing.assert_allclose(run.chain[s][live], st.params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="params after sweep %d" % s)
    assert run._acceptance.accepted_count == int(live.sum()) + st.accepted
    err = run.engine.download_slot(_lib.SLOT_ERR)
    assert np.max(np.abs(err - st.err)) <= 1e-11 * np.max(np.abs(st.err))
    assert run.robust.count == chain.count == 5
    want = chain.weight_mean()
    print("weight mean: max rel", np.nanmax(np.abs(run.robust.weight_mean / want - 1.)))
    np.testing.assert_allclose(run.robust.weight_mean, want, rtol=1e-12)


# ---- 6. chains=R ---------------------------------------------------------------------------------------

def test_two_chains_are_the_single_runs_bit_for_bit():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, min_acceptance_rate=0., refresh_every=0, max_iterations=8,
              robust=dict(nu=3, every=2, start=1), posterior_burn_in=3)
    both = d3d.Run(cube, inst, seed=21, chains=2, **kw)
    singles = [d3d.Run(cube, inst, seed=21 + r, **kw) for r in range(2)]
    for r in range(2):
        np.testing.assert_array_equal(both.chains[r], singles[r].chain)
        np.testing.assert_array_equal(both.robusts[r].weight_mean, singles[r].robust.weight_mean)
        assert both.robusts[r].count == singles[r].robust.count == 3          # sweeps 3, 5, 7
    assert both.robust.count == 6
    np.testing.assert_allclose(both.robust.weight_mean,
                               0.5 * (singles[0].robust.weight_mean + singles[1].robust.weight_mean), rtol=1e-14)


# ---- 7. resume --------------------------------------------------------------------------------------------

def test_resume_remakes_the_last_draw_and_refuses_another_nu(tmp_path):
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    name = str(tmp_path / "ck")
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, robust=4)
    whole = d3d.Run(cube, inst, max_iterations=13, **kw)
    d3d.Run(cube, inst, max_iterations=7, write_every=7, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    np.testing.assert_array_equal(state["robust_keywords"], [4, 1, 0])
    resume = dict(initial_parameters=name + "_parameters.npy", resume_state=name + "_state.npz")
    second = d3d.Run(cube, inst, max_iterations=7, **dict(kw, **resume))
    # (the resumed run rebuilds the residual from the parameters: rounding-level differences)
    np.testing.assert_allclose(second.chain[-1], whole.chain[-1], rtol=1e-8, atol=1e-8)
    assert second.robust.count == 6                                            # its own sweeps 7 .. 12
    gaussian = d3d.Run(cube, inst, max_iterations=13, **dict(kw, robust=None))
    assert not np.allclose(gaussian.chain[-1], whole.chain[-1], rtol=1e-3, atol=1e-3)
    for other in (3, dict(nu=4, every=2), None):
        with pytest.raises(ValueError, match="resume_state was written with robust="):
            d3d.Run(cube, inst, max_iterations=7, **dict(kw, robust=other, **resume))


# ---- 8. what it is for: spiked voxels ------------------------------------------------------------------------

SPIKE_SHARE = 0.03        # of the voxels; DESIGN.md section 8l: the oracle's margins at 1, 2 and 3 %


def test_spiked_voxels_are_downweighted_and_the_flux_map_improves():
    """synthetic_cube(32, 12, 12) with +50 sigma on SPIKE_SHARE of the voxels, never two in one
    spectrum; nu = 4, 400 sweeps from the truth, moments from sweep 100.  E[lambda | r] =
    (nu + 1) / (nu + r^2 / sigma^2) is 0.002 at 50 sigma and the prior mean is 1: the mean weight is
    below 0.1 at every spiked voxel and its median over the others above 0.5.  Against the Gaussian
    run the rms errors of the posterior-mean c map and flux map over the spaxels whose window holds a
    spike are smaller (the direction only).  On the oracle's chains the
    Gaussian run's rms is 2.07 times the robust run's for the flux map at this share (1.55 at 1 %,
    1.58 at 2 %) and 1.48 times for the c map (1.40, 1.35; 1.50 at one spike in every spectrum, the
    most the case allows): the c map's margin is 1.48, not the factor 2 the share was raised for, its
    rms being that of the faint outer spaxels whose centre neither likelihood identifies."""
    D, H, W = 32, 12, 12
    inst, cube, var, truth, sigma = synthetic_cube(D=D, H=H, W=W)
    rng = np.random.default_rng(12346)
    n = int(round(SPIKE_SHARE * D * H * W))
    sp = rng.choice(H * W, size=n, replace=False)              # never two in one spectrum
    spikes = np.zeros((D, H, W), dtype=bool)
    spikes[rng.integers(0, D, size=n), sp // W, sp % W] = True
    assert spikes.sum() == n and spikes.sum(0).max() == 1
    spiked = inst.build_cube(cube.data + 50. * sigma * spikes)
    fh, fw = (s // 2 for s in inst.fsf.as_image(cube).shape)
    near = np.zeros((H, W), dtype=bool)
    for y, x in zip(*np.nonzero(spikes.any(0))):
        near[max(y - fh, 0):y + fh + 1, max(x - fw, 0):x + fw + 1] = True
    kw = dict(variance=var, initial_parameters=truth, seed=7, min_acceptance_rate=0., max_iterations=400,
              posterior_burn_in=100)
    robust = d3d.Run(spiked, inst, robust=4, **kw)
    gauss = d3d.Run(spiked, inst, **kw)
    mean = robust.robust.weight_mean
    assert robust.robust.count == 300
    print("weight mean: max at the spikes", mean[spikes].max(), "median elsewhere", np.median(mean[~spikes]))
    assert np.all(mean[spikes] < 0.1)
    assert np.median(mean[~spikes]) > 0.5
    assert robust.robust.downweighted()[spikes].all()
    flux = truth[..., 0] * truth[..., 2] * np.sqrt(2. * np.pi)

    def rms(run):
        return (np.sqrt(np.mean((run.posterior.parameters_mean[..., 1] - truth[..., 1])[near] ** 2)),
                np.sqrt(np.mean((run.posterior.flux_mean - flux)[near] ** 2)))

    (c_r, f_r), (c_g, f_g) = rms(robust), rms(gauss)
    print("rms c: gaussian %.4g robust %.4g ratio %.3g; rms F: gaussian %.4g robust %.4g ratio %.3g"
          % (c_g, c_r, c_g / c_r, f_g, f_r, f_g / f_r))
    assert f_r < f_g
    assert c_r < c_g


# ---- 9. with the other keywords ----------------------------------------------------------------------------------

def test_runs_with_adaptation_prior_histograms_and_regions():
    """The keywords together, one sweep per device call and 64: every output bit for bit the same; the
    first six sweeps (draws after 2, 4 and 6, the prior on) are tests/composed_oracle.py's at 1e-9."""
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., max_iterations=60, refresh_every=25,
              robust=dict(nu=5, every=2), adapt_sweeps=20, adapt_window=10, smoothness=dict(c=1.),
              posterior_burn_in=20, posterior_histograms=dict(pilot=10, span=6.),
              regions=regions.blocks((9, 9), 3))
    run = d3d.Run(cube, inst, sweeps_per_call=64, **kw)
    assert np.isfinite(run.chain).all() and np.isfinite(run.parameters).all()
    assert run.robust.count == 20 and np.isfinite(run.robust.weight_mean).all()       # sweeps 20, 22 .. 58
    assert np.all(run.robust.weight_mean > 0.) and np.isfinite(run.robust.weights).all()
    assert run.posterior.count == 40 and np.isfinite(run.posterior.convolved_mean).all()
    assert np.isfinite(run.posterior.histograms.median).all()
    assert np.isfinite(run.posterior.regions.flux).all()
    assert np.isfinite(run.jump_scale).all() and run.adapted_until == 20
    one = d3d.Run(cube, inst, sweeps_per_call=1, **kw)
    a, b = CO.run_outputs(run), CO.run_outputs(one)
    assert sorted(a) == sorted(b) and "robust_weight_mean" in a
    for k in sorted(a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    ft = CO.features_of(lam=(0., 1., 0.), robust=dict(nu=5, every=2, start=0, accumulate_from=20),
                        adapt=dict(target=0.25, window=10, last=20, gain=2.0, range=(1e-3, 1e3)))
    want, co = CO.chain_of_run(run, cube.data, var, inst.fsf.as_image(cube), inst.lsf.as_vector(cube), ft, 6)
    assert co.rescale_due(6) and not co.rescale_due(5) and not np.array_equal(co.ivar, co.pb["i0"])
    np.testing.assert_allclose(run.chain[:7], want, rtol=1e-9, atol=1e-9)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------

def test_refusals():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    with pytest.raises(ValueError, match="robust= with tempering="):
        d3d.Run(cube, inst, variance=var, max_iterations=4, robust=4, tempering=dict(rungs=2, beta_min=0.5))

    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="robust=: the line model Lorentzian"):
        d3d.Run(cube, inst, variance=var, model=Lorentzian, max_iterations=4, robust=4)
    case = shape_case((13, 5, 7))
    with engine_of(case) as eng:
        for bad in (dict(nu=0), dict(nu=31), dict(nu=4, every=0), dict(nu=4, start=-1)):
            with pytest.raises(ValueError):
                eng.robust_begin(**bad)
        with pytest.raises(RuntimeError, match="not begun"):
            eng.robust_step(1)
        eng.robust_begin(4)
        with pytest.raises(NotImplementedError, match="robust weights are armed"):
            eng.set_tile(0, 0, 7, 0, 5, 0, 7)
        with pytest.raises(RuntimeError, match="d3d_robust_end first"):
            eng.set_data(case["data"], case["var"], mask=case["mask"])
        with pytest.raises(RuntimeError, match="d3d_robust_end first"):
            eng.upload_slot(_lib.SLOT_IVAR, case["var"])
        eng.robust_end()
        eng.set_tile(0, 0, 7, 0, 5, 0, 7)
        with pytest.raises(NotImplementedError, match="on a tile"):
            eng.robust_begin(4)
    with _lib.Engine((13, 5, 7), (5, 5)) as eng:
        with pytest.raises(RuntimeError, match="data not set"):
            eng.robust_begin(4)
    # chains that share a launch write their pending updates back together: armed alike, or refused
    with engine_of(case) as a, engine_of(case) as b:
        a.robust_begin(4)
        with pytest.raises(ValueError, match="robust weights"):
            _lib.mh_sweeps_batch([a, b], 1, 1)
        b.robust_begin(4, every=2)
        with pytest.raises(ValueError, match="robust weights"):
            _lib.mh_sweeps_batch([a, b], 1, 1)
        b.robust_begin(3)
        _lib.mh_sweeps_batch([a, b], 2, 1)
        assert a.robust_get(False, False)[2] == b.robust_get(False, False)[2] == 2
