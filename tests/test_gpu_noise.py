"""
Noise-scale inference on the device (csrc/d3d_noise.hip, Run(noise=...)): the sums d3d_noise_step
folds are tests/noise_oracle.py's bit for bit and its draw the oracle's at every shape and grouping,
whatever the options; an armed run that never draws is the run without the keyword bit for bit and
d3d_noise_end restores the base cube; begin / end return their device memory; the draws have their
Gamma distribution; the chain follows the oracle's chain; chains=R, resume and the other Run
keywords work with it; every refusal; and it does what it is for on a cube whose noise is not the
one it was told.
"""
import gc
import os

import numpy as np
import pytest
from scipy import stats

import deconv3d_amd as d3d
from deconv3d_amd import _lib, regions, tiling
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import composed_oracle as CO
from tests import noise_oracle as NO
from tests.cases import make_case
from tests.test_gpu_run import synthetic_cube

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9           # a start no run reaches: armed, no draw
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_recovery.npz")


def engine_of(case, options=None, var="cube", seed=NO.STEP_SEED):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    if var == "cube":
        eng.set_data(case["data"], case["var"], mask=case["mask"])
    else:
        eng.set_data(case["data"], None, var_scalar=var, mask=case["mask"])
    eng.set_params(case["init"])
    eng.mh_config(case["min_b"], case["max_b"], 0.1, 35.0, seed=seed, refresh_every=0)
    return eng


def begin(eng, group, G, spaxels=None, **kw):
    eng.noise_begin(group, G, spaxels, **dict(dict(start=NEVER, capacity=4), **kw))


# ---- 1. the draw against the oracle ------------------------------------------------------------

@pytest.mark.parametrize("shape", NO.STEP_SHAPES)
def test_step_draws_the_oracles_scales(shape):
    """One real sweep (pending layers to write back), then the draw from the device's own downloaded
    residual, for every grouping with and without a map of spaxels with holes: N_g equal, Q_g bit for
    bit, tau and the rewritten SLOT_IVAR at rtol 1e-12 (IEEE-identical arithmetic around a log, a cos
    and a sqrt of a few ulp), exactly 0 where the voxel carries nothing, channels that are not
    rescaled bit-equal to the base."""
    case = NO.shape_case(shape)
    D, H, W = shape
    i0 = NO.base_ivar(case["data"], case["var"])
    assert (i0 == 0).sum() >= D + 2 and (i0 == 1e-12).sum() == 2
    worst = 0.
    with engine_of(case) as eng:
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), i0)
        begin(eng, *NO.grouping("cube", D))
        eng.mh_sweeps(1, 1)
        for sp in (None, NO.holes(H, W)):
            for name in NO.GROUPINGS:
                group, G = NO.grouping(name, D)
                begin(eng, group, G, sp)                      # (afresh: the base cube back first)
                np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), i0)
                eng.noise_step(NO.STEP_SWEEP)
                ivar, err = eng.download_slot(_lib.SLOT_IVAR), eng.download_slot(_lib.SLOT_ERR)
                want = NO.draw_scales(NO.STEP_SEED, NO.STEP_SWEEP, err, i0, group, sp, G=G)
                scale, sweeps, voxels, sums, tau = eng.noise_get()
                what = "%s %s holes=%s" % (shape, name, sp is not None)
                np.testing.assert_array_equal(voxels, want["voxels"], err_msg=what)
                np.testing.assert_array_equal(sums, want["sums"], err_msg=what)
                assert list(sweeps) == [NO.STEP_SWEEP] and scale.shape == (1, G)
                live = want["voxels"] >= 2
                assert np.isnan(scale[0][~live]).all() and (name != "three" or not live[1])
                rel = np.max(np.abs(tau / want["tau"] - 1.))
                worst = max(worst, rel)
                np.testing.assert_allclose(tau, want["tau"], rtol=1e-12, atol=0., err_msg=what)
                np.testing.assert_allclose(scale[0][live], want["scale"][live], rtol=1e-12, atol=0.)
                np.testing.assert_allclose(ivar, np.where(i0 == 0., 0., i0 * want["tau"][:, None, None]),
                                           rtol=1e-12, atol=0., err_msg=what)
                assert np.all(ivar[i0 == 0.] == 0.)
                still = (group < 0) | ~live[np.maximum(group, 0)]
                np.testing.assert_array_equal(ivar[still], i0[still], err_msg=what)
                np.testing.assert_array_equal(tau[still], 1.)
    print(shape, "tau: max rel", worst)


# ---- 2. the same draw whatever the options -------------------------------------------------------

def test_draw_is_bit_identical_across_options():
    case = NO.shape_case((16, 16, 9), seed=8)
    case["data"] = np.nan_to_num(case["data"])       # (a NaN voxel would rule the uniform variant out)
    v0 = float(np.median(case["var"]))
    group, G = NO.grouping("channel", 16)

    def one(options, parts=False):
        with engine_of(case, options, var=v0) as eng:
            if parts:
                tiling.apply_parts(eng, tiling.TileLayout(case["H"], case["W"], 5, 5, 2, 1))
            uniform = eng.variance_is_uniform()
            begin(eng, group, G)
            assert not eng.variance_is_uniform()
            eng.mh_sweeps(1, 1)
            eng.noise_step(1)
            return dict(ivar=eng.download_slot(_lib.SLOT_IVAR), err=eng.download_slot(_lib.SLOT_ERR),
                        params=eng.get_params(), uniform=uniform, got=eng.noise_get())

    ref = one(None)
    assert ref["uniform"]
    for options in ({"mh_layers": 1}, {"mh_layers": 2}, {"uniform_ivar": 0}, {"uniform_ivar": 1}):
        got = one(options)
        assert got["uniform"] == (options.get("uniform_ivar", 1) == 1)
        for k in ("params", "err", "ivar"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (options, k))
        for a, b in zip(got["got"], ref["got"]):
            np.testing.assert_array_equal(a, b)
    # a partitioned context scans in another order: its own residual, the oracle's scales from it,
    # and the bits of an unpartitioned context given that residual
    got = one(None, parts=True)
    i0 = np.full(got["err"].shape, 1. / v0)
    want = NO.draw_scales(NO.STEP_SEED, 1, got["err"], i0, group, G=G)
    np.testing.assert_array_equal(got["got"][3], want["sums"])
    np.testing.assert_allclose(got["ivar"], i0 * want["tau"][:, None, None], rtol=1e-12)
    with engine_of(case, {"mh_layers": 1}, var=v0) as eng:
        begin(eng, group, G)
        eng.upload_slot(_lib.SLOT_ERR, got["err"])
        eng.noise_step(1)
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), got["ivar"])


def test_a_timed_step_is_the_same_draw():
    """Option noise_timing: HIP events between the three launches of d3d_noise_step, nothing else."""
    case = NO.shape_case((21, 30, 24))
    group, G = NO.grouping("channel", 21)
    got = []
    for timing in (0, 1):
        with engine_of(case, {"noise_timing": timing}) as eng:
            begin(eng, group, G)
            eng.mh_sweeps(1, 1)
            eng.noise_step(1)
            got.append((eng.download_slot(_lib.SLOT_IVAR),) + eng.noise_get())
            ns = [eng.get_option("noise_%s_ns" % k) for k in ("sums", "draw", "apply")]
            assert all(v > 0 for v in ns) if timing else ns == [0, 0, 0]
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


def test_default_variance_equals_the_same_constant_as_a_cube():
    inst, cube, _, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(seed=3, min_acceptance_rate=0., refresh_every=0, max_iterations=9, noise=True)
    a = d3d.Run(cube, inst, variance=None, **kw)
    b = d3d.Run(cube, inst, variance=a.variance_cube.copy(), **kw)
    np.testing.assert_array_equal(a.chain, b.chain)
    np.testing.assert_array_equal(a.noise.scale, b.noise.scale)
    assert a.noise.count == b.noise.count == 8 and a.noise.scale.shape == (8, 16)


# ---- 3. armed without a draw: the run without the keyword -----------------------------------------

@pytest.mark.parametrize("uniform", [True, False])
def test_a_start_never_reached_leaves_the_chain_and_end_restores_the_slot(uniform):
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    if not uniform:
        var = var * (0.5 + np.random.default_rng(1).random(var.shape))
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, max_iterations=12)
    plain = d3d.Run(cube, inst, **kw)
    armed = d3d.Run(cube, inst, noise=dict(start=NEVER), **kw)
    np.testing.assert_array_equal(armed.chain, plain.chain)
    np.testing.assert_array_equal(armed.likelihoods, plain.likelihoods)
    np.testing.assert_array_equal(armed.engine.download_slot(_lib.SLOT_ERR), plain.engine.download_slot(_lib.SLOT_ERR))
    assert armed.noise.count == 0 and armed.noise.scale.shape == (0, 16) and np.isnan(armed.noise.channel_scale).all()
    assert plain.noise is None and plain.engine.variance_is_uniform() == uniform
    assert not armed.engine.variance_is_uniform()
    armed.engine.noise_step(5)
    assert not np.array_equal(armed.engine.download_slot(_lib.SLOT_IVAR), 1. / var)
    with pytest.raises(RuntimeError, match="series of noise scales is full"):
        armed.engine.noise_step(6)                     # (a start never reached: a capacity of one row)
    armed.engine.noise_end()
    np.testing.assert_array_equal(armed.engine.download_slot(_lib.SLOT_IVAR), 1. / var)
    assert armed.engine.variance_is_uniform() == uniform
    with pytest.raises(RuntimeError, match="not begun"):
        armed.engine.noise_get()


# ---- 4. ownership ---------------------------------------------------------------------------------------

def test_begin_end_and_close_return_the_device_memory():
    case = NO.shape_case((13, 5, 7))
    group, G = NO.grouping("three", 13)
    gc.collect()                                      # (engines of earlier tests' runs)
    with engine_of(case) as eng:
        fresh = eng.get_option("device_bytes")
        eng.mh_sweeps(1, 1)
        before = eng.get_option("device_bytes")
        begin(eng, group, G, NO.holes(5, 7), capacity=100)
        armed = eng.get_option("device_bytes")
        Dp = 14
        assert armed - before >= 5 * 7 * Dp * 8 + NO.STREAMS * Dp * 12 + 100 * G * 8
        begin(eng, group, G, NO.holes(5, 7), capacity=100)
        assert eng.get_option("device_bytes") == armed             # a second begin takes no more
        eng.noise_step(1)
        eng.noise_end()
        assert eng.get_option("device_bytes") == before
        begin(eng, group, G, NO.holes(5, 7), capacity=100)
        assert eng.get_option("device_bytes") == armed
    # (the armed engine closed without an end: everything back)
    with engine_of(case) as eng:
        assert eng.get_option("device_bytes") == fresh


# ---- 5. the distribution of the device's draws -----------------------------------------------------

def test_device_draws_are_gamma():
    """2000 sweep numbers at one residual on (32, 6, 5), a scale per channel: tau_z (b0 + Q_z / 2) ~
    Gamma(a0 + N_z / 2), whatever the channel's N_z, through its own CDF."""
    case = NO.shape_case((32, 6, 5))
    group, G = NO.grouping("channel", 32)
    n = 2000
    with engine_of(case) as eng:
        begin(eng, group, G, shape=1.5, rate=0.25, capacity=n)
        eng.mh_sweeps(1, 1)
        for s in range(n):
            eng.noise_step(s)
        scale, sweeps, voxels, sums, _ = eng.noise_get()
    assert scale.shape == (n, 32) and list(sweeps) == list(range(n)) and voxels.min() >= 2
    u = stats.gamma(1.5 + 0.5 * voxels).cdf((1. / scale) * (0.25 + 0.5 * sums))
    ks = stats.kstest(u.ravel(), "uniform")
    print(ks)
    assert ks.pvalue > 1e-3, ks


# ---- 6. the chain against the oracle's ---------------------------------------------------------------

def run_of_case(case, **kw):
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(case["lsf"]), fsf=ImageFieldSpreadFunction(case["fsf"]))
    cube = d3d.MUSE().build_cube(case["data"])
    return d3d.Run(cube, inst, variance=case["var"], mask=case["mask"], initial_parameters=case["init"],
                   min_acceptance_rate=0., refresh_every=0, **kw)


def test_chain_follows_the_oracles_update_by_update():
    """Five sweeps with every = 1 on c1: parameters after every sweep, the carried residual and the
    accepted count as tests/test_gpu_robust.py compares them; the series of scales at rtol 1e-12."""
    case = make_case("c1")
    run = run_of_case(case, seed=77, max_iterations=6, noise=True)
    st = O.MHState(case["data"], case["var"], case["mask"], case["fsf"], case["lsf"], case["init"],
                   run.min_boundaries, run.max_boundaries, 0.1, run.gibbs_apriori_variance, 77)
    chain = NO.NoiseChain(st, NO.group_of("channel", case["data"].shape[0]))
    live = case["mask"] == 1
    for s in range(1, 6):
        chain.sweep(s)
        np.testing.assert_allclose(run.chain[s][live], st.params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="params after sweep %d" % s)
    assert run._acceptance.accepted_count == int(live.sum()) + st.accepted
    err = run.engine.download_slot(_lib.SLOT_ERR)
    assert np.max(np.abs(err - st.err)) <= 1e-11 * np.max(np.abs(st.err))
    assert run.noise.count == 5 and list(run.noise.sweeps) == chain.sweeps
    print("scales: max rel", np.max(np.abs(run.noise.scale / chain.scale() - 1.)))
    np.testing.assert_allclose(run.noise.scale, chain.scale(), rtol=1e-12)
    np.testing.assert_array_equal(run.noise.groups, np.arange(32))
    np.testing.assert_array_equal(run.noise.voxels, (NO.base_ivar(case["data"], case["var"]) != 0).sum(axis=(1, 2)))


# ---- 7. chains=R ---------------------------------------------------------------------------------------

def test_two_chains_are_the_single_runs_bit_for_bit():
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, min_acceptance_rate=0., refresh_every=0, max_iterations=8,
              noise=dict(per="cube", every=2, start=1), posterior_burn_in=3)
    both = d3d.Run(cube, inst, seed=21, chains=2, **kw)
    singles = [d3d.Run(cube, inst, seed=21 + r, **kw) for r in range(2)]
    for r in range(2):
        np.testing.assert_array_equal(both.chains[r], singles[r].chain)
        np.testing.assert_array_equal(both.noises[r].scale, singles[r].noise.scale)
        assert list(both.noises[r].sweeps) == [1, 3, 5, 7] and both.noises[r].scale.shape == (4, 1)
    assert both.noise.count == 8
    np.testing.assert_array_equal(both.noise.scale, np.concatenate([s.noise.scale for s in singles]))
    # (the mean takes the draws from posterior_burn_in on: sweeps 3, 5, 7 of either chain)
    np.testing.assert_allclose(both.noise.scale_mean, np.mean([s.noise.scale[1:] for s in singles]), rtol=1e-14)


def test_resume_remakes_the_last_draw_and_refuses_other_keywords(tmp_path):
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    name = str(tmp_path / "ck")
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, noise=True)
    whole = d3d.Run(cube, inst, max_iterations=13, **kw)
    d3d.Run(cube, inst, max_iterations=7, write_every=7, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    np.testing.assert_array_equal(state["noise_keywords"], [1, 0, 0, 0, 16])
    np.testing.assert_array_equal(state["noise_group"], np.arange(16))
    resume = dict(initial_parameters=name + "_parameters.npy", resume_state=name + "_state.npz")
    second = d3d.Run(cube, inst, max_iterations=7, **dict(kw, **resume))
    # (the resumed run rebuilds the residual from the parameters: rounding-level differences)
    np.testing.assert_allclose(second.chain[-1], whole.chain[-1], rtol=1e-8, atol=1e-8)
    assert list(second.noise.sweeps) == list(range(7, 13))                     # its own sweeps 7 .. 12
    np.testing.assert_allclose(second.noise.scale, whole.noise.scale[6:], rtol=1e-8)
    fixed = d3d.Run(cube, inst, max_iterations=13, **dict(kw, noise=None))
    assert not np.allclose(fixed.chain[-1], whole.chain[-1], rtol=1e-3, atol=1e-3)
    for other in (dict(per="cube"), dict(every=2), None):
        with pytest.raises(ValueError, match="resume_state was written with"):
            d3d.Run(cube, inst, max_iterations=7, **dict(kw, noise=other, **resume))


# ---- 8. what it is for: a variance that is not the one given ---------------------------------------------

def test_inflated_channels_are_recovered():
    """synthetic_cube(32, 12, 12) from the truth, the true noise variance RECOVERY_FACTOR = 4 times the
    given one on a fixed third of the channels (z % 3 == 1); noise=True, 400 iterations, means from sweep
    100.  The cube is the fixture's, which tests/noise_oracle.py: make_recovery_fixture builds with the
    oracle's forward model (the device's cube is checked to be the same to rounding), so that the
    fixture's means of the oracle's chain belong to the very data the device runs on.  On the oracle's
    chain the mean scales of the inflated channels span 3.339275 .. 4.742394 and those of the others
    0.812206 .. 1.229627; one posterior standard deviation of a single channel's
    scale, sqrt(2 / N_z) = sqrt(2 / 144) = 0.117851, widens either band.  The device's means are the
    oracle's to 1e-9.  Printed, not asserted: the ratio of posterior.parameters_std to the
    fixed-variance run's at the brightest spaxels."""
    D, H, W = 32, 12, 12
    inst, cube, var, truth, sigma = synthetic_cube(D=D, H=H, W=W)
    golden = np.load(GOLDEN)
    np.testing.assert_allclose(NO.recovery_data(cube.data, sigma), golden["data"], rtol=1e-11, atol=1e-11)
    cube = inst.build_cube(golden["data"])
    kw = dict(variance=var, initial_parameters=truth, seed=NO.RECOVERY_SEED, min_acceptance_rate=0.,
              max_iterations=NO.RECOVERY_ITERATIONS, posterior_burn_in=NO.RECOVERY_BURN_IN)
    run = d3d.Run(cube, inst, noise=True, **kw)
    fixed = d3d.Run(cube, inst, **kw)
    infl = NO.recovery_inflated(D)
    mean = run.noise.channel_scale
    assert run.noise.count == 399 and (run.noise.sweeps >= NO.RECOVERY_BURN_IN).sum() == 300
    np.testing.assert_array_equal(mean, run.noise.scale_mean)
    sd = np.sqrt(2. / (H * W))
    print("mean scale: inflated %.6f .. %.6f, others %.6f .. %.6f; max |device / oracle - 1| = %.3g"
          % (mean[infl].min(), mean[infl].max(), mean[~infl].min(), mean[~infl].max(),
             np.max(np.abs(mean / golden["oracle_scale_mean"] - 1.))))
    assert np.all((mean[infl] > 3.339275 - sd) & (mean[infl] < 4.742394 + sd))
    assert np.all((mean[~infl] > 0.812206 - sd) & (mean[~infl] < 1.229627 + sd))
    np.testing.assert_allclose(mean, golden["oracle_scale_mean"], rtol=1e-9, atol=0.)
    np.testing.assert_allclose(run.noise.variance(var)[:, 3, 4], var[:, 3, 4] * mean, rtol=1e-15)
    bright = truth[..., 0] > 0.5 * truth[..., 0].max()
    ratio = run.posterior.parameters_std[bright] / fixed.posterior.parameters_std[bright]
    print("parameters_std, noise= over fixed variance, brightest spaxels: median (a, c, w) =", np.median(ratio, axis=0))


# ---- 9. with the other keywords ----------------------------------------------------------------------------------

def test_runs_with_adaptation_prior_histograms_and_regions(tmp_path):
    """The keywords together, one sweep per device call and 64: every output bit for bit the same; the
    first six sweeps (draws after 2, 4 and 6, the prior on) are tests/composed_oracle.py's at 1e-9."""
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., max_iterations=60, refresh_every=25,
              noise=dict(per=np.arange(16) // 4, every=2, shape=1., rate=1., spaxels="unmasked"),
              adapt_sweeps=20, adapt_window=10, smoothness=dict(c=1.),
              posterior_burn_in=20, posterior_histograms=dict(pilot=10, span=6.),
              regions=regions.blocks((9, 9), 3))
    run = d3d.Run(cube, inst, sweeps_per_call=64, **kw)
    assert np.isfinite(run.chain).all() and np.isfinite(run.parameters).all()
    assert run.noise.count == 29 and run.noise.scale.shape == (29, 4)                    # sweeps 2, 4 .. 58
    assert np.isfinite(run.noise.scale).all() and np.all(run.noise.scale > 0.)
    assert np.isfinite(run.noise.scale_mean).all() and np.isfinite(run.noise.scale_std).all()
    assert run.noise.quantiles([0.16, 0.84]).shape == (2, 4) and run.noise.channel_scale.shape == (16,)
    assert run.posterior.count == 40 and np.isfinite(run.posterior.convolved_mean).all()
    assert np.isfinite(run.posterior.histograms.median).all()
    assert np.isfinite(run.posterior.regions.flux).all()
    assert np.isfinite(run.jump_scale).all() and run.adapted_until == 20
    run.noise.save(str(tmp_path / "n"))
    assert np.load(str(tmp_path / "n_noise.npz"))["scale"].shape == (29, 4)
    one = d3d.Run(cube, inst, sweeps_per_call=1, **kw)
    a, b = CO.run_outputs(run), CO.run_outputs(one)
    assert sorted(a) == sorted(b) and "noise_scale" in a
    for k in sorted(a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    ft = CO.features_of(lam=(0., 1., 0.), adapt=dict(target=0.25, window=10, last=20, gain=2.0, range=(1e-3, 1e3)),
                        noise=dict(group=np.arange(16) // 4, every=2, start=0, shape=1., rate=1.,
                                   spaxels=np.asarray(run.mask) == 1))
    want, co = CO.chain_of_run(run, cube.data, var, inst.fsf.as_image(cube), inst.lsf.as_vector(cube), ft, 6)
    assert co.noise.sweeps == [2, 4, 6] and min(m.min() for m in co.noise.margins) > 1e-9
    np.testing.assert_allclose(run.chain[:7], want, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(run.noise.scale[:3], co.noise.scale(), rtol=1e-9, atol=0.)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------

def test_refusals():
    case = NO.shape_case((13, 5, 7))
    group, G = NO.grouping("channel", 13)
    with engine_of(case) as eng:
        for bad in (dict(n_groups=0), dict(n_groups=12), dict(shape=-1.), dict(rate=-1.), dict(every=0),
                    dict(start=-1), dict(capacity=0)):
            with pytest.raises(ValueError):
                eng.noise_begin(group, **dict(dict(n_groups=G), **bad))
        with pytest.raises(ValueError, match="a label is -1"):
            eng.noise_begin(np.full(13, -2), 1)
        with pytest.raises(RuntimeError, match="not begun"):
            eng.noise_step(1)
        with pytest.raises(RuntimeError, match="not begun"):
            eng.noise_count()
        eng.robust_begin(4)
        held = eng.get_option("device_bytes")
        with pytest.raises(NotImplementedError, match="robust weights are armed"):
            eng.noise_begin(group, G)
        assert eng.get_option("device_bytes") == held                  # (refused before any allocation)
        eng.robust_end()
        eng.post_begin()
        eng.pred_begin()
        held = eng.get_option("device_bytes")
        with pytest.raises(NotImplementedError, match="predictive accuracy is armed"):
            eng.noise_begin(group, G)
        assert eng.get_option("device_bytes") == held
        eng.pred_end()
        eng.post_end()
        eng.noise_begin(group, G)
        with pytest.raises(NotImplementedError, match="noise scales are armed"):
            eng.robust_begin(4)
        eng.post_begin()
        with pytest.raises(NotImplementedError, match="noise scales are armed"):
            eng.pred_begin()
        eng.post_end()
        with pytest.raises(NotImplementedError, match="noise scales are armed"):
            eng.set_tile(0, 0, 7, 0, 5, 0, 7)
        with pytest.raises(RuntimeError, match="d3d_noise_end first"):
            eng.set_data(case["data"], case["var"], mask=case["mask"])
        with pytest.raises(RuntimeError, match="d3d_noise_end first"):
            eng.upload_slot(_lib.SLOT_IVAR, case["var"])
        eng.noise_end()
        eng.set_tile(0, 0, 7, 0, 5, 0, 7)
        with pytest.raises(NotImplementedError, match="on a tile"):
            eng.noise_begin(group, G)
    with _lib.Engine((13, 5, 7), (5, 5)) as eng:
        with pytest.raises(RuntimeError, match="data not set"):
            eng.noise_begin(group, G)
    # a tempered context, and a tempering group of armed contexts
    with engine_of(case) as a, engine_of(case) as b:
        temper = _lib.TemperGroup([a, b], [1., 0.5], seed=1)
        with pytest.raises(NotImplementedError, match="tempered context"):
            a.noise_begin(group, G)
        temper.close()
        a.noise_begin(group, G)
        with pytest.raises(NotImplementedError, match="noise scales are armed"):
            _lib.TemperGroup([a, b], [1., 0.5], seed=1)
    # chains that share a launch write their pending updates back together: armed alike, or refused
    with engine_of(case) as a, engine_of(case) as b:
        begin(a, group, G, start=0)
        with pytest.raises(ValueError, match="noise scales"):
            _lib.mh_sweeps_batch([a, b], 1, 1)
        begin(b, group, G, start=0, every=2)
        with pytest.raises(ValueError, match="noise scales"):
            _lib.mh_sweeps_batch([a, b], 1, 1)
        begin(b, *NO.grouping("cube", 13), start=0)
        _lib.mh_sweeps_batch([a, b], 2, 1)
        assert a.noise_count() == b.noise_count() == 2
    # Run: the keywords it cannot be combined with
    inst, cube, var, _, _ = synthetic_cube(D=16, H=9, W=9, seed=4)
    for other, what in ((dict(robust=4), "noise= with robust="),
                        (dict(predictive=True, posterior_burn_in=2), "noise= with predictive="),
                        (dict(tempering=dict(rungs=2, beta_min=0.5)), "noise= with tempering=")):
        with pytest.raises(ValueError, match=what):
            d3d.Run(cube, inst, variance=var, max_iterations=4, noise=True, **other)
