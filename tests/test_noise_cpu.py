"""
CPU tests (no GPU) of the noise scales (Run(noise=...), deconv3d_amd/noise.py, tests/noise_oracle.py):
the oracle's array Philox is the oracle's; its Marsaglia-Tsang draw has the Gamma distribution it
claims and the scale the mean the formula gives; no accept decision of a draw the GPU tests compare
is closer than 1e-9 to flipping; the sums' order is the documented one; the keyword is validated and
robust=, predictive=, tempering=, a host-evaluated model and a checkpoint written with other values
are refused before any device work; the report; the C entry points are declared, bound, built and
cite the reference lines they extend.
"""
import os
import re

import numpy as np
import pytest
from scipy import stats

import deconv3d_amd as d3d
from deconv3d_amd import _lib, noise
from oracle import deconv3d_oracle as O
from tests import noise_oracle as NO
from tests import robust_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_noise_begin", "d3d_noise_step", "d3d_noise_count", "d3d_noise_get", "d3d_noise_end")
N_DRAWS = 20000


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- the draw -------------------------------------------------------------------------------

def test_array_philox_is_the_oracles_and_the_tag_is_its_own():
    index = np.array([0, 1, 77, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.uint64)
    for seed, sweep, block in ((12345, 1, 0), (2 ** 40 + 3, 2 ** 31 + 7, 31)):
        ux, uy = NO.philox_pairs(seed, index, sweep, block)
        for i, v in enumerate(index):
            r = O.philox4x32_10((int(v), sweep, block, NO.TAG), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
            assert ux[i] == O.u64_to_unit((r[1] << 32) | r[0])
            assert uy[i] == O.u64_to_unit((r[3] << 32) | r[2])
    assert NO.TAG not in (0, RO.TAG)
    # (with robust's tag it is robust's stream: one arithmetic, the tag an argument)
    np.testing.assert_array_equal(NO.philox_pairs(9, index, 4, 2, RO.TAG), RO.philox_pairs(9, index, 4, 2))
    # every tag of csrc/ differs from this one
    tags = set()
    csrc = os.path.join(ROOT, "deconv3d_amd", "csrc")
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            tags.update(re.findall(r"_TAG\s*=\s*(0x[0-9A-Fa-f]+)u", open(os.path.join(csrc, name)).read()))
    values = sorted(int(t, 16) for t in tags)
    assert NO.TAG in values and RO.TAG in values and len(values) == len(set(values))


@pytest.mark.parametrize("alpha", [1., 1.5, 8., 72.5, 45000.])
def test_the_draw_is_a_gamma(alpha):
    g, margin, attempts = NO.gamma_draw(99, np.arange(N_DRAWS, dtype=np.uint64), 5, alpha)
    ks = stats.kstest(g, stats.gamma(alpha).cdf)
    print("alpha", alpha, ks, "attempts: mean", attempts.mean(), "max", attempts.max())
    assert ks.pvalue > 1e-3, (alpha, ks)
    assert attempts.max() < NO.ATTEMPTS and margin.min() > 0.


@pytest.mark.parametrize("shape, rate, n, q", [(0., 0., 9., 5.), (2., 3., 145., 160.), (0., 0., 90000., 88000.)])
def test_the_mean_scale_at_fixed_sums(shape, rate, n, q):
    """E[s] = (b0 + Q/2) / (alpha - 1) of an InvGamma(alpha, b0 + Q/2), within 4 standard errors of
    20 000 draws (its variance is mean^2 / (alpha - 2))."""
    alpha, b = shape + 0.5 * n, rate + 0.5 * q
    g, _, _ = NO.gamma_draw(7, np.arange(N_DRAWS, dtype=np.uint64), 3, alpha)
    s = 1. / (g / b)
    want = b / (alpha - 1.)
    se = want / np.sqrt(alpha - 2.) / np.sqrt(N_DRAWS)
    print("alpha", alpha, "mean", s.mean(), "want", want, "se", se)
    assert abs(s.mean() - want) <= 4. * se


def test_the_sums_take_the_documented_order():
    """Spaxel by spaxel in plain Python: stream j = spaxel % 1024, in turn; partials in index order;
    channels of a group in increasing z."""
    rng = np.random.default_rng(3)
    D, H, W = 3, 37, 31
    err, i0 = rng.normal(0., 2., (D, H, W)), rng.random((D, H, W)) + 0.5
    i0[1, 4, 5] = 0.
    err[1, 4, 5] = np.nan
    sp = NO.holes(H, W)
    q_z, n_z = NO.channel_sums(err, i0, sp)
    for z in range(D):
        part, n = [0.0] * NO.STREAMS, 0
        for s in range(H * W):
            y, x = divmod(s, W)
            if sp[y, x] and i0[z, y, x] != 0.:
                part[s % NO.STREAMS] = part[s % NO.STREAMS] + (err[z, y, x] * err[z, y, x]) * i0[z, y, x]
                n += 1
        q = 0.0
        for p in part:
            q = q + p
        assert q == q_z[z] and n == n_z[z]
    group = np.array([1, -1, 1])
    q_g, n_g = NO.group_sums(q_z, n_z, group, 3)
    assert q_g[1] == q_z[0] + q_z[2] and n_g[1] == n_z[0] + n_z[2] and q_g[0] == q_g[2] == 0.
    got = NO.draw_scales(5, 2, err, i0, group, sp, G=3)
    assert np.isnan(got["scale"][[0, 2]]).all() and got["scale"][1] == 1. / got["tau_g"][1]
    np.testing.assert_array_equal(got["tau"], [got["tau_g"][1], 1., got["tau_g"][1]])
    # a rate of exactly zero keeps the previous tau
    zero = NO.draw_scales(5, 2, np.zeros((D, H, W)), i0, group, sp, G=3, tau_before=[1., 0.25, 1.])
    assert zero["tau_g"][1] == 0.25 and zero["scale"][1] == 4.


def margins_of(seed, sweeps, group, G, n_z):
    _, n_g = NO.group_sums(np.zeros(len(n_z)), n_z, group, G)
    idx = np.nonzero(n_g >= 2.)[0]
    out = []
    for s in sweeps:
        out.append(NO.gamma_draw(seed, idx, s, 0.5 * n_g[idx])[1])
    return np.concatenate(out)


def test_no_compared_decision_is_within_1e9_of_flipping():
    """The accept decision of a draw depends on (seed, sweep, group, N_g) alone.  For every draw
    tests/test_gpu_noise.py compares with the oracle -- the step cases, the chain on c1, the recovery
    run -- |log u3 - bound| and |v| exceed 1e-9: a last-bit difference in log or cos flips none."""
    from tests.cases import make_case
    from tests.test_gpu_run import synthetic_cube
    worst = np.inf
    for shape in NO.STEP_SHAPES:
        case = NO.shape_case(shape)
        i0 = NO.base_ivar(case["data"], case["var"])
        for sp in (None, NO.holes(case["H"], case["W"])):
            _, n_z = NO.channel_sums(np.zeros(i0.shape), i0, sp)
            for name in NO.GROUPINGS:
                group, G = NO.grouping(name, case["D"])
                worst = min(worst, margins_of(NO.STEP_SEED, [NO.STEP_SWEEP], group, G, n_z).min())
    case = make_case("c1")
    i0 = NO.base_ivar(case["data"], case["var"])
    _, n_z = NO.channel_sums(np.zeros(i0.shape), i0)
    worst = min(worst, margins_of(77, range(1, 6), NO.group_of("channel", i0.shape[0]), i0.shape[0], n_z).min())
    # the recovery run: synthetic_cube(32, 12, 12) has no NaN voxel, every channel counts its 144 voxels
    n_z = np.full(32, 144.)
    worst = min(worst, margins_of(NO.RECOVERY_SEED, range(1, NO.RECOVERY_ITERATIONS), NO.group_of("channel", 32),
                                  32, n_z).min())
    print("smallest margin", worst)
    assert worst > 1e-9


# ---- keywords ---------------------------------------------------------------------------------

def test_keywords_become_a_dict():
    assert noise.check_keywords(None) is None and noise.check_keywords(False) is None
    want = dict(per="channel", every=1, start=0, shape=0., rate=0., spaxels="all")
    assert noise.check_keywords(True) == want and noise.check_keywords({}) == want
    got = noise.check_keywords(dict(per="cube", every=np.int64(3), start=7, shape=2, rate=0.5, spaxels="unmasked"))
    assert got == dict(per="cube", every=3, start=7, shape=2., rate=0.5, spaxels="unmasked")
    got = noise.check_keywords(dict(per=[0, -1, 2, 2], spaxels=[[1, 0], [1, 1]]))
    np.testing.assert_array_equal(got["per"], [0, -1, 2, 2])
    mask = np.array([[1., 0.], [1., 1.]])
    cfg = noise.resolve(got, 4, mask)
    assert cfg["G"] == 3 and cfg["group"].dtype == np.int32 and cfg["map"].dtype == np.uint8
    np.testing.assert_array_equal(cfg["map"], [[1, 0], [1, 1]])
    cfg = noise.resolve(noise.check_keywords(True), 5, mask)
    np.testing.assert_array_equal(cfg["group"], np.arange(5))
    assert cfg["G"] == 5 and cfg["map"] is None
    cfg = noise.resolve(noise.check_keywords(dict(per="cube", spaxels="unmasked")), 5, mask)
    np.testing.assert_array_equal(cfg["group"], np.zeros(5))
    np.testing.assert_array_equal(cfg["map"], [[1, 0], [1, 1]])
    for bad in (dict(per=[0, 1, 2]), dict(spaxels=np.ones((3, 2), dtype=int))):
        with pytest.raises(ValueError, match="noise"):
            noise.resolve(noise.check_keywords(bad), 4, mask)
    k = dict(every=3, start=2)
    assert noise.last_due(k, 1) is None and [noise.last_due(k, s) for s in (2, 4, 5, 6)] == [2, 2, 5, 5]
    # rows: the due sweeps among origin + 1 .. origin + max_iterations - 1, and one for a re-made draw
    assert noise.capacity(dict(every=1, start=0), 6) == 5 + 1
    assert noise.capacity(dict(every=2, start=1), 8) == 4 + 1              # 1, 3, 5, 7
    assert noise.capacity(dict(every=2, start=1), 8, 10) == 4 + 1          # 11, 13, 15, 17
    assert noise.capacity(dict(every=1, start=10 ** 9), 100) == 1
    assert noise.capacity(dict(every=5, start=3), 4) == 1 + 1              # 3


@pytest.mark.parametrize("value", [
    4, "channel", dict(per="spaxel"), dict(per=[0.5, 1.]), dict(per=[-2, 0]), dict(per=[-1, -1]), dict(every=0),
    dict(every=1.5), dict(start=-1), dict(shape=-1.), dict(rate=-0.5), dict(rate=np.nan), dict(shape="1"),
    dict(spaxels="some"), dict(spaxels=[[0, 2]]), dict(spaxels=[1, 0]), dict(nu=4), (1, 2),
    dict(per=np.zeros(5, dtype=int)), dict(spaxels=np.ones((3, 3), dtype=int)),
])
def test_run_refuses_bad_keywords_before_any_device_work(value):
    with pytest.raises(ValueError, match="noise"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, noise=value)


@pytest.mark.parametrize("other, what", [
    (dict(robust=4), "noise= with robust="),
    (dict(predictive=True, posterior_burn_in=10), "noise= with predictive="),
    (dict(tempering=dict(rungs=2, beta_min=0.5)), "noise= with tempering="),
])
def test_run_refuses_robust_predictive_and_tempering(other, what):
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, noise=True, **other)


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="noise=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, noise=True)


# ---- the checkpoint record ------------------------------------------------------------------------

def resolved(value, depth=8, mask=None):
    return noise.resolve(noise.check_keywords(value), depth, np.ones((9, 9)) if mask is None else mask)


def state_of(value=None):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=1)
    if value is not None:
        state.update(noise.keyword_record(resolved(value)))
    return state


def test_the_record_holds_the_keywords():
    rec = noise.keyword_record(resolved(dict(per="cube", every=2, start=5, shape=1.5, rate=0.25)))
    np.testing.assert_array_equal(rec["noise_keywords"], [2, 5, 1.5, 0.25, 1])
    np.testing.assert_array_equal(rec["noise_group"], np.zeros(8))
    assert rec["noise_spaxels"].size == 0
    rec = noise.keyword_record(resolved(dict(spaxels="unmasked")))
    np.testing.assert_array_equal(rec["noise_spaxels"], np.ones((9, 9)))


@pytest.mark.parametrize("saved, kw, what", [
    (True, dict(noise=dict(every=2)), "other every, start, shape, rate"),
    (True, dict(noise=dict(per="cube")), "other every, start, shape, rate or number of groups"),
    (dict(per=[0, 0, 0, 0, 1, 1, 1, 1]), dict(noise=dict(per=[0, 0, 0, 1, 1, 1, 1, 1])), "channel groups"),
    (True, dict(noise=dict(spaxels="unmasked")), "counted spaxels"),
    (True, dict(), "this run has none"),
    (None, dict(noise=True), "written without noise="),
])
def test_run_refuses_a_state_written_with_other_values(saved, kw, what):
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(saved), **kw)


def test_resume_accepts_the_same_values():
    value = dict(per="cube", every=2, start=5, shape=1.)
    state = state_of(value)
    noise.check_resume(state, state, resolved(value))
    noise.check_resume(state_of(), state_of(), None)


# ---- the report --------------------------------------------------------------------------------

def test_report_and_pooled_report(tmp_path):
    cfg = resolved(dict(per=[0, 0, -1, 1, 2, 2, 2, 2]))
    calls = []
    scale_a = np.array([[1., 4., np.nan], [3., 6., np.nan], [5., 8., np.nan]])

    def fetch_a():
        calls.append(1)
        return scale_a, np.array([2, 3, 4]), np.array([162., 81., 0.]), np.array([150., 300., 0.]), np.ones(8)

    a = noise.NoiseReport(cfg, fetch_a, burn_in=3)
    assert calls == [] and a.n_groups == 3                                          # nothing fetched yet
    assert a.count == 3 and calls == [1]
    np.testing.assert_array_equal(a.scale, scale_a)
    np.testing.assert_array_equal(a.sweeps, [2, 3, 4])
    np.testing.assert_array_equal(a.voxels, [162., 81., 0.])
    np.testing.assert_array_equal(a.scale_mean, [4., 7., np.nan])                   # sweeps 3 and 4
    np.testing.assert_allclose(a.scale_std[:2], [np.sqrt(2.), np.sqrt(2.)])
    np.testing.assert_array_equal(a.quantiles([0., 1.])[:, :2], [[3., 6.], [5., 8.]])
    np.testing.assert_array_equal(a.channel_scale, [4., 4., np.nan, 7., np.nan, np.nan, np.nan, np.nan])
    np.testing.assert_array_equal(a.variance(np.full((8, 1, 2), 2.))[:, 0, 0], [8., 8., 2., 14., 2., 2., 2., 2.])
    assert calls == [1]                                                             # once
    everything = noise.NoiseReport(cfg, fetch_a)
    np.testing.assert_array_equal(everything.scale_mean, [3., 6., np.nan])
    # a resumed run's re-made draw lies before its first sweep: not reported
    resumed = noise.NoiseReport(cfg, fetch_a, first_sweep=3)
    np.testing.assert_array_equal(resumed.sweeps, [3, 4])
    b = noise.NoiseReport(cfg, lambda: (scale_a[:2] + 1., np.array([3, 4]), np.array([162., 81., 0.]),
                                        np.zeros(3), np.ones(8)), burn_in=3)
    both = noise.pooled([a, b])
    assert both.count == 5
    np.testing.assert_array_equal(both.sweeps, [2, 3, 4, 3, 4])
    np.testing.assert_array_equal(both.scale_mean[:2], [(3. + 5. + 2. + 4.) / 4., (6. + 8. + 5. + 7.) / 4.])
    empty = noise.NoiseReport(cfg, lambda: (np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros(3), np.zeros(3),
                                            np.ones(8)))
    assert empty.count == 0 and np.isnan(empty.scale_mean).all() and np.isnan(empty.channel_scale).all()
    assert np.isnan(empty.quantiles(0.5)).all()
    np.testing.assert_array_equal(empty.variance(3.)[:, 0, 0], np.full(8, 3.))
    both.save(str(tmp_path / "r"))
    saved = np.load(str(tmp_path / "r_noise.npz"))
    assert saved["scale"].shape == (5, 3) and int(saved["burn_in"]) == 3
    np.testing.assert_array_equal(saved["groups"], cfg["group"])
    assert d3d.NoiseReport is noise.NoiseReport


# ---- the C ABI -----------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_built_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("noise-scale inference: variance factors of channel groups"):]
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.NOISE_PROTOTYPES
        decl = section.index("int %s(" % name)
        comment = section[section.rindex("/*", 0, decl):decl]
        assert "lib/run.py:171-200" in comment and "lib/run.py:407-426" in comment, name
    for name in ("noise_begin", "noise_step", "noise_count", "noise_get", "noise_end"):
        assert callable(getattr(_lib.Engine, name))
    make = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\bd3d_noise\.hip\b", make, flags=re.M)
    import __graft_entry__ as entry
    assert "d3d_noise.hip" in entry.SOURCES                                    # d3d_source_hash covers it
    src = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "d3d_noise.hip")).read()
    assert "fp contract(off)" in src and "0x%08x" % NO.TAG in src.lower()
    assert "NOISE_STREAMS = %d" % NO.STREAMS in open(os.path.join(ROOT, "deconv3d_amd", "csrc", "d3d_ctx.h")).read()
