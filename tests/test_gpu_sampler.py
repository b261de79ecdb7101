"""
The DEVICE's random layer (csrc/d3d_rng.h) against references that are not the oracle: the
published Philox known answers, the exact inverse CDF of the truncated normal and the exact
posterior of a one-spaxel problem, all from tests/golden/sampler_reference.npz
(tests/sampler_reference.py writes it; tests/test_sampler_reference_cpu.py is the CPU half).
Lines that begin with "sampler-check" are the figures of profiles/sampler_checks.txt.
"""
import numpy as np
import pytest
from scipy import stats

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with _lib.Engine((4, 3, 3), (1, 1)) as e:
        yield e


@pytest.fixture(scope="module")
def fixture():
    return np.load(R.FIXTURE, allow_pickle=False)


# ---- Philox -------------------------------------------------------------------------------------

def units_of(words):
    """u64_to_unit of the words as philox_pair pairs them, in exact integer arithmetic."""
    w = words.astype(np.uint64)
    lo = (w[:, 1] << np.uint64(32)) | w[:, 0]
    hi = (w[:, 3] << np.uint64(32)) | w[:, 2]
    return np.stack([((v >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52 for v in (lo, hi)], axis=1)


def test_device_philox_reproduces_the_random123_known_answers(eng, fixture):
    words, pairs = eng.philox(fixture["philox_counters"], fixture["philox_keys"])
    np.testing.assert_array_equal(words, fixture["philox_words"])
    np.testing.assert_array_equal(pairs, units_of(fixture["philox_words"]))


def test_device_philox_equals_the_oracle_on_random_counters_and_keys(eng):
    rng = np.random.default_rng(20240)
    n = 4096                                         # 16 workgroups of the hook, the last one full
    counters = rng.integers(0, 2 ** 32, size=(n + 37, 4), dtype=np.uint64).astype(np.uint32)   # and one that is not
    keys = rng.integers(0, 2 ** 32, size=(n + 37, 2), dtype=np.uint64).astype(np.uint32)
    words, pairs = eng.philox(counters, keys)
    want = np.array([O.philox4x32_10(c, k) for c, k in zip(counters.tolist(), keys.tolist())], dtype=np.uint32)
    np.testing.assert_array_equal(words, want)
    np.testing.assert_array_equal(pairs, units_of(want))
    assert pairs.min() >= 2.0 ** -53 and pairs.max() <= 1.0 - 2.0 ** -53
    assert eng.philox(np.zeros((0, 4)), np.zeros((0, 2)))[0].shape == (0, 4)
    with pytest.raises(ValueError):
        eng.philox(counters[:3], keys[:2])


def test_device_philox_with_wide_seeds_and_spaxel_indices(eng):
    """The chain's layout -- counter (global spaxel, sweep, block, 0), key (seed low, seed high) --
    at seeds above 2^32 (both key words in use) and spaxel indices up to 2^32 - 1, against the
    oracle's philox_pair; and Engine.rtnorm with such a seed against the oracle's draws."""
    seeds = [12345, 12345 + 2 ** 32, 2 ** 32, 0x9e3779b97f4a7c15, 2 ** 64 - 1]
    spaxels = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    rows = [(seed, sp, sweep, blk) for seed in seeds for sp in spaxels
            for sweep in (0, 1, 2 ** 32 - 1) for blk in (0, 2, 999)]
    counters = np.array([(sp, sweep, blk, 0) for _, sp, sweep, blk in rows], dtype=np.uint32)
    keys = np.array([(seed & 0xFFFFFFFF, seed >> 32) for seed, _, _, _ in rows], dtype=np.uint32)
    _, pairs = eng.philox(counters, keys)
    want = np.array([O.philox_pair(*row) for row in rows])
    np.testing.assert_array_equal(pairs, want)
    # the high word of the seed is in the key: 12345 and 12345 + 2^32 are different streams
    per_seed = pairs.reshape(len(seeds), -1)
    assert len({row.tobytes() for row in per_seed}) == len(seeds)
    seed = 0x0123456789abcdef
    x = eng.rtnorm(0.0, 9.0, 4.0, 3.0, size=64, seed=seed)
    want = R.oracle_draws(0.0, 9.0, 4.0, 3.0, 64, seed=seed)
    np.testing.assert_allclose(x, want, rtol=0, atol=1e-12)
    assert not np.array_equal(x, eng.rtnorm(0.0, 9.0, 4.0, 3.0, size=64, seed=seed & 0xFFFFFFFF))


# ---- truncated normal, inverse-CDF branches -----------------------------------------------------

@pytest.mark.parametrize("k", range(len(R.INVCDF_REGIMES)), ids=[r[4] for r in R.INVCDF_REGIMES])
def test_inverse_cdf_draws_sit_on_the_exact_ones(eng, fixture, k):
    """alpha < 6: the device's draw i against x*_i = F^-1(u_i) by mpmath, as |x - x*| dF/dx, a
    distance in probability.  Device and oracle evaluate one formula, so they share its
    conditioning (1e-16 in the body, 1e-6 in an interval 1e-9 wide at 3 sigma); their libm differ
    by a few ulp: the bar is 8 times the oracle's own maximum, plus 2^-50."""
    lo, hi, mu, sigma, label = R.INVCDF_REGIMES[k]
    np.testing.assert_array_equal(fixture["regimes"][k], [lo, hi, mu, sigma])
    bar = 8.0 * fixture["oracle_max"][k] + 2.0 ** -50
    for wave in (False, True):
        x = eng.rtnorm(lo, hi, mu, sigma, size=R.N_EXACT, seed=R.SEED, wave_mode=wave)
        assert np.all(x >= lo) and np.all(x <= hi), label
        err = R.probability_error(x, fixture["x_star"][k], fixture["x_star_lo"][k], fixture["density"][k])
        print("sampler-check inverse-cdf %-52s %-6s device max %.3g  oracle max %.3g  bar %.3g"
              % (label, "wave" if wave else "scalar", err.max(), fixture["oracle_max"][k], bar))
        assert err.max() <= bar, (label, wave, err.max(), bar)


# ---- truncated normal, tail branch --------------------------------------------------------------

@pytest.mark.parametrize("lo,hi,mu,sigma,label", R.TAIL_REGIMES, ids=[r[4] for r in R.TAIL_REGIMES])
def test_tail_draws_follow_the_truncated_normal(eng, lo, hi, mu, sigma, label):
    """alpha >= 6, also in intervals far narrower than the exponential proposal (which used to
    give up there after 1000 trials and return the bound)."""
    x = eng.rtnorm(lo, hi, mu, sigma, size=R.N_KS, seed=R.SEED)
    assert x.shape == (R.N_KS,)
    assert np.all(x > lo) and np.all(x < hi), (label, np.mean(x == lo), np.mean(x == hi))
    ks = stats.kstest(x, lambda t: R.truncnorm_cdf(t, lo, hi, mu, sigma))
    print("sampler-check tail %-40s KS D %.4f p %.3f" % (label, ks.statistic, ks.pvalue))
    assert ks.pvalue > 1e-3, (label, ks)
    np.testing.assert_array_equal(eng.rtnorm(lo, hi, mu, sigma, size=2048, seed=R.SEED, wave_mode=True), x[:2048])
    # draw for draw the oracle's: log differs by ulps between the libms, which moves a draw of the
    # exponential proposal by that fraction of its distance from the bound (1e-12 of the interval
    # allowed); z may then round to the neighbouring double, and alpha + u width and mu + sigma z
    # round twice more where they are not fused (4 ulp of sigma z, the largest term)
    want = R.oracle_draws(lo, hi, mu, sigma, 200)
    width = min(hi - lo, 10.0 * sigma)
    tol = 1e-12 * width + 4 * np.spacing(abs(mu) + max(abs(lo), abs(hi)))
    assert np.max(np.abs(x[:200] - want)) <= tol, (label, np.max(np.abs(x[:200] - want)), tol)


# ---- a long chain against the exact posterior ---------------------------------------------------

# a seed of its own each: the families draw the same numbers from one seed, and seed 11 is the
# oracle's chain of tests/test_sampler_reference_cpu.py
CHAINS = [  # (kind, options, small_parts, mh_defer as run, seed)
    ("general", {}, 1, 1, 21),
    ("general", {"mh_small": 0}, 0, 1, 22),
    ("general", {"mh_defer": 0}, 0, 0, 23),
    ("uniform", {}, 1, 1, 24),
    ("doublet", {}, 1, 1, 25),
]


@pytest.mark.parametrize("kind,opts,small,defer,seed", CHAINS,
                         ids=["default", "mh_small=0", "mh_defer=0", "uniform variance", "doublet"])
def test_device_chain_samples_the_exact_posterior(fixture, kind, opts, small, defer, seed):
    """16 independent one-spaxel problems in one cube (disjoint 3x3 windows, one data patch tiled):
    16 replicas of one posterior on 16 Philox streams.  1000 + 3000 sweeps; mean and second
    moment of (a, c, w), P(w > 3.5), P(c < 7.5) over the replicas against the quadrature:
    z = (mean over replicas - exact) / (sd over replicas / 4), Student's t with 15 degrees of
    freedom, |z| < 4.5 (two-sided p 4e-4 per statistic)."""
    prob = R.posterior_problem(kind)
    exact = fixture["posterior_" + kind]
    D, H, W = prob["data"].shape
    first, last = R.POST_BURN + 1, R.POST_BURN + R.POST_KEEP
    with _lib.Engine((D, H, W), prob["fsf"].shape, options=opts) as e:
        e.set_taps(prob["fsf"], None)
        e.set_data(prob["data"], prob["var"], mask=prob["mask"])
        if prob["line_shape"] is not None:
            e.set_line_shape(*prob["line_shape"])
        e.set_params(prob["init"])
        e.mh_config(R.POST_MIN_B, R.POST_MAX_B, R.POST_JUMP, R.POST_RA, seed=seed, refresh_every=0)
        assert e.get_option("small_parts") == small and e.get_option("mh_defer") == defer
        assert e.variance_is_uniform() == (kind == "uniform")
        e.mh_sweeps(R.POST_BURN, 1)
        chain = np.full((last + 1, H, W, 3), np.nan)
        accepted = e.mh_sweeps(R.POST_KEEP, first, 1, chain, None)
    kept = chain[first:]
    assert np.all(np.isfinite(kept[:, prob["mask"] == 1]))
    z = R.z_scores(kept, exact)
    print("sampler-check posterior %-20s seed %d accepted %.3f  z: %s"
          % (kind + " " + ",".join("%s=%d" % kv for kv in opts.items()), seed, accepted / (16.0 * R.POST_KEEP),
             ", ".join("%s %+.2f" % (n, v) for n, v in zip(R.POST_STATS, z))))
    assert np.all(np.abs(z) < 4.5), dict(zip(R.POST_STATS, np.round(z, 2)))
