"""
The chain's random layer against references that are not the oracle (tests/sampler_reference.py),
CPU half: the oracle's Philox against the published known answers, the committed fixture against
its generator, the cost and the distribution of the oracle's tail sampler in intervals narrower
than its exponential proposal, and a long oracle chain against the exact posterior.  The device
half is tests/test_gpu_sampler.py; the device restates the oracle and is compared with it draw by draw
there.
"""
import numpy as np
import pytest
from scipy import stats

from oracle import deconv3d_oracle as O
from tests import sampler_reference as R


@pytest.fixture(scope="module")
def fixture():
    return np.load(R.FIXTURE, allow_pickle=False)


def test_oracle_philox_reproduces_the_random123_known_answers():
    for counter, key, words in R.PHILOX_KAT:
        assert O.philox4x32_10(counter, key) == words
    # the layout of philox_pair: counter = (spaxel, sweep, block, 0), key = (seed low, seed high),
    # uniforms of words (1, 0) and (3, 2)
    seed, sp, sweep, blk = 0x299f31d0a4093822, 0x243f6a88, 0x85a308d3, 0x13198a2e
    r = O.philox4x32_10((sp, sweep, blk, 0), (0xa4093822, 0x299f31d0))
    assert O.philox_pair(seed, sp, sweep, blk) == (O.u64_to_unit((r[1] << 32) | r[0]),
                                                   O.u64_to_unit((r[3] << 32) | r[2]))
    assert O.u64_to_unit(0) == 2.0 ** -53 and O.u64_to_unit(2 ** 64 - 1) == 1.0 - 2.0 ** -53


def test_fixture_holds_the_regimes_and_uniforms_of_the_module(fixture):
    """Without mpmath: what of the fixture can be rebuilt here is what the module says."""
    np.testing.assert_array_equal(fixture["regimes"], np.array([r[:4] for r in R.INVCDF_REGIMES]))
    assert np.signbit(fixture["regimes"][-1, 0]) and fixture["regimes"][-1, 0] == 0.0   # -0.0 survives
    np.testing.assert_array_equal(fixture["u"], R.uniforms())
    np.testing.assert_array_equal(fixture["philox_words"], np.array([k[2] for k in R.PHILOX_KAT], dtype=np.uint32))
    assert fixture["x_star"].shape == (len(R.INVCDF_REGIMES), R.N_EXACT)
    for (lo, hi, mu, sigma, label), xs in zip(R.INVCDF_REGIMES, fixture["x_star"]):
        assert not R.is_tail(lo, hi, mu, sigma), label
        assert np.all(xs >= lo) and np.all(xs <= hi), label
    for lo, hi, mu, sigma, label in R.TAIL_REGIMES:
        assert R.is_tail(lo, hi, mu, sigma), label


def test_committed_fixture_is_what_the_reference_generates(fixture):
    pytest.importorskip("mpmath")
    fresh = R.build_fixture()
    assert sorted(fresh) == sorted(fixture.files)
    for name in fresh:
        if name.startswith("posterior_"):
            # numpy's exp differs in the last bit between CPUs; 1e-10 is a millionth of what the chains resolve
            np.testing.assert_allclose(fixture[name], fresh[name], rtol=1e-10, atol=0, err_msg=name)
        elif name == "oracle_max":
            # a maximum of rounding errors of scipy's erfc / ndtr and their inverses: another libm moves it
            # by ulps of the draw, a fraction of the figure itself; the device's bar is 8 times it
            np.testing.assert_allclose(fixture[name], fresh[name], rtol=0.25, atol=0, err_msg=name)
        else:
            assert fixture[name].dtype == fresh[name].dtype, name
            np.testing.assert_array_equal(fixture[name], fresh[name], err_msg=name)


def test_oracle_inverse_cdf_draws_sit_on_the_exact_ones(fixture):
    """The oracle's error in probability, regime by regime, is the stored maximum (to the quarter of
    it that another libm may move it by) -- and that is
    the conditioning of the formula in fp64, not a defect: at most 4 ulp of the larger CDF value
    over the mass of the interval (2 erfc / ndtr evaluations of relative error 1e-16 each, one
    rounding of their combination, one inversion), times a libm allowance of 4."""
    for k, (lo, hi, mu, sigma, label) in enumerate(R.INVCDF_REGIMES):
        x = R.oracle_draws(lo, hi, mu, sigma, R.N_EXACT)
        err = R.probability_error(x, fixture["x_star"][k], fixture["x_star_lo"][k], fixture["density"][k])
        assert abs(err.max() - fixture["oracle_max"][k]) <= 0.25 * fixture["oracle_max"][k], label
        a, b = (lo - mu) / sigma, (hi - mu) / sigma
        if b <= 0:
            a, b = -b, -a
        side = stats.norm.sf if a > 0 else stats.norm.cdf
        mass = abs(side(a) - side(b))
        cond = 16 * np.finfo(float).eps * max(side(a), side(b)) / mass
        # + the draw's own rounding: half an ulp of x (and of the standardised bounds) times the density
        scale = max(abs(v) for v in (lo, hi, mu) if np.isfinite(v))
        cond += 4 * np.spacing(scale) * fixture["density"][k].max()
        assert err.max() <= cond, (label, err.max(), cond)


@pytest.mark.parametrize("lo,hi,mu,sigma,label", R.TAIL_REGIMES)
def test_oracle_tail_sampler_is_cheap_and_exact_in_narrow_intervals(lo, hi, mu, sigma, label):
    """A trial of the exponential proposal (lam * width >= 1) lands inside the interval with
    probability >= 1 - 1/e and Robert's test then accepts with probability >= 0.98 at alpha >= 6;
    a trial of the uniform proposal (lam * width < 1) is accepted with probability
    exp(-(z^2 - alpha^2) / 2) >= exp(-lam (z - alpha)), on average >= (1 - exp(-lam width)) /
    (lam width) >= 1 - 1/e.  So >= 0.62 per trial either way: the mean number of Philox blocks is
    <= 1.62, and 25 trials fail with probability 3e-11."""
    count = []
    x = R.oracle_draws(lo, hi, mu, sigma, 2000, count=count)
    assert np.mean(count) <= 2.0 and max(count) <= 25, (label, np.mean(count), max(count))
    assert np.all(x > lo) and np.all(x < hi), label
    ks = stats.kstest(x, lambda t: R.truncnorm_cdf(t, lo, hi, mu, sigma))
    assert ks.pvalue > 1e-3, (label, ks)


def test_wide_tail_intervals_keep_their_draws():
    """lam (beta - alpha) >= 1 takes the untruncated proposal as before: the formula restated."""
    for lo, hi, mu, sigma, label in R.TAIL_REGIMES[:4]:
        a, b = (lo - mu) / sigma, (hi - mu) / sigma
        if b <= 0:
            a, b = -b, -a
        lam = 0.5 * (a + np.sqrt(a * a + 4.0))
        assert lam * (b - a) >= 1.0, label
        x = R.oracle_draws(lo, hi, mu, sigma, 50)
        for i in range(50):
            for blk in range(O.BLK_GIBBS, O.BLK_GIBBS + 1000):
                u1, u2 = O.philox_pair(R.SEED, i, 0, blk)
                z = a - np.log(u1) / lam
                if z <= b and np.log(u2) <= -0.5 * (z - lam) ** 2:
                    break
            want = mu + sigma * (z if (hi - mu) / sigma > 0 else -z)
            assert abs(x[i] - want) <= 4 * np.spacing(abs(want)), (label, i)


def test_oracle_chain_samples_the_exact_posterior(fixture):
    """4000 sweeps of the oracle's chain on the lattice of 16 independent one-spaxel problems
    (seed 11), against the quadrature: all eight z below 3 (Student's t, 15 degrees of freedom).
    The device chains of tests/test_gpu_sampler.py face 4.5."""
    prob = R.posterior_problem("general")
    exact = fixture["posterior_general"]
    chain = R.oracle_chain(prob, seed=11)
    z = R.z_scores(chain, exact)
    print("oracle chain against the exact posterior, z:",
          ", ".join("%s %+.2f" % (n, v) for n, v in zip(R.POST_STATS, z)))
    assert np.all(np.abs(z) < 3.0), dict(zip(R.POST_STATS, np.round(z, 2)))
