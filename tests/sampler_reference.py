"""
Independent references for the chain's random layer (csrc/d3d_rng.h and its restatement in
oracle/deconv3d_oracle.py).  Device and oracle are two copies of one design of ours there, so
parity between them says nothing about the design.  This module looks outside it:

  * the published Random123 known answers of Philox4x32-10;
  * the exact inverse CDF of the truncated normal, by mpmath at 60 digits, at the uniforms the
    sampler consumes -- so that a draw of the inverse-CDF branches can be compared with the
    number it should have been, in probability;
  * the exact posterior of a one-spaxel problem by quadrature (amplitude integrated analytically,
    midpoint grid over centre and width), for long chains to be compared with.

mpmath may be missing where the GPU tests run: everything they need is in
tests/golden/sampler_reference.npz, written by ``python -m tests.sampler_reference``;
tests/test_sampler_reference_cpu.py regenerates it and compares.  Only ``build_fixture`` and
what it calls import mpmath.
"""
import math
import os

import numpy as np

from oracle import deconv3d_oracle as O

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_reference.npz")

# --------------------------------------------------------------------------------------------- #
# Philox4x32-10: known answers of Random123 (kat_vectors), counter[4] key[2] -> words[4]          #
# --------------------------------------------------------------------------------------------- #

PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# --------------------------------------------------------------------------------------------- #
# The truncated normal                                                                          #
# --------------------------------------------------------------------------------------------- #

SEED = 2024            # the stream of tests/test_gpu_rtnorm.py: draw i is (SEED, spaxel i, sweep 0)
N_EXACT = 256          # draws per regime with an exact counterpart
INF = float("inf")

# (lo, hi, mu, sigma, label): standardised lower bound (after mirroring) below TN_TAIL = 6
INVCDF_REGIMES = [
    (0.0, 50.0, 1.0, 1.0, "body"),
    (0.0, 9.0, 4.0, 3.0, "two-sided wide"),
    (-1.0, 2.0, 0.0, 1.0, "straddles the mode"),
    (0.0, 0.5, 2.0, 1.5, "narrow"),
    (0.0, 50.0, -2.9, 1.0, "lower bound at 2.9 sigma (erfc branch)"),
    (0.0, 50.0, -5.99, 1.0, "just below the tail seam"),
    (0.0, 30.0, 45.0, 4.0, "mass against the upper bound"),
    (-9.0, -1.0, 2.0, 1.0, "mirrored body"),
    (0.0, 12.5, 3.0, 1e-3, "tiny sigma"),
    (0.0, 1e-6, 0.5, 1.0, "width 1e-6 in the body"),
    (0.0, 1e-9, -3.0, 1.0, "width 1e-9 at 3 sigma"),
    (-1e-9, 1e-9, 0.0, 1.0, "width 2e-9 across the mode"),
    (2.0, 2.0 + 1e-7, 0.0, 1.0, "width 1e-7 at 2 sigma"),
    (0.0, 50.0, -5.999999, 1.0, "a hair below the tail seam"),
    (-40.0, 40.0, 0.0, 1.0, "bounds at 40 sigma"),
    (0.0, INF, -3.0, 1.0, "no upper bound"),
    (-INF, 0.0, 3.0, 1.0, "no lower bound (mirrored)"),
    (-1.5, 0.0, 0.0, 1.0, "beta == 0.0 exactly (mirrored, then alpha == -0.0)"),
    (-0.0, 2.0, 0.0, 1.0, "alpha == -0.0 exactly"),
]

# standardised lower bound (after mirroring) at or beyond TN_TAIL: Robert's rejection sampler
TAIL_REGIMES = [
    (0.0, 50.0, -6.0, 1.0, "the tail seam, alpha = 6"),
    (0.0, 50.0, -8.0, 1.0, "far tail"),
    (0.0, 0.3, -7.0, 1.0, "tail with a near upper bound"),
    (-50.0, 0.0, 8.0, 1.0, "mirrored far tail (beta <= 0)"),
    (0.0, 1e-4, -7.0, 1.0, "tail, width 1e-4"),
    (0.0, 1e-3, -7.0, 1.0, "tail, width 1e-3"),
    (0.0, 1e-6, -20.0, 1.0, "tail at 20 sigma, width 1e-6"),
    (-1e-4, 0.0, 7.0, 1.0, "mirrored tail, width 1e-4"),
    (2.0, 2.001, -700.0, 100.0, "tail, width 1e-5 sigma at 7 sigma"),
    # lam * width of 0.71 and 0.93: the uniform proposal where its acceptance rule shapes the draw (the
    # density falls to a half and to 0.4 across the interval; above, lam * width <= 0.007 leaves it flat)
    (0.0, 0.1, -7.0, 1.0, "tail, lam * width 0.71"),
    (0.0, 0.13, -7.0, 1.0, "tail, lam * width 0.93, just under the switch"),
    (-0.13, 0.0, 7.0, 1.0, "mirrored tail, lam * width 0.93"),
]
N_KS = 20000           # draws of a KS test against the analytic CDF


def is_mirrored(lo, hi, mu, sigma):
    """The sampler's own test (beta <= 0 in fp64): the draw is minus a draw of the mirrored interval."""
    return (hi - mu) / sigma <= 0.0


def is_tail(lo, hi, mu, sigma):
    a, b = (lo - mu) / sigma, (hi - mu) / sigma
    if b <= 0.0:
        a, b = -b, -a
    return a >= O.TN_TAIL


def uniforms(n=N_EXACT, seed=SEED):
    """u_i of draw i: the first uniform of the first truncated-normal block."""
    return np.array([O.philox_pair(seed, i, 0, O.BLK_GIBBS)[0] for i in range(n)])


def oracle_draws(lo, hi, mu, sigma, n, seed=SEED, count=None):
    """The oracle's draws 0..n-1 of the stream Engine.rtnorm uses.  count: a list that receives
    the Philox blocks each draw consumed."""
    out = np.empty(n)
    for i in range(n):
        blk = [O.BLK_GIBBS]

        def draw():
            pair = O.philox_pair(seed, i, 0, blk[0])
            blk[0] += 1
            return pair
        out[i] = O.truncated_normal(lo, hi, mu, sigma, draw)
        if count is not None:
            count.append(blk[0] - O.BLK_GIBBS)
    return out


def probability_error(x, x_star, x_star_lo, density):
    """|x - x*| dF/dx: how far the draws x are from the exact ones in probability.  x* is kept as
    the double nearest to it plus the remainder, so that its own rounding (half an ulp of x, which
    a density of 1e9 turns into 1e-7 of probability) stays out of the figure."""
    return np.abs((np.asarray(x) - x_star) - x_star_lo) * density


def truncnorm_cdf(x, lo, hi, mu, sigma):
    """Analytic CDF of N(mu, sigma^2) truncated to [lo, hi] in fp64, in survival-function form where
    the interval lies on the upper side of the mean (well conditioned there)."""
    from scipy import stats
    a, b = (lo - mu) / sigma, (hi - mu) / sigma
    z = (np.asarray(x) - mu) / sigma
    if a + b > 0:
        sa, sb, sx = stats.norm.sf(a), stats.norm.sf(b), stats.norm.sf(z)
        return (sa - sx) / (sa - sb)
    ca, cb, cx = stats.norm.cdf(a), stats.norm.cdf(b), stats.norm.cdf(z)
    return (cx - ca) / (cb - ca)


def exact_draws(lo, hi, mu, sigma, u, start):
    """(x*, remainder, dF/dx at x*) of F(x*) = u (1 - u on a mirrored interval) for the normal
    N(mu, sigma^2) truncated to [lo, hi], all four taken as the exact doubles they are.  60
    digits; Newton from ``start`` (any approximate draws), on the side of the normal where the
    interval lies, with the bracket checked afterwards."""
    import mpmath as mp
    mp.mp.dps = 60
    m, s = mp.mpf(mu), mp.mpf(sigma)
    a, b = (mp.mpf(lo) - m) / s, (mp.mpf(hi) - m) / s
    r2 = mp.sqrt(2)
    upper = a + b > 0                       # survival functions there, so that nothing cancels

    def mass(z):                            # probability beyond z (upper) or below it
        return mp.erfc(z / r2) / 2 if upper else mp.erfc(-z / r2) / 2

    def pdf(z):
        return mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
    ma, mb = mass(a), mass(b)
    norm = abs(mb - ma)
    mirrored = is_mirrored(lo, hi, mu, sigma)
    xs, rem, dens = [], [], []
    for ui, x0 in zip(u, start):
        p = 1 - mp.mpf(float(ui)) if mirrored else mp.mpf(float(ui))   # F(x*) = p
        target = ma + p * (mb - ma)         # mass(z*) on either side
        z = (mp.mpf(float(x0)) - m) / s
        z = min(max(z, a), b)
        if mp.isinf(z):
            z = mp.mpf(0)
        slope = -1 if upper else 1
        for _ in range(200):
            step = (mass(z) - target) / (slope * pdf(z))
            z = min(max(z - step, a), b)
            if abs(step) <= mp.mpf(10) ** -50 * max(1, abs(z)):
                break
        else:
            raise RuntimeError("Newton did not converge for %r" % ((lo, hi, mu, sigma),))
        d = mp.mpf(10) ** -40 * max(1, abs(z))
        g0, g1 = mass(max(z - d, a)) - target, mass(min(z + d, b)) - target
        assert g0 * g1 <= 0, "root not bracketed"
        x = m + s * z
        xd = float(x)
        xs.append(xd)
        rem.append(float(x - mp.mpf(xd)))
        dens.append(float(pdf(z) / s / norm))
    return np.array(xs), np.array(rem), np.array(dens)


# --------------------------------------------------------------------------------------------- #
# One-spaxel posteriors                                                                         #
# --------------------------------------------------------------------------------------------- #

POST_D, POST_HW, POST_STEP = 16, 12, 3
POST_TRUTH = (4.0, 7.3, 3.2)
POST_SIGMA = 0.35
POST_MIN_B = np.array([0.0, 3.0, 0.5])
POST_MAX_B = np.array([10.0, 12.0, 4.0])
POST_RA = 25.0
POST_JUMP = 0.5
POST_BURN, POST_KEEP = 1000, 3000
POST_DATA_SEED = 5
POST_W_CUT, POST_C_CUT = 3.5, 7.5
POST_KINDS = ("general", "uniform", "doublet")
DOUBLET = ([0., 3.8], [1., 1.4])
POST_STATS = ("mean a", "mean c", "mean w", "var a", "var c", "var w", "P(w > 3.5)", "P(c < 7.5)")
# midpoint cells over (c, w): both thresholds on cell edges, also with half as many cells.  The
# midpoint rule's error is cell^2 / 24 times the change of the integrand's slope across the
# range, which for a probability up to an edge inside the posterior is not small: 240 x 280
# cells leave 2e-4 in P(c < 7.5), these leave 2e-5 there and 1e-7 in the moments -- against a
# Monte-Carlo error of 5e-3 of the chains (build_fixture asserts what the halved grid changes).
POST_GRID = (960, 1120)


def posterior_fsf():
    g = np.exp(-0.5 * (np.arange(3) - 1.0) ** 2 / 0.8 ** 2)
    f = np.outer(g, g)
    return f / f.sum()


def unit_line(kind, c, w):
    """Unit-amplitude line over the channels, c and w broadcast: [D, ...]."""
    z = np.arange(POST_D, dtype=np.float64).reshape((POST_D,) + (1,) * np.ndim(c))
    off, rat = DOUBLET if kind == "doublet" else ([0.], [1.])
    s = 0.
    for d, r in zip(off, rat):
        s = s + r * np.exp(-1. * ((z - c) - d) ** 2 / (2. * w ** 2))
    return s


def posterior_problem(kind, data_seed=POST_DATA_SEED):
    """The lattice of section 'exact posterior' of DESIGN.md 4: one 3x3x16 patch (data, variance)
    tiled 4x4 over 12x12, live spaxels at the patch centres -- 16 disjoint windows, 16
    independent replicas of one posterior.  kind: 'general' (per-voxel variance), 'uniform'
    (one variance) or 'doublet' (per-voxel variance, two-component line)."""
    rng = np.random.default_rng(data_seed)
    u = rng.uniform(size=(POST_D, 3, 3))
    n = rng.standard_normal((POST_D, 3, 3))
    sd = POST_SIGMA * (np.ones_like(u) if kind == "uniform" else 0.7 + 0.6 * u)
    fsf = posterior_fsf()
    a, c, w = POST_TRUTH
    patch = a * unit_line(kind, c, w)[:, None, None] * fsf + sd * n
    reps = POST_HW // POST_STEP
    mask = np.zeros((POST_HW, POST_HW), dtype=np.int64)
    mask[1::POST_STEP, 1::POST_STEP] = 1
    init = np.tile(np.array(POST_TRUTH), (POST_HW, POST_HW, 1))
    return dict(kind=kind, fsf=fsf, patch=patch, patch_var=sd ** 2,
                data=np.tile(patch, (1, reps, reps)), var=np.tile(sd ** 2, (1, reps, reps)),
                mask=mask, init=init, line_shape=DOUBLET if kind == "doublet" else None)


def exact_posterior(prob, grid=POST_GRID):
    """The eight POST_STATS of p(a, c, w | patch): flat prior on the (c, w) box, N(0, POST_RA) on
    the amplitude cut to its box -- what the chain's Gibbs step (lib/run.py:491-496) and its
    bounded Metropolis step define.  The amplitude is integrated in closed form: given (c, w) it
    is N(mu, ro) of gibbs_moments truncated to the box, of mass Z, and the (c, w) marginal is
    sqrt(ro) exp(mu^2 / 2 ro) Z."""
    from scipy.special import ndtr
    nc, nw = grid
    hc = (POST_MAX_B[1] - POST_MIN_B[1]) / nc
    hw = (POST_MAX_B[2] - POST_MIN_B[2]) / nw
    c = (POST_MIN_B[1] + hc * (np.arange(nc) + 0.5))[:, None]
    w = (POST_MIN_B[2] + hw * (np.arange(nw) + 0.5))[None, :]
    fsf, d, v = prob["fsf"], prob["patch"], prob["patch_var"]
    A = np.sum(fsf ** 2 / v, axis=(1, 2))           # s_ee = sum_z line_z^2 A_z
    B = np.sum(fsf * d / v, axis=(1, 2))            # s_eu = sum_z line_z B_z
    s_ee = np.zeros((nc, nw))
    s_eu = np.zeros((nc, nw))
    for z0 in range(POST_D):                        # channel by channel: the grids are large
        off, rat = prob["line_shape"] or ([0.], [1.])
        line = 0.
        for dk, rk in zip(off, rat):
            line = line + rk * np.exp(-1. * ((z0 - c) - dk) ** 2 / (2. * w ** 2))
        s_ee += line ** 2 * A[z0]
        s_eu += line * B[z0]
    ro = POST_RA / (1. + POST_RA * s_ee)
    mu = ro * s_eu
    sr = np.sqrt(ro)
    al, be = (POST_MIN_B[0] - mu) / sr, (POST_MAX_B[0] - mu) / sr
    # mass of the box, on the side of the normal where the difference does not cancel
    Z = np.where(al > 0, ndtr(-al) - ndtr(-be), ndtr(be) - ndtr(al))
    with np.errstate(divide="ignore"):
        logp = 0.5 * np.log(ro) + 0.5 * mu ** 2 / ro + np.log(Z)
    p = np.exp(logp - logp.max())
    p /= p.sum()
    Zs = np.where(Z > 0, Z, 1.0)                    # (p is 0 where Z is)
    phi_a, phi_b = np.exp(-0.5 * al ** 2), np.exp(-0.5 * be ** 2)
    k = 1. / math.sqrt(2. * math.pi)
    # first and second moment of N(mu, ro) truncated to the amplitude box
    m1 = mu + sr * k * (phi_a - phi_b) / Zs
    m2 = mu ** 2 + ro + sr * k * ((mu + POST_MIN_B[0]) * phi_a - (mu + POST_MAX_B[0]) * phi_b) / Zs
    cc, ww = np.broadcast_to(c, p.shape), np.broadcast_to(w, p.shape)
    mean = [np.sum(p * m1), np.sum(p * cc), np.sum(p * ww)]
    second = [np.sum(p * m2), np.sum(p * cc ** 2), np.sum(p * ww ** 2)]
    var = [s - m ** 2 for s, m in zip(second, mean)]
    return np.array(mean + var + [np.sum(p[:, w[0] > POST_W_CUT]), np.sum(p[c[:, 0] < POST_C_CUT, :])])


def chain_statistics(chain, exact):
    """The eight POST_STATS of every replica of a kept chain [n, H, W, 3], [16, 8].  Second
    moments are taken about the EXACT mean, so that their expectation is the exact variance
    whatever the chain's autocorrelation (about the replica's own mean they are biased low)."""
    live = chain[:, 1::POST_STEP, 1::POST_STEP, :].reshape(chain.shape[0], -1, 3)
    mean = live.mean(axis=0)
    var = ((live - exact[None, None, :3]) ** 2).mean(axis=0)
    pw = (live[..., 2] > POST_W_CUT).mean(axis=0)
    pc = (live[..., 1] < POST_C_CUT).mean(axis=0)
    return np.concatenate((mean, var, pw[:, None], pc[:, None]), axis=1)


def z_scores(chain, exact):
    """(mean over the 16 replicas - exact) / (their sd / 4): Student's t with 15 degrees of
    freedom for a chain that samples the exact posterior."""
    s = chain_statistics(chain, exact)
    return (s.mean(axis=0) - exact) / (s.std(axis=0, ddof=1) / math.sqrt(s.shape[0]))


def oracle_chain(prob, seed, burn=POST_BURN, keep=POST_KEEP):
    """The oracle's chain at the settings the device tests use: [keep, H, W, 3]."""
    st = O.MHState(prob["data"], prob["var"], prob["mask"], prob["fsf"], None, prob["init"],
                   POST_MIN_B, POST_MAX_B, jump_amplitude=POST_JUMP,
                   gibbs_apriori_variance=POST_RA, seed=seed)
    out = np.empty((keep,) + prob["init"].shape)
    for s in range(1, burn + keep + 1):
        O.mh_sweep(st, s)
        if s > burn:
            out[s - burn - 1] = st.params
    return out


# --------------------------------------------------------------------------------------------- #
# The fixture                                                                                   #
# --------------------------------------------------------------------------------------------- #

def build_fixture():
    """Every array of tests/golden/sampler_reference.npz (needs mpmath)."""
    out = {}
    out["philox_counters"] = np.array([k[0] for k in PHILOX_KAT], dtype=np.uint32)
    out["philox_keys"] = np.array([k[1] for k in PHILOX_KAT], dtype=np.uint32)
    out["philox_words"] = np.array([k[2] for k in PHILOX_KAT], dtype=np.uint32)
    u = uniforms()
    out["u"] = u
    out["regimes"] = np.array([r[:4] for r in INVCDF_REGIMES])
    xs, rems, dens, omax = [], [], [], []
    for lo, hi, mu, sigma, label in INVCDF_REGIMES:
        assert not is_tail(lo, hi, mu, sigma), label
        xo = oracle_draws(lo, hi, mu, sigma, N_EXACT)
        x, rem, den = exact_draws(lo, hi, mu, sigma, u, xo)
        xs.append(x)
        rems.append(rem)
        dens.append(den)
        omax.append(probability_error(xo, x, rem, den).max())
    out["x_star"] = np.array(xs)
    out["x_star_lo"] = np.array(rems)
    out["density"] = np.array(dens)
    out["oracle_max"] = np.array(omax)
    half = (POST_GRID[0] // 2, POST_GRID[1] // 2)
    for kind in POST_KINDS:
        prob = posterior_problem(kind)
        exact = exact_posterior(prob)
        coarse = exact_posterior(prob, half)
        # the error falls like cell^2 (the density does not vanish at w = 4): a third of this is left
        assert np.all(np.abs(exact[:6] - coarse[:6]) < 1e-6), (kind, exact - coarse)
        assert np.all(np.abs(exact[6:] - coarse[6:]) < 1e-4), (kind, exact - coarse)
        out["posterior_" + kind] = exact
    return out


def main():
    np.savez(FIXTURE, **build_fixture())
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
