"""
Numpy restatement of the noise scales (include/deconv3d_hip.h: d3d_noise_*; csrc/d3d_noise.hip): the
sums in the device's order, the Marsaglia-Tsang draw operation for operation on the oracle's Philox
arithmetic (tests/robust_oracle.py's array form, here with the counter's tag as an argument), and a
chain that alternates the oracle's sweep with the rescaling.  Test infrastructure only.
"""
import numpy as np

from oracle import deconv3d_oracle as O
from tests.robust_oracle import TWO_PI, _M32, base_ivar  # noqa: F401  (base_ivar: re-exported)

TAG = 0x4E4F4953          # fourth counter word of the scales' streams (the sweep: 0; robust: 0x52425354)
STREAMS = 1024            # d3dh::NOISE_STREAMS
ATTEMPTS = 16             # Marsaglia-Tsang attempts before the fall-back g = d


def philox_pairs(seed, index, sweep, block, tag=TAG):
    """O.philox_pair's two uniforms for the counters (index, sweep, block, tag), for an array of
    indices: O.philox4x32_10's rounds in uint64 arithmetic (tests/robust_oracle.py's, any tag)."""
    c0 = np.asarray(index, dtype=np.uint64) & _M32
    c1 = np.full(c0.shape, int(sweep) & 0xFFFFFFFF, dtype=np.uint64)
    c2 = np.full(c0.shape, int(block) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(c0.shape, int(tag) & 0xFFFFFFFF, dtype=np.uint64)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(O._M0) * c0
        p1 = np.uint64(O._M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & _M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ np.uint64(k0)) & _M32, lo1, (hi0 ^ c3 ^ np.uint64(k1)) & _M32, lo0
        k0 = (k0 + O._W0) & 0xFFFFFFFF
        k1 = (k1 + O._W1) & 0xFFFFFFFF

    def unit(hi, lo):                     # O.u64_to_unit
        u = (hi << np.uint64(32)) | lo
        return ((u >> np.uint64(12)).astype(np.float64) + 0.5) * (1.0 / 4503599627370496.0)

    return unit(c1, c0), unit(c3, c2)


def channel_sums(err, i0, spaxels=None):
    """``(Q_z (D,), N_z (D,))`` in the device's order: stream j of STREAMS adds the counted terms
    (r r) i0 of the spaxels j, j + STREAMS, ... in turn; the partials are then added in index order.
    (A term that is not counted enters as +0.0, which changes no bit of a non-negative sum.)"""
    err, i0 = np.asarray(err, dtype=np.float64), np.asarray(i0, dtype=np.float64)
    D = err.shape[0]
    r, b = err.reshape(D, -1), i0.reshape(D, -1)
    HW = r.shape[1]
    counted = b != 0.0
    if spaxels is not None:
        counted = counted & (np.asarray(spaxels).reshape(-1) != 0)[None, :]
    with np.errstate(invalid="ignore"):
        term = np.where(counted, (r * r) * b, 0.0)
    rounds = (HW + STREAMS - 1) // STREAMS
    padded = np.zeros((D, rounds * STREAMS))
    padded[:, :HW] = term
    padded = padded.reshape(D, rounds, STREAMS)
    part = np.zeros((D, STREAMS))
    for k in range(rounds):
        part = part + padded[:, k, :]
    q = np.zeros(D)
    for j in range(STREAMS):
        q = q + part[:, j]
    return q, counted.sum(axis=1).astype(np.float64)


def group_sums(q_z, n_z, group, G):
    """``(Q_g, N_g)``: the channels of every group in increasing z."""
    q, n = np.zeros(G), np.zeros(G)
    for z, g in enumerate(np.asarray(group)):
        if g >= 0:
            q[g] = q[g] + q_z[z]
            n[g] = n[g] + n_z[z]
    return q, n


def gamma_draw(seed, index, sweep, alpha, tag=TAG):
    """``(g, margin, attempts)``: g ~ Gamma(alpha, 1) by Marsaglia and Tsang for every entry of the
    arrays ``index`` (first counter word) and ``alpha`` (>= 1): attempt t takes block 2t for (u1, u2)
    and the first uniform of block 2t + 1 for u3; no acceptance in ATTEMPTS attempts gives g = d.
    ``margin`` is the smallest |log u3 - bound| and |v| over the attempts made (how far the nearest
    decision was from flipping), ``attempts`` the number made."""
    index = np.asarray(index)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), index.shape)
    d = alpha - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = d.copy()
    open_ = np.ones(index.shape, dtype=bool)
    margin = np.full(index.shape, np.inf)
    attempts = np.zeros(index.shape, dtype=np.int64)
    for t in range(ATTEMPTS):
        if not open_.any():
            break
        u1, u2 = philox_pairs(seed, index, sweep, 2 * t, tag)
        u3, _ = philox_pairs(seed, index, sweep, 2 * t + 1, tag)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
        v1 = 1.0 + c * x
        positive = v1 > 0.0
        v = np.where(positive, v1, 1.0)
        v = v * v * v
        bound = 0.5 * x * x + d - d * v + d * np.log(v)
        accept = positive & (np.log(u3) < bound)
        m = np.where(positive, np.minimum(np.abs(np.log(u3) - bound), np.abs(v1)), np.abs(v1))
        margin = np.where(open_, np.minimum(margin, m), margin)
        attempts = attempts + open_
        g = np.where(open_ & accept, d * v, g)
        open_ = open_ & ~accept
    return g, margin, attempts


def draw_scales(seed, sweep, err, i0, group, spaxels=None, shape=0.0, rate=0.0, G=None, tau_before=None):
    """The draw after sweep ``sweep`` (the run's numbering) from the residual ``err`` and the base
    1/variance ``i0``: a dict of ``tau_g`` (G,), ``scale`` (G,) (NaN where N_g < 2), ``voxels`` = N_g,
    ``sums`` = Q_g, ``tau`` (D,) per channel, and the draw's ``margin``."""
    group = np.asarray(group, dtype=np.int64)
    G = int(group.max()) + 1 if G is None else G
    q, n = group_sums(*channel_sums(err, i0, spaxels), group, G)
    tau_g = np.ones(G) if tau_before is None else np.array(tau_before, dtype=np.float64)
    live = n >= 2.0
    tau_g[~live] = 1.0
    rate_g = rate + 0.5 * q
    margin = np.full(G, np.inf)
    if live.any():
        idx = np.nonzero(live)[0]
        gam, mar, _ = gamma_draw(seed, idx, sweep, shape + 0.5 * n[idx])
        ok = rate_g[idx] != 0.0
        tau_g[idx[ok]] = gam[ok] / rate_g[idx[ok]]
        margin[idx] = mar
    scale = np.where(live, 1.0 / tau_g, np.nan)
    tau = np.where(group >= 0, tau_g[np.maximum(group, 0)], 1.0)
    return dict(tau_g=tau_g, scale=scale, voxels=n, sums=q, tau=tau, margin=margin)


def group_of(per, D):
    """``per='channel' | 'cube'`` as the label vector."""
    return np.arange(D, dtype=np.int64) if per == "channel" else np.zeros(D, dtype=np.int64)


class NoiseChain(object):
    """The oracle's chain (O.MHState, O.mh_sweep) with the rescaling after every due sweep, and the
    series of scales as the device keeps it."""

    def __init__(self, state, group, every=1, start=0, shape=0.0, rate=0.0, spaxels=None):
        self.st, self.every, self.start, self.shape, self.rate = state, every, start, shape, rate
        self.group = np.asarray(group, dtype=np.int64)
        self.G = int(self.group.max()) + 1
        self.spaxels = spaxels
        self.i0 = base_ivar(state.data, state.var)
        self.tau_g = np.ones(self.G)
        self.series, self.sweeps, self.margins = [], [], []

    def rescale(self, sweep):
        got = draw_scales(self.st.seed, sweep, self.st.err, self.i0, self.group, self.spaxels, self.shape,
                          self.rate, self.G, self.tau_g)
        self.tau_g = got["tau_g"]
        ivar = np.where(self.i0 == 0.0, 0.0, self.i0 * got["tau"][:, None, None])
        with np.errstate(divide="ignore"):
            self.st.var = 1.0 / ivar                      # (inf where the voxel carries nothing)
        self.series.append(got["scale"])
        self.sweeps.append(sweep)
        self.margins.append(got["margin"])
        return ivar

    def sweep(self, s):
        O.mh_sweep(self.st, s)
        if s >= self.start and (s - self.start) % self.every == 0:
            self.rescale(s)

    def scale(self):
        return np.array(self.series).reshape(len(self.series), self.G)


# ---- the cases tests/test_gpu_noise.py compares with the device (tests/test_noise_cpu.py checks their
# accept margins, which depend on the seed, the sweep, the group and N_g alone, not on the residual)

FSF5 = np.outer([0.1, 0.2, 0.4, 0.2, 0.1], [0.15, 0.2, 0.3, 0.2, 0.15])
STEP_SEED, STEP_SWEEP = 77, 1
# odd depth and pad channel | a plain one | several blocks | three lane steps per spectrum | more
# spaxels (1147) than streams, and no multiple of them | 5625 spaxels: k_noise_sums' outer loop
# (sp += 4 * STREAMS) takes a second trip, in which every stream adds a fifth spaxel and streams
# 0 .. 504 a sixth (4097 .. 5120 spaxels would only partly fill the trip's first group), at an odd
# depth with its pad channel
STEP_SHAPES = [(13, 5, 7), (32, 6, 5), (21, 30, 24), (300, 4, 4), (6, 37, 31), (5, 75, 75)]
GROUPINGS = ("channel", "cube", "three")


def shape_case(shape, seed=31):
    """A synthetic case of that shape with NaN voxels (one whole spectrum too) and zero variances
    (tests/test_gpu_robust.py's)."""
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


def grouping(name, D):
    """``(group (D,), G)``: every channel its own group; one group; or three groups of which group 1
    is empty, with every fifth channel never rescaled."""
    z = np.arange(D)
    if name == "three":
        return np.where(z % 5 == 0, -1, np.where(z < D // 2, 0, 2)).astype(np.int64), 3
    return group_of(name, D), (D if name == "channel" else 1)


def holes(H, W):
    """A map of counted spaxels with holes: every third spaxel is left out, and one whole row."""
    m = (np.arange(H * W).reshape(H, W) % 3 != 1).astype(np.uint8)
    m[H // 2, :] = 0
    return m


# ---- the recovery case (tests/test_gpu_noise.py) ---------------------------------

RECOVERY_SEED, RECOVERY_ITERATIONS, RECOVERY_BURN_IN, RECOVERY_FACTOR = 7, 400, 100, 4.0


def recovery_inflated(D):
    """The fixed third of the channels whose true noise variance is RECOVERY_FACTOR times the given one."""
    return np.arange(D) % 3 == 1


def recovery_data(data, sigma):
    """``data`` (noise of standard deviation ``sigma`` in it) with independent noise of variance
    (RECOVERY_FACTOR - 1) sigma^2 added on the inflated channels: their variance is then RECOVERY_FACTOR
    times the given sigma^2."""
    rng = np.random.default_rng(4711)
    extra = rng.normal(0., np.sqrt(RECOVERY_FACTOR - 1.0) * sigma, size=data.shape)
    return data + extra * recovery_inflated(data.shape[0])[:, None, None]


def recovery_chain(data, var, mask, fsf, lsf, truth, min_b, max_b, ra):
    """The oracle's run of the recovery case: ``(mean scale per channel over the sweeps from the
    burn-in on, the whole series)``."""
    st = O.MHState(data, var, mask, fsf, lsf, truth, min_b, max_b, 0.1, ra, RECOVERY_SEED)
    chain = NoiseChain(st, group_of("channel", data.shape[0]))
    for s in range(1, RECOVERY_ITERATIONS):
        chain.sweep(s)
    series = chain.scale()
    return series[np.array(chain.sweeps) >= RECOVERY_BURN_IN].mean(axis=0), series


def make_recovery_fixture(path):
    """tests/golden/noise_recovery.npz: tests/test_gpu_run.py: synthetic_cube(32, 12, 12) with the
    oracle's forward model in the device's place, recovery_data's extra noise, and the mean scales of
    recovery_chain on it (20 s)."""
    import deconv3d_amd as d3d
    D, H, W, A0 = 32, 12, 12, 10.0
    inst = d3d.MUSE(fsf_fwhm=0.6)
    rng = np.random.default_rng(12345)
    y, x = np.indices((H, W))
    r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
    truth = np.dstack((A0 * np.exp(-r2 / (2. * (H / 6.) ** 2)),
                       D / 2. + (D / 8.) * np.tanh((x - W / 2.) / (W / 8.)), rng.uniform(1.5, 3.0, size=(H, W))))
    blank = inst.build_cube(np.ones((D, H, W)))
    fsf, lsf = inst.fsf.as_image(blank), inst.lsf.as_vector(blank)
    mask = np.ones((H, W))
    sigma = 0.05 * A0 * fsf.max()
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    data = recovery_data(clean + rng.normal(0., sigma, size=clean.shape), sigma)
    max_b = O.model_max_boundaries(data, fsf)
    mean, _ = recovery_chain(data, np.full(data.shape, sigma ** 2), mask, fsf, lsf, truth,
                             O.model_min_boundaries(), max_b, float(max_b[0] ** 2))
    np.savez(path, data=data, oracle_scale_mean=mean)
