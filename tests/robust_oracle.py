"""
Numpy restatement of the Student-t weights (include/deconv3d_hip.h: d3d_robust_*; csrc/d3d_robust.hip):
the draw, operation for operation, on the oracle's Philox arithmetic (oracle.deconv3d_oracle.
philox4x32_10 / u64_to_unit, here on whole arrays), and a chain that alternates the oracle's sweep
with the reweighting.  Test infrastructure only.
"""
import numpy as np

from oracle import deconv3d_oracle as O

TAG = 0x52425354          # fourth counter word of the weights' streams (the sweep's blocks use 0)
TWO_PI = 6.283185307179586
_M32 = np.uint64(0xFFFFFFFF)


def philox_pairs(seed, voxels, sweep, block):
    """O.philox_pair's two uniforms for the counters (voxel, sweep, block, TAG), for an array of
    voxel indices: O.philox4x32_10's rounds in uint64 arithmetic."""
    c0 = np.asarray(voxels, dtype=np.uint64) & _M32
    c1 = np.full(c0.shape, int(sweep) & 0xFFFFFFFF, dtype=np.uint64)
    c2 = np.full(c0.shape, int(block) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(c0.shape, TAG, dtype=np.uint64)
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


def uniforms(seed, voxels, sweep, count):
    """Uniforms 0 .. count-1 of every voxel's stream: block b yields uniforms 2b and 2b + 1."""
    out = []
    for b in range((count + 1) // 2):
        out.extend(philox_pairs(seed, voxels, sweep, b))
    return out[:count]


def gamma_draw(nu, us):
    """g ~ Gamma((nu + 1) / 2, 1) from the uniforms ``us`` (m = (nu + 1) // 2 of them, two more
    for an even nu): -log of their product taken from the left, plus -log(u_a) cos(2 pi u_b)^2."""
    m = (nu + 1) // 2
    prod = 1.0 * us[0]
    for u in us[1:m]:
        prod = prod * u
    g = -np.log(prod)
    if nu % 2 == 0:
        t = np.cos(TWO_PI * us[m + 1])
        g = g + (-np.log(us[m])) * (t * t)
    return g


def n_uniforms(nu):
    return (nu + 1) // 2 + (2 if nu % 2 == 0 else 0)


def base_ivar(data, var):
    """d3d_set_data's 1/variance: zero variances are 1e12, NaN voxels carry nothing."""
    var = np.where(np.asarray(var, dtype=np.float64) == 0.0, 1e12, var)
    return np.where(np.isnan(data) | np.isnan(var), 0.0, 1.0 / var)


def draw_weights(seed, sweep, nu, err, i0):
    """lambda (D,H,W) of the draw after sweep ``sweep`` (the run's numbering) from the residual
    ``err`` and the base 1/variance ``i0``; voxel = z H W + y W + x."""
    err = np.asarray(err, dtype=np.float64)
    voxels = np.arange(err.size, dtype=np.uint64).reshape(err.shape)
    g = gamma_draw(nu, uniforms(seed, voxels, sweep, n_uniforms(nu)))
    return (2.0 * g) / (float(nu) + (err * err) * i0)


class RobustChain(object):
    """The oracle's chain (O.MHState, O.mh_sweep) with the reweighting after every due sweep, and
    the running mean of the weights as the device keeps it."""

    def __init__(self, state, nu, every=1, start=0, accumulate_from=0):
        self.st, self.nu, self.every, self.start, self.accumulate_from = state, nu, every, start, accumulate_from
        self.i0 = base_ivar(state.data, state.var)
        self.weights = np.ones(self.i0.shape)
        self.mean = np.zeros(self.i0.shape)
        self.count = 0

    def reweight(self, sweep):
        lam = draw_weights(self.st.seed, sweep, self.nu, self.st.err, self.i0)
        ivar = np.where(self.i0 == 0.0, 0.0, lam * self.i0)
        with np.errstate(divide="ignore"):
            self.st.var = 1.0 / ivar                      # (inf where the voxel carries nothing)
        self.weights = lam
        if sweep >= self.accumulate_from:
            self.count += 1
            self.mean = np.where(self.i0 == 0.0, 0.0, self.mean + (lam - self.mean) / float(self.count))
        return ivar

    def sweep(self, s):
        O.mh_sweep(self.st, s)
        if s >= self.start and (s - self.start) % self.every == 0:
            self.reweight(s)

    def weight_mean(self):
        return np.where(self.i0 == 0.0, np.nan, self.mean)
