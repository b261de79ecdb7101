"""
Numpy restatement of the pointwise predictive accuracy (include/deconv3d_hip.h: d3d_pred_*;
csrc/d3d_pred.hip; deconv3d_amd/predictive.py): both densities, the streaming update, the extraction,
the device's fold of a spectrum and the pooling of chains, operation for operation in fp64 -- and the
same quantities evaluated directly in extended precision, which is what the streaming forms are
judged against.  Test infrastructure only.
"""
import math

import numpy as np

from oracle import deconv3d_oracle as O


def base_ivar(data, var):
    """What d3d_set_data leaves in SLOT_IVAR: 1/var, 1e-12 for a zero variance, 0 for a NaN voxel."""
    v = np.where(var == 0., 1e12, var)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(data) | np.isnan(v), 0., 1. / v)


def q_of(err, i0, nu=0):
    """The chain-varying part of the log density: Gaussian (nu 0) -1/2 (r r) i0; Student-t marginal
    -((nu + 1)/2) log1p((r r) i0 / nu)."""
    x = (err * err) * i0
    if not nu:
        return -0.5 * x
    return -((0.5 * (float(nu) + 1.)) * np.log1p(x / float(nu)))


def log_norm(nu=0):
    if not nu:
        return -0.5 * math.log(2. * math.pi)
    nu = float(nu)
    return math.lgamma(0.5 * (nu + 1.)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)


def log_density(err, i0, nu=0):
    """log p(y_v | theta) of one state, NaN where the voxel is not counted."""
    with np.errstate(divide="ignore"):
        k = 0.5 * np.log(i0) + log_norm(nu)
    return np.where(i0 != 0., k + q_of(err, i0, nu), np.nan)


class Accum(object):
    """The four accumulators of k_pred_accum over arrays of one shape."""

    def __init__(self, shape):
        self.n = 0
        self.M, self.S = np.zeros(shape), np.zeros(shape)
        self.mean, self.m2 = np.zeros(shape), np.zeros(shape)

    def add(self, q, counted=None):
        """One sample: d = q - M; e = exp(-|d|); S = d <= 0 ? S + e : S e + 1; M = d <= 0 ? M : q (the
        first sample: M = q, S = 1); Welford's step.  Voxels outside ``counted`` keep their zeros."""
        q = np.asarray(q, dtype=np.float64)
        counted = np.ones(q.shape, dtype=bool) if counted is None else counted
        self.n += 1
        n = float(self.n)
        if self.n == 1:
            M, S = q, np.ones(q.shape)
        else:
            d = q - self.M
            e = np.exp(-np.abs(d))
            S = np.where(d <= 0., self.S + e, self.S * e + 1.)
            M = np.where(d <= 0., self.M, q)
        delta = q - self.mean
        mean = self.mean + delta / n
        m2 = self.m2 + delta * (q - mean)
        self.M, self.S = np.where(counted, M, self.M), np.where(counted, S, self.S)
        self.mean, self.m2 = np.where(counted, mean, self.mean), np.where(counted, m2, self.m2)
        return self

    def parts(self):
        return self.n, self.M, self.S, self.mean, self.m2


def accumulate(qs, counted=None):
    acc = Accum(np.shape(qs[0]))
    for q in qs:
        acc.add(q, counted)
    return acc


def merge(parts):
    """(n, M, S, mean, M2) of disjoint blocks into their union's: M = max M_r, S = sum S_r exp(M_r -
    M) in the order given, Chan's merge of (mean, M2) block after block."""
    live = [p for p in parts if p[0] > 0]
    M = live[0][1]
    for p in live[1:]:
        M = np.maximum(M, p[1])
    S = np.zeros_like(M)
    for p in live:
        S = S + p[2] * np.exp(p[1] - M)
    n, mean, m2 = live[0][0], live[0][3], live[0][4]
    for p in live[1:]:
        nb, total = p[0], n + p[0]
        delta = p[3] - mean
        mean = mean + delta * (float(nb) / total)
        m2 = m2 + p[4] + delta * delta * (float(n) * nb / total)
        n = total
    return n, M, S, mean, m2


def direct(qs):
    """(M, S, mean, M2) of the samples evaluated directly in extended precision (two passes)."""
    qs = np.asarray(qs, dtype=np.longdouble)
    M = qs.max(axis=0)
    S = np.exp(qs - M).sum(axis=0)
    mean = qs.mean(axis=0)
    m2 = ((qs - mean) ** 2).sum(axis=0)
    return M, S, mean, m2


def extract(n, M, S, m2, i0, nu=0):
    """(lppd_v, p_v): lppd = (k + M) + log(S / n), k = 1/2 log(i0) + log_norm(nu); p = M2 / (n - 1),
    NaN below two samples; NaN where i0 == 0."""
    counted = i0 != 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        k = 0.5 * np.log(i0) + log_norm(nu)
        lppd = (k + M) + np.log(S / float(n))
        p = np.full(np.shape(i0), np.nan) if n < 2 else m2 / (float(n) - 1.)
    return np.where(counted, lppd, np.nan), np.where(counted, p, np.nan)


def fold_maps(lppd, p):
    """k_pred_maps: per spaxel the sums over its counted voxels of lppd_v, p_v, 1 and (lppd_v - p_v)^2;
    lane l of 64 takes the channel pairs l, l + 64, ... (even channel first), then the lanes fold by
    halves (32, 16, .. 1)."""
    D, H, W = lppd.shape
    counted = ~np.isnan(lppd)
    e = lppd - p
    terms = (lppd, p, np.ones(lppd.shape), e * e)
    out = np.zeros((H, W, 4))
    for t in range(4):
        lanes = np.zeros((64, H, W))
        for z in range(D):
            lane = (z // 2) % 64
            lanes[lane] = np.where(counted[z], lanes[lane] + terms[t][z], lanes[lane])
        width = 32
        while width:
            lanes = lanes[:width] + lanes[width:2 * width]
            width //= 2
        out[..., t] = lanes[0]
    return out


def scalars(maps):
    """lppd, p_waic, elpd, se = sqrt(N var_v(elpd_v)) from the map's sums."""
    lppd, p, n, sq = (float(np.sum(maps[..., k])) for k in range(4))
    elpd = lppd - p
    return lppd, p, elpd, math.sqrt(n * (sq - elpd * elpd / n) / (n - 1.))


def compare(lppd_a, p_a, lppd_b, p_b):
    """(delta elpd, its standard error) of a against b from the pointwise differences."""
    counted = ~np.isnan(lppd_a)
    d = ((lppd_a - p_a) - (lppd_b - p_b))[counted]
    return float(d.sum()), float(np.sqrt(d.size * d.var(ddof=1)))


def residual(data, params, mask, fsf, lsf):
    """The device's residual of a state: NaN voxels hold 0 data (they are not counted)."""
    return O.compute_error_in_one_step(np.where(np.isnan(data), 0., data), params, mask, fsf, lsf)
