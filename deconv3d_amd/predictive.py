# coding=utf-8
"""
Pointwise predictive accuracy of a run: ``Run(predictive=True)``.

The reference scores one state of the chain (its chi2, lib/run.py:407-426); that says neither which
of two models of one cube the data prefer nor where in the field a model fails.  The standard answer
is the pointwise predictive density over the posterior samples ``s``: for every voxel ``v``

    lppd_v = log mean_s p(y_v | theta_s)        p_v = var_s log p(y_v | theta_s)

``elpd = sum_v (lppd_v - p_v)`` estimates the expected log predictive density of new data and
``WAIC = -2 elpd``; the pointwise values also give the standard error of a difference between two
runs.  The device folds every sample of the posterior moments into four accumulator cubes between
the sweeps (include/deconv3d_hip.h: d3d_pred_*); this module holds the host
side: keyword validation, the lazily downloaded maps and cubes, the exact pooling of several chains'
accumulators and the comparison of two runs (pure numpy).

The likelihood is the run's: Gaussian, or with ``robust=`` the Student-t marginal (the weight
integrated out) on the base variance -- so runs that differ in ``nu`` compare.
"""
from __future__ import annotations

import math

import numpy as np


def check_keyword(predictive, burn_in):
    """``Run``'s ``predictive=``: None / False (off: returns None), True or a dict (no key is known
    yet); returns ``dict()``.  Needs ``posterior_burn_in`` (ValueError)."""
    if predictive is None or predictive is False:
        return None
    if predictive is not True:
        if not isinstance(predictive, dict):
            raise ValueError("predictive= MUST be None, True or a dict(), got %r" % (predictive,))
        if predictive:
            raise ValueError("predictive=: unknown key(s) %s (none is defined yet)"
                             % sorted(predictive, key=str))
    if burn_in is None:
        raise ValueError("predictive= needs posterior_burn_in=: the predictive density is averaged "
                         "over the samples the posterior moments take")
    return dict()


def base_ivar(data, variance):
    """The base 1/variance d3d_set_data derives: 0 where the datum or the variance is NaN, 1e-12
    where the variance is 0.  A voxel counts iff this is not 0."""
    data, variance = np.asarray(data, dtype=np.float64), np.asarray(variance, dtype=np.float64)
    v = np.where(variance == 0., 1e12, variance)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isnan(data) | np.isnan(v), 0., 1. / v)


def log_norm(nu=0):
    """The part of ``k_v`` no voxel changes: ``-1/2 log(2 pi)`` (``nu`` 0: Gaussian) or
    ``lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi)``; ``k_v`` adds ``1/2 log(i0_v)``."""
    if not nu:
        return -0.5 * math.log(2. * math.pi)
    nu = float(nu)
    return math.lgamma(0.5 * (nu + 1.)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)


def merge(parts):
    """The accumulators ``(n, M, S, mean, M2)`` of disjoint blocks of samples into those of their
    union, exactly: ``M = max M_r``, ``S = sum_r S_r exp(M_r - M)`` (blocks in the order given) and
    Chan's merge of ``(mean, M2)`` block after block.  A block with n == 0 contributes nothing."""
    parts = [(int(p[0]),) + tuple(np.asarray(a, dtype=np.float64) for a in p[1:]) for p in parts]
    if not parts:
        raise ValueError("no accumulators to merge")
    if len(set(a.shape for p in parts for a in p[1:])) != 1:
        raise ValueError("accumulators of different shapes")
    live = [p for p in parts if p[0] > 0]
    if not live:
        return parts[0]
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


def extract(n, M, S, m2, i0, nu=0):
    """``(lppd_v, p_v)`` cubes from the accumulators of ``n`` samples: ``lppd = (k + M) + log(S / n)``
    with ``k = 1/2 log(i0) + log_norm(nu)`` and ``p = M2 / (n - 1)`` (NaN for n < 2); NaN where
    ``i0 == 0``.  The device's expression (k_pred_maps), operation for operation."""
    i0 = np.asarray(i0, dtype=np.float64)
    counted = i0 != 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        k = 0.5 * np.log(i0) + log_norm(nu)
        lppd = (k + M) + np.log(S / float(n))
        p = np.full(i0.shape, np.nan) if n < 2 else m2 / (float(n) - 1.)
    return np.where(counted, lppd, np.nan), np.where(counted, p, np.nan)


def fold_maps(lppd, p):
    """(H, W, 4) of the device's map: sums over the counted voxels of every spaxel of ``lppd_v``,
    ``p_v``, 1 and ``(lppd_v - p_v)^2``, in the device's order -- lane l of 64 takes the channel pairs
    l, l + 64, ... (the even channel first), then the lanes fold by halves."""
    D, H, W = lppd.shape
    counted = ~np.isnan(lppd)
    terms = (lppd, p, np.ones(lppd.shape), (lppd - p) * (lppd - p))
    lanes = np.zeros((4, 64, H, W))
    for z in range(D):
        lane = (z // 2) % 64
        for t in range(4):
            lanes[t, lane] = np.where(counted[z], lanes[t, lane] + terms[t][z], lanes[t, lane])
    width = 32
    while width:
        lanes = lanes[:, :width] + lanes[:, width:2 * width]
        width //= 2
    return np.ascontiguousarray(np.moveaxis(lanes[:, 0], 0, -1))


class PredictiveAccuracy(object):
    """
    The predictive accuracy of ``count`` posterior samples.  Per spaxel, (H, W): ``lppd_map``,
    ``p_waic_map``, ``elpd_map = lppd_map - p_waic_map`` and ``voxels`` (the counted voxels: every
    voxel with a finite datum and variance, at masked spaxels too).  Scalars: ``lppd``, ``p_waic``,
    ``elpd``, ``waic = -2 elpd`` and ``se``, the standard error ``sqrt(N var_v(elpd_v))`` of ``elpd``
    over the N counted voxels.  Per voxel, (D, H, W) with NaN where not counted: ``lppd_cube``,
    ``p_waic_cube``.  ``p_waic`` needs two samples (NaN below).  ``compare(other)`` scores this run
    against another of the same data.  ``nu``: 0 for the Gaussian likelihood, else the Student-t's
    degrees of freedom.  Device results are fetched on first access and kept:
    ``maps()`` returns the (H, W, 4) sums, ``cubes(lppd, p_waic)`` the two cubes (None for one not
    asked for), ``raw()`` the accumulators ``(M, S, mean, M2)`` of :func:`merge`.
    """

    def __init__(self, count, maps, cubes, raw=None, nu=0):
        self.count = int(count)
        self.nu = int(nu)
        self._maps, self._cubes, self._raw = maps, cubes, raw
        self._cache = {}

    @classmethod
    def from_engine(cls, engine, nu=0):
        """What a device context holds now."""
        return cls(engine.pred_count(), engine.pred_maps, engine.pred_cubes, engine.pred_get, nu)

    @classmethod
    def from_accumulators(cls, count, M, S, mean, m2, i0, nu=0):
        """Extracted on the host (pooled chains)."""
        def cubes(lppd=True, p_waic=True):
            return extract(count, M, S, m2, i0, nu)

        return cls(count, lambda: fold_maps(*cubes()), cubes, lambda: (M, S, mean, m2), nu)

    def _get(self, what):
        if what not in self._cache:
            if what == "maps":
                self._cache[what] = np.asarray(self._maps(), dtype=np.float64)
            elif what == "raw":
                self._cache[what] = tuple(self._raw())
            else:
                got = self._cubes(what == "lppd", what == "p_waic")
                self._cache[what] = np.asarray(got[0] if what == "lppd" else got[1], dtype=np.float64)
        return self._cache[what]

    def accumulators(self):
        """``(count, M, S, mean, M2)`` as :func:`merge` takes them."""
        return (self.count,) + self._get("raw")

    lppd_map = property(lambda self: self._get("maps")[..., 0])
    p_waic_map = property(lambda self: self._get("maps")[..., 1])
    elpd_map = property(lambda self: self.lppd_map - self.p_waic_map)
    voxels = property(lambda self: self._get("maps")[..., 2].astype(np.int64))
    lppd_cube = property(lambda self: self._get("lppd"))
    p_waic_cube = property(lambda self: self._get("p_waic"))
    lppd = property(lambda self: float(np.sum(self.lppd_map)))
    p_waic = property(lambda self: float(np.sum(self.p_waic_map)))
    elpd = property(lambda self: self.lppd - self.p_waic)
    waic = property(lambda self: -2. * self.elpd)

    @property
    def se(self):
        n = float(np.sum(self._get("maps")[..., 2]))
        if n < 2:
            return float("nan")
        total, squares = self.elpd, float(np.sum(self._get("maps")[..., 3]))
        return math.sqrt(n * max(squares - total * total / n, 0.) / (n - 1.)) if total == total else float("nan")

    def compare(self, other):
        """``(delta_elpd, se_delta)``: this run's elpd minus ``other``'s (positive: the data prefer
        this one) and the standard error ``sqrt(N var_v(d_v))`` of the sum of the pointwise
        differences ``d_v``.  ValueError unless both count the same voxels of one shape."""
        mine = self.lppd_cube - self.p_waic_cube
        theirs = other.lppd_cube - other.p_waic_cube
        if mine.shape != theirs.shape:
            raise ValueError("compare(): cubes of different shapes, %s and %s" % (mine.shape, theirs.shape))
        counted = ~np.isnan(self.lppd_cube)
        if not np.array_equal(counted, ~np.isnan(other.lppd_cube)):
            raise ValueError("compare(): the two runs count different voxels (another datum or variance is NaN)")
        d = (mine - theirs)[counted]
        if d.size < 2:
            return float(np.sum(d)), float("nan")
        return float(np.sum(d)), float(np.sqrt(d.size * np.var(d, ddof=1)))

    def save(self, prefix):
        """``<prefix>_posterior_predictive.npz``: count, nu, the maps, the scalars and the cubes."""
        np.savez("%s_posterior_predictive.npz" % prefix, count=self.count, nu=self.nu,
                 lppd_map=self.lppd_map, p_waic_map=self.p_waic_map, elpd_map=self.elpd_map,
                 voxels=self.voxels, lppd=self.lppd, p_waic=self.p_waic, elpd=self.elpd, waic=self.waic,
                 se=self.se, lppd_cube=self.lppd_cube, p_waic_cube=self.p_waic_cube)


def pooled(parts, i0):
    """The PredictiveAccuracy of several chains' samples together (``chains=R``): their accumulators
    merged exactly (:func:`merge`), extracted on the host with the base 1/variance ``i0``."""
    parts = list(parts)
    count, nu = sum(p.count for p in parts), parts[0].nu
    kept = []

    def raw():             # (the chains' cubes are downloaded on first access, once)
        if not kept:
            kept.append(merge([p.accumulators() for p in parts])[1:])
        return kept[0]

    def cubes(lppd=True, p_waic=True):
        M, S, _, m2 = raw()
        return extract(count, M, S, m2, i0, nu)

    return PredictiveAccuracy(count, lambda: fold_maps(*cubes()), cubes, raw, nu)
