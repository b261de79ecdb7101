# coding=utf-8
"""
Student-t likelihood of ``Run(robust=...)``: keyword validation, the checkpoint record and the
report.  The reference's likelihood is Gaussian with a known variance (lib/run.py:171-192,
407-426), which single voxels tens of sigma off -- cosmic-ray hits, sky-line residuals, bad
columns -- pull on through every FSF window that holds them.  A Student-t error with ``nu`` degrees
of freedom is that Gaussian with each voxel's variance divided by a latent weight
``lambda_v ~ Gamma(nu/2, rate nu/2)``; the device redraws the weights between sweeps from
``lambda_v | r_v ~ Gamma((nu + 1)/2, rate (nu + r_v^2 / variance_v)/2)`` and the sweep kernels run
on ``variance_v / lambda_v`` (include/deconv3d_hip.h: d3d_robust_*).

``run.likelihoods``, the chi2 map and the window probe of a robust run are those of the conditional
Gaussian under the current weights, not Student-t log densities; ``Run(predictive=True)`` scores the
run by the Student-t marginal instead (deconv3d_amd/predictive.py).
"""
from __future__ import annotations

import numpy as np

from .cube import Cube

KEYS = ("nu", "every", "start")
NU_MAX = 30      # the draw takes (nu + 1) // 2 uniforms (plus a Box-Muller pair for an even nu)


def _integer(name, v, lo, hi=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("robust %s= MUST be an integer, got %r" % (name, v))
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError("robust %s= MUST be %s, got %d"
                         % (name, ">= %d" % lo if hi is None else "from %d to %d" % (lo, hi), v))
    return v


def check_keywords(robust):
    """``robust=`` as ``dict(nu=, every=, start=)``, or None when the keyword is None; ValueError
    otherwise.  An integer is ``nu``; a dict may hold ``nu`` (1 to 30, required), ``every`` (redraw
    after one sweep in how many, default 1) and ``start`` (the first sweep a draw follows, in the
    whole run's numbering, default 0)."""
    if robust is None:
        return None
    if not isinstance(robust, dict):
        robust = dict(nu=robust)
    unknown = sorted(set(robust) - set(KEYS), key=str)
    if unknown:
        raise ValueError("robust= has unknown key(s) %s: any of %s"
                         % (", ".join(repr(k) for k in unknown), ", ".join(KEYS)))
    if "nu" not in robust:
        raise ValueError("robust= needs nu, the degrees of freedom of the Student-t error")
    return dict(nu=_integer("nu", robust["nu"], 1, NU_MAX),
                every=_integer("every", robust.get("every", 1), 1),
                start=_integer("start", robust.get("start", 0), 0))


def check_run(cfg, tempering_cfg):
    """The refusal that needs no device: ``tempering=`` (a rung's ``variance / beta`` under
    reweighting is not a tempered Student-t)."""
    if cfg is not None and tempering_cfg is not None:
        raise ValueError("robust= with tempering=: a rung's variance / beta with Student-t weights "
                         "is not the tempered Student-t likelihood")


def last_due(cfg, sweep):
    """The last sweep <= ``sweep`` (the run's numbering) that a draw follows, or None."""
    if sweep < cfg["start"]:
        return None
    return sweep - (sweep - cfg["start"]) % cfg["every"]


def keyword_record(cfg):
    """``(nu, every, start)`` as the int64 vector a checkpoint's state holds."""
    return np.array([cfg[k] for k in KEYS], dtype=np.int64)


def check_resume(state, files, cfg):
    """ValueError when ``resume_state`` was written with other ``robust=`` values than this run's."""
    saved = "robust_keywords" in files
    if cfg is None and not saved:
        return
    fmt = lambda v: "dict(%s)" % ", ".join("%s=%d" % kv for kv in zip(KEYS, np.ravel(v)))  # noqa: E731
    if cfg is None:
        raise ValueError("resume_state was written with robust=%s; this run has none"
                         % fmt(state["robust_keywords"]))
    if not saved:
        raise ValueError("resume_state was written without robust=; this run asks for robust=%s"
                         % fmt(keyword_record(cfg)))
    old, new = np.asarray(state["robust_keywords"], dtype=np.int64), keyword_record(cfg)
    if old.shape != new.shape or not np.array_equal(old, new):
        raise ValueError("resume_state was written with robust=%s; this run has robust=%s"
                         % (fmt(old), fmt(new)))


class RobustReport(object):
    """
    The weights of a robust run: ``nu``, ``every``, ``start``, ``count`` (draws in the mean),
    ``weight_mean`` (D, H, W) -- the posterior mean of every voxel's weight over the accumulated
    draws, about 1 for a voxel the model explains and ``(nu + 1) / (nu + r^2 / variance)`` for one
    ``r`` off; NaN where the voxel carries no information (NaN voxels) or nothing was accumulated --
    and ``weights``, the last draw.  ``fetch(weights, weight_mean)`` returns ``(weights,
    weight_mean, count)``; the arrays are downloaded on first access and kept.
    """

    def __init__(self, cfg, count, fetch, template=None):
        self.nu, self.every, self.start = cfg["nu"], cfg["every"], cfg["start"]
        self.count = int(count)
        self._fetch = fetch
        self._template = template
        self._cache = {}

    @classmethod
    def from_engine(cls, engine, cfg, template=None):
        """The weights a device context holds now."""
        return cls(cfg, engine.robust_get(False, False)[2], engine.robust_get, template)

    def _get(self, which):
        if which not in self._cache:
            got = self._fetch(which == "weights", which == "weight_mean")
            self._cache[which] = np.asarray(got[0] if which == "weights" else got[1], dtype=np.float64)
        return self._cache[which]

    @property
    def weights(self):
        return self._get("weights")

    @property
    def weight_mean(self):
        mean = self._get("weight_mean")
        return mean if self.count > 0 else np.full(mean.shape, np.nan)

    def downweighted(self, threshold=0.5):
        """0/1 cube (uint8) of the voxels whose mean weight lies below ``threshold``."""
        with np.errstate(invalid="ignore"):
            return (self.weight_mean < threshold).astype(np.uint8)

    def save(self, prefix, clobber=False):
        """``<prefix>_robust_weight_mean.fits`` and ``<prefix>_robust.npz`` (nu, every, start, count,
        weights), beside the files of ``Run.save(prefix)``."""
        t = self._template
        cube = Cube(data=self.weight_mean) if t is None else \
            Cube(data=self.weight_mean, meta=t.meta, x=t.x, y=t.y, z=t.z)
        cube.to_fits("%s_robust_weight_mean.fits" % prefix, clobber)
        np.savez("%s_robust.npz" % prefix, nu=self.nu, every=self.every, start=self.start,
                 count=self.count, weights=self.weights)


def pooled(reports, template=None):
    """The report of several chains' weights: the means pooled by their counts; ``weights`` is
    chain 0's last draw."""
    first = reports[0]
    count = sum(r.count for r in reports)

    def fetch(weights, weight_mean):
        mean = None
        if weight_mean:
            mean = np.zeros(first._get("weight_mean").shape)
            for r in reports:
                if r.count:
                    mean += r._get("weight_mean") * (float(r.count) / count)
            if count == 0:
                mean = first._get("weight_mean")
        return (first.weights if weights else None), mean, count

    return RobustReport(dict(nu=first.nu, every=first.every, start=first.start), count, fetch, template)
