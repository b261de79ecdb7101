# coding=utf-8
"""
Noise-scale inference of ``Run(noise=...)``: keyword validation, the checkpoint record and the
report.  The reference takes the variance as known (lib/run.py:171-200: the given cube, or one
constant from a corner of the data) and divides every chi2 by it (lib/run.py:407-426); variance
cubes of instrument pipelines are often low by tens of per cent, and wrong channel by channel under
sky lines.  Here the variance of every voxel of a group ``g`` of channels is ``s_g variance_v`` with
``s_g ~ InvGamma(shape, rate)`` (0, 0: Jeffreys' ``1/s``); between sweeps the device redraws
``1/s_g ~ Gamma(shape + N_g/2, rate rate + Q_g/2)``, ``N_g`` the counted voxels of the group and
``Q_g`` the sum of their ``r^2 / variance`` -- an exact Gibbs step -- and the sweep kernels run on the
rescaled variance (include/deconv3d_hip.h: d3d_noise_*).

``run.likelihoods`` and the chi2 map of such a run are those of the conditional Gaussian under the
current scales.
"""
from __future__ import annotations

import numpy as np

KEYS = ("per", "every", "start", "shape", "rate", "spaxels")


def _integer(name, v, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("noise %s= MUST be an integer, got %r" % (name, v))
    if int(v) < lo:
        raise ValueError("noise %s= MUST be >= %d, got %d" % (name, lo, int(v)))
    return int(v)


def _real(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not np.isfinite(v) or v < 0:
        raise ValueError("noise %s= MUST be a finite number >= 0, got %r" % (name, v))
    return float(v)


def check_keywords(noise):
    """``noise=`` as ``dict(per=, every=, start=, shape=, rate=, spaxels=)``, or None when the keyword
    is None or False; ValueError otherwise.  ``True`` is ``dict()``.  ``per`` is ``'channel'`` (the
    default: every channel its own scale), ``'cube'`` (one scale) or a vector of D integer labels
    (-1: the channel is never rescaled; the groups are 0 .. max); ``every`` (redraw after one sweep in
    how many, default 1) and ``start`` (the first sweep a draw follows, the whole run's numbering,
    default 0); ``shape`` and ``rate`` of the inverse-gamma prior (default 0, 0); ``spaxels`` the
    spaxels whose voxels are counted: ``'all'`` (default, masked ones too), ``'unmasked'`` or an
    (H, W) 0/1 map.  Shapes are checked by `resolve`."""
    if noise is None or noise is False:
        return None
    if noise is True:
        noise = {}
    if not isinstance(noise, dict):
        raise ValueError("noise= MUST be True or a dict of %s, got %r" % (", ".join(KEYS), noise))
    unknown = sorted(set(noise) - set(KEYS), key=str)
    if unknown:
        raise ValueError("noise= has unknown key(s) %s: any of %s"
                         % (", ".join(repr(k) for k in unknown), ", ".join(KEYS)))
    per = noise.get("per", "channel")
    if isinstance(per, str):
        if per not in ("channel", "cube"):
            raise ValueError("noise per= MUST be 'channel', 'cube' or a vector of integer labels, got %r" % per)
    else:
        labels = np.asarray(per)
        if labels.ndim != 1 or labels.size == 0 or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError("noise per= MUST be 'channel', 'cube' or a vector of integer labels, got an "
                             "array of shape %s and type %s" % (labels.shape, labels.dtype))
        if labels.min() < -1:
            raise ValueError("noise per=: a label is -1 (never rescaled) or >= 0, got %d" % labels.min())
        if labels.max() < 0:
            raise ValueError("noise per=: no channel has a group (every label is -1)")
        per = labels.astype(np.int64)
    spaxels = noise.get("spaxels", "all")
    if isinstance(spaxels, str):
        if spaxels not in ("all", "unmasked"):
            raise ValueError("noise spaxels= MUST be 'all', 'unmasked' or an (H, W) 0/1 map, got %r" % spaxels)
    else:
        spaxels = np.asarray(spaxels)
        if spaxels.ndim != 2 or not np.isin(spaxels, (0, 1)).all():
            raise ValueError("noise spaxels= MUST be 'all', 'unmasked' or an (H, W) map of 0 and 1")
        spaxels = spaxels.astype(np.uint8)
    return dict(per=per, every=_integer("every", noise.get("every", 1), 1),
                start=_integer("start", noise.get("start", 0), 0),
                shape=_real("shape", noise.get("shape", 0.)), rate=_real("rate", noise.get("rate", 0.)),
                spaxels=spaxels)


def check_run(cfg, tempering_cfg, robust_cfg, predictive_cfg):
    """The refusals that need no device: ``robust=``, ``predictive=`` and ``tempering=``."""
    if cfg is None:
        return
    if robust_cfg is not None:
        raise ValueError("noise= with robust=: both rewrite 1/variance from the base cube; composing them "
                         "needs the weights' draw to read the scales and the sums to carry the weights "
                         "(not built)")
    if predictive_cfg is not None:
        raise ValueError("noise= with predictive=: the density's normaliser 1/2 log(1/variance) is added at "
                         "extraction and would have to enter every sample once the variance is drawn")
    if tempering_cfg is not None:
        raise ValueError("noise= with tempering=: a rung's variance / beta is not rescaled with the scales "
                         "of rung 0, and the exchange's energies assume one variance")


def resolve(cfg, depth, mask):
    """The keyword against the cube: ``cfg`` with ``group`` (D,) int32, ``G`` and ``map`` ((H, W) uint8,
    or None for every spaxel); ValueError on a shape that does not fit."""
    per = cfg["per"]
    if isinstance(per, str):
        group = np.arange(depth) if per == "channel" else np.zeros(depth)
    else:
        if per.shape != (depth,):
            raise ValueError("noise per= has %d labels, the cube has %d channels" % (per.size, depth))
        group = per
    group = np.ascontiguousarray(group, dtype=np.int32)
    spaxels = cfg["spaxels"]
    if isinstance(spaxels, str):
        smap = None if spaxels == "all" else (np.asarray(mask) == 1).astype(np.uint8)
    else:
        if spaxels.shape != np.shape(mask):
            raise ValueError("noise spaxels= has shape %s, the cube's spaxels %s" % (spaxels.shape, np.shape(mask)))
        smap = spaxels
    return dict(cfg, group=group, G=int(group.max()) + 1, map=smap)


def capacity(cfg, max_iterations, sweep_origin=0):
    """Rows the series needs: the due sweeps among ``sweep_origin + 1 .. sweep_origin + max_iterations
    - 1``, one more for the draw a resumed run re-makes, at least 1."""
    first, last = sweep_origin + 1, sweep_origin + max_iterations - 1
    lo = max(first, cfg["start"])
    lo += (cfg["start"] - lo) % cfg["every"]
    due = 0 if lo > last else (last - lo) // cfg["every"] + 1
    return due + 1


def last_due(cfg, sweep):
    """The last sweep <= ``sweep`` (the run's numbering) that a draw follows, or None."""
    if sweep < cfg["start"]:
        return None
    return sweep - (sweep - cfg["start"]) % cfg["every"]


def keyword_record(cfg):
    """What a checkpoint's state holds of a resolved keyword: ``noise_keywords`` = (every, start,
    shape, rate, G) as float64, ``noise_group`` (D,) int32 and ``noise_spaxels`` (H, W) uint8 (empty:
    every spaxel)."""
    return dict(noise_keywords=np.array([cfg["every"], cfg["start"], cfg["shape"], cfg["rate"], cfg["G"]],
                                        dtype=np.float64),
                noise_group=np.asarray(cfg["group"], dtype=np.int32),
                noise_spaxels=np.zeros((0, 0), dtype=np.uint8) if cfg["map"] is None else cfg["map"])


def check_resume(state, files, cfg):
    """ValueError when ``resume_state`` was written with other ``noise=`` values than this run's."""
    saved = "noise_keywords" in files
    if cfg is None and not saved:
        return
    if cfg is None:
        raise ValueError("resume_state was written with noise=; this run has none")
    if not saved:
        raise ValueError("resume_state was written without noise=; this run asks for it")
    new = keyword_record(cfg)
    for key, what in (("noise_keywords", "every, start, shape, rate or number of groups"),
                      ("noise_group", "channel groups (per=)"), ("noise_spaxels", "counted spaxels")):
        old = np.asarray(state[key])
        if old.shape != new[key].shape or not np.array_equal(old, new[key]):
            raise ValueError("resume_state was written with noise= of other %s than this run's" % what)


class NoiseReport(object):
    """
    The scales of a ``noise=`` run: ``scale`` (n, G), the draws ``s_g`` of every group (NaN for a
    group of fewer than 2 counted voxels), ``sweeps`` (n,) the sweep each followed, ``groups`` (D,) the
    label of every channel, ``voxels`` (G,) the counted voxels ``N_g``, ``count`` = n.  ``scale_mean``,
    ``scale_std`` and ``quantiles(q)`` cover the draws of the sweeps from ``burn_in`` on (all when it
    is None).  ``channel_scale`` (D,) is ``scale_mean`` per channel, NaN where the channel is not
    scaled; ``variance(given)`` the given variance times it.  ``fetch()`` returns ``(scale, sweeps,
    voxels, last_sum, tau)``; it is called on first access and the arrays are kept.
    """

    def __init__(self, cfg, fetch, burn_in=None, first_sweep=0):
        self.every, self.start, self.shape, self.rate = cfg["every"], cfg["start"], cfg["shape"], cfg["rate"]
        self.groups = np.asarray(cfg["group"], dtype=np.int64)
        self.n_groups = int(cfg["G"])
        self.burn_in = burn_in
        self._first_sweep = first_sweep     # (a resumed run's re-made draw lies before it: not reported)
        self._fetch = fetch
        self._got = None

    @classmethod
    def from_engine(cls, engine, cfg, burn_in=None, first_sweep=0):
        """The scales a device context holds now."""
        return cls(cfg, engine.noise_get, burn_in, first_sweep)

    def _get(self):
        if self._got is None:
            scale, sweeps, voxels, last_sum, tau = self._fetch()
            keep = np.asarray(sweeps) >= self._first_sweep
            self._got = dict(scale=np.asarray(scale, dtype=np.float64).reshape(-1, self.n_groups)[keep],
                             sweeps=np.asarray(sweeps, dtype=np.int64)[keep],
                             voxels=np.asarray(voxels, dtype=np.float64),
                             last_sum=np.asarray(last_sum, dtype=np.float64), tau=np.asarray(tau, dtype=np.float64))
        return self._got

    scale = property(lambda self: self._get()["scale"])
    sweeps = property(lambda self: self._get()["sweeps"])
    voxels = property(lambda self: self._get()["voxels"])
    last_sum = property(lambda self: self._get()["last_sum"])
    count = property(lambda self: len(self._get()["sweeps"]))

    def _kept(self):
        got = self._get()
        return got["scale"] if self.burn_in is None else got["scale"][got["sweeps"] >= self.burn_in]

    @property
    def scale_mean(self):
        kept = self._kept()
        return kept.mean(axis=0) if len(kept) else np.full(self.n_groups, np.nan)

    @property
    def scale_std(self):
        kept = self._kept()
        return kept.std(axis=0, ddof=1) if len(kept) > 1 else np.full(self.n_groups, np.nan)

    def quantiles(self, q):
        """Quantiles ``q`` of every group's kept draws, shape ``np.shape(q) + (G,)``."""
        kept = self._kept()
        if not len(kept):
            return np.full(np.shape(q) + (self.n_groups,), np.nan)
        return np.quantile(kept, q, axis=0)

    @property
    def channel_scale(self):
        mean = self.scale_mean
        return np.where(self.groups >= 0, mean[np.maximum(self.groups, 0)], np.nan)

    def variance(self, given):
        """The given variance (a (D, H, W) cube or a constant) times ``channel_scale``, times 1 where
        that is NaN."""
        factor = np.where(np.isnan(self.channel_scale), 1., self.channel_scale)
        return np.asarray(given, dtype=np.float64) * factor[:, None, None]

    def save(self, prefix):
        """``<prefix>_noise.npz``: scale, sweeps, groups, voxels, scale_mean, scale_std,
        channel_scale and the keywords."""
        np.savez("%s_noise.npz" % prefix, scale=self.scale, sweeps=self.sweeps, groups=self.groups,
                 voxels=self.voxels, scale_mean=self.scale_mean, scale_std=self.scale_std,
                 channel_scale=self.channel_scale, every=self.every, start=self.start, shape=self.shape,
                 rate=self.rate, burn_in=-1 if self.burn_in is None else self.burn_in)


def pooled(reports):
    """The report of several chains: their series one after the other (``sweeps`` too); ``voxels``
    is chain 0's (the counted set is the same for all)."""
    first = reports[0]

    def fetch():
        return (np.concatenate([r.scale for r in reports]), np.concatenate([r.sweeps for r in reports]),
                first.voxels, first.last_sum, first._get()["tau"])

    cfg = dict(every=first.every, start=first.start, shape=first.shape, rate=first.rate, group=first.groups,
               G=first.n_groups)
    return NoiseReport(cfg, fetch, first.burn_in, first._first_sweep)
