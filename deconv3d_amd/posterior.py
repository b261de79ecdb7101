# coding=utf-8
"""
Posterior moments of a run: mean and standard deviation of the SAMPLES' clean cube,
LSF (x) FSF convolved cube, parameters and integrated flux, accumulated on the device while
the chain runs (include/deconv3d_hip.h: d3d_post_*; ``Run(posterior_burn_in=...)``).

The reference's estimator is the mean of the saved parameter chain and the cubes of that mean
map (lib/run.py:581-593, 597-652).  Where the per-spaxel parameters are not identified --
neighbours trade flux through the FSF -- every sample fits the data while the cubes of the mean
map do not; the estimator that is right there is the mean of the cubes.  This module holds the
host side: lazily downloaded moments, their standard deviations, and the pooling of several
chains' moments (pure numpy).

The per-spaxel ``(a, c, w, F)`` are heavy-tailed, so mean and standard deviation summarise them
badly; :class:`PosteriorHistograms` reads medians, intervals and modes off the per-spaxel
histograms the device keeps beside the moments (d3d_hist_*; ``Run(posterior_histograms=...)``).
"""
from __future__ import annotations

import numpy as np

from .cube import Cube

PARAMETERS, CLEAN, CONVOLVED = 0, 1, 2


def _merge(a, b):
    """Chan, Golub & LeVeque's combination of two (n, mean, M2) triples."""
    na, ma, sa = a
    nb, mb, sb = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    delta = mb - ma
    return n, ma + delta * (float(nb) / n), sa + sb + delta * delta * (float(na) * nb / n)


def pool(moments):
    """Combine ``(n, mean, M2)`` triples -- sample count, mean and sum of squared deviations
    of disjoint blocks of samples -- into the triple of their union, pairwise (a balanced
    tree of Chan's two-block formula).  Blocks with n == 0 contribute nothing (their arrays
    are not read); a block with n == 1 has M2 == 0.  The sample variance is M2 / (n - 1)."""
    blocks = []
    for n, mean, m2 in moments:
        n = int(n)
        if n < 0:
            raise ValueError("a block of %d samples" % n)
        blocks.append((n, np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)))
    if not blocks:
        raise ValueError("no moments to pool")
    shapes = set(b[1].shape for b in blocks) | set(b[2].shape for b in blocks)
    if len(shapes) != 1:
        raise ValueError("moments of different shapes: %s" % sorted(shapes))
    while len(blocks) > 1:
        merged = [_merge(blocks[i], blocks[i + 1]) for i in range(0, len(blocks) - 1, 2)]
        if len(blocks) % 2:
            merged.append(blocks[-1])
        blocks = merged
    n, mean, m2 = blocks[0]
    if n == 0:
        mean, m2 = np.zeros_like(mean), np.zeros_like(m2)
    return n, mean, m2


def std_from_m2(n, m2):
    """sqrt(M2 / (n - 1)); NaN for n < 2."""
    m2 = np.asarray(m2, dtype=np.float64)
    if n < 2:
        return np.full(m2.shape, np.nan)
    return np.sqrt(np.maximum(m2, 0.0) / (n - 1.0))


class PosteriorMoments(object):
    """
    ``count`` samples' moments.  ``fetch(which)`` returns ``(mean, M2)`` of the parameter map
    (``which`` 0: (H, W, 4), columns a, c, w, F), the clean cube (1) or the convolved cube
    (2: (D, H, W)); it is called on first access of an attribute that needs it and its result
    is kept.  ``template``: the Cube whose axes and meta ``clean_cube()`` / ``convolved_cube()``
    carry.

    ``*_std`` is ``sqrt(M2 / (count - 1))``: NaN for ``count < 2``.  With ``count == 0``
    every array is NaN.
    """

    def __init__(self, count, fetch, template=None, histograms=None):
        self.count = int(count)
        self._fetch = fetch
        self._template = template
        self._cache = {}
        self.histograms = histograms    # a PosteriorHistograms, or None
        self.regions = None             # a regions.RegionPosterior (Run(regions=...)), or None
        self.predictive = None          # a predictive.PredictiveAccuracy (Run(predictive=...)), or None

    @classmethod
    def from_engine(cls, engine, template=None, histograms=False):
        """The moments a device context holds now (downloaded on first access); ``histograms``:
        with the context's histograms (hist_begin) as ``.histograms``."""
        return cls(engine.post_count(), engine.post_get, template,
                   PosteriorHistograms.from_engine(engine) if histograms else None)

    def moments(self, which):
        """``(count, mean, M2)`` as :func:`pool` takes them."""
        if which not in self._cache:
            mean, m2 = self._fetch(which)
            self._cache[which] = (np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64))
        return (self.count,) + self._cache[which]

    def _mean(self, which):
        n, mean, _ = self.moments(which)
        return mean if n > 0 else np.full(mean.shape, np.nan)

    def _std(self, which):
        n, _, m2 = self.moments(which)
        return std_from_m2(n, m2)

    @property
    def parameters_mean(self):
        return self._mean(PARAMETERS)[..., :3]

    @property
    def parameters_std(self):
        return self._std(PARAMETERS)[..., :3]

    @property
    def flux_mean(self):
        return self._mean(PARAMETERS)[..., 3]

    @property
    def flux_std(self):
        return self._std(PARAMETERS)[..., 3]

    @property
    def clean_mean(self):
        return self._mean(CLEAN)

    @property
    def clean_std(self):
        return self._std(CLEAN)

    @property
    def convolved_mean(self):
        return self._mean(CONVOLVED)

    @property
    def convolved_std(self):
        return self._std(CONVOLVED)

    def _cube(self, data):
        t = self._template
        if t is None:
            return Cube(data=data)
        return Cube(data=data, meta=t.meta, x=t.x, y=t.y, z=t.z)

    def clean_cube(self):
        """E[clean cube] as a Cube with the input's axes and meta."""
        return self._cube(self.clean_mean)

    def convolved_cube(self):
        """E[convolved cube] as a Cube with the input's axes and meta."""
        return self._cube(self.convolved_mean)

    def save(self, prefix, clobber=False):
        """``<prefix>_posterior_{clean,convolved}_{mean,std}.fits`` and
        ``<prefix>_posterior_parameters.npz`` (count, parameters_mean, parameters_std,
        flux_mean, flux_std), beside the files of ``Run.save(prefix)``; with regions their
        ``<prefix>_posterior_regions.npz``, with the predictive accuracy its
        ``<prefix>_posterior_predictive.npz``."""
        for name in ("clean", "convolved"):
            for kind in ("mean", "std"):
                self._cube(getattr(self, "%s_%s" % (name, kind))).to_fits(
                    "%s_posterior_%s_%s.fits" % (prefix, name, kind), clobber)
        np.savez("%s_posterior_parameters.npz" % prefix, count=self.count,
                 parameters_mean=self.parameters_mean, parameters_std=self.parameters_std,
                 flux_mean=self.flux_mean, flux_std=self.flux_std)
        if self.regions is not None:
            self.regions.save(prefix)
        if self.predictive is not None:
            self.predictive.save(prefix)


class PosteriorHistograms(object):
    """
    The histograms of one chain's ``(a, c, w, F)`` samples after the pilot: per unmasked spaxel
    and quantity 64 equal bins over a range frozen at the pilot's mean +- span standard deviations
    (clipped to the model's bounds), and two tail counters for what fell outside.  Everything is
    (H, W, 4) in the order a, c, w, F and NaN where masked or while ``count == 0``.

    ``count``: samples in every histogram.  ``quantiles(qs)``: (H, W, 4, len(qs)), extracted on
    the device, linear inside the crossing bin -- within one bin width ``(hi - lo) / 64`` of the
    sample quantile while it lies inside the range, else the range's end.  ``median``;
    ``interval(0.68)``: the central interval ``(lo, hi)``; ``mode``: the centre of the fullest
    bin; ``outside``: the share of the samples beyond the range -- a mode the pilot never visited
    is counted there, not resolved: read a spaxel with a large share off the chain instead.
    ``counts`` (H, W, 4, 64), ``tails`` (H, W, 4, 2: below, above) and ``range`` (H, W, 4, 2: lo,
    hi) are the downloaded counters.  Device results are fetched on first access and kept.
    """

    def __init__(self, count, get, quantiles, pilot=None, span=None):
        self.count = int(count)
        self.pilot, self.span = pilot, span
        self._get = get
        self._quantiles = quantiles
        self._raw = None
        self._cache = {}

    @classmethod
    def from_engine(cls, engine, pilot=None, span=None):
        return cls(engine.hist_count(), engine.hist_get, engine.hist_quantiles, pilot, span)

    def _counters(self):
        if self._raw is None:
            self._raw = self._get()
        return self._raw

    counts = property(lambda self: self._counters()[0])
    tails = property(lambda self: self._counters()[1])
    range = property(lambda self: self._counters()[2])

    def _extract(self, qs):
        qs = tuple(float(q) for q in np.atleast_1d(qs))
        if not qs:
            raise ValueError("no quantile asked for")
        for q in qs:
            if not 0. < q < 1.:
                raise ValueError("quantile %r lies outside (0, 1)" % q)
        if qs not in self._cache:
            parts = [self._quantiles(qs[i:i + 8]) for i in range(0, len(qs), 8)]
            self._cache[qs] = (np.concatenate([p[0] for p in parts], axis=-1),) + tuple(parts[0][1:])
        return self._cache[qs]

    def quantiles(self, qs):
        return self._extract(qs)[0]

    @property
    def median(self):
        return self._extract((0.5,))[0][..., 0]

    def interval(self, mass=0.68):
        """The central interval holding ``mass`` of the samples: ``(lo, hi)``."""
        if not 0. < mass < 1.:
            raise ValueError("interval(%r): a mass inside (0, 1)" % mass)
        both = self._extract((0.5 - 0.5 * mass, 0.5 + 0.5 * mass))[0]
        return both[..., 0], both[..., 1]

    @property
    def mode(self):
        return self._extract((0.5,))[1]

    @property
    def outside(self):
        return self._extract((0.5,))[2]

    def save(self, prefix):
        """``<prefix>_posterior_histograms.npz``: count, pilot, span, counts, tails, range, median,
        the 68 % interval (lo68, hi68), mode and outside."""
        lo68, hi68 = self.interval(0.68)
        np.savez("%s_posterior_histograms.npz" % prefix, count=self.count,
                 pilot=-1 if self.pilot is None else self.pilot,
                 span=np.nan if self.span is None else self.span,
                 counts=self.counts, tails=self.tails, range=self.range, median=self.median,
                 lo68=lo68, hi68=hi68, mode=self.mode, outside=self.outside)


def check_histograms(keyword, burn_in):
    """``Run``'s ``posterior_histograms``: None / False (off: returns None), True, or a dict with
    any of ``pilot`` (integer >= 2) and ``span`` (finite, positive); returns
    ``dict(pilot=200, span=6.0)`` updated with it.  Needs ``posterior_burn_in`` (ValueError)."""
    if keyword is None or keyword is False:
        return None
    cfg = dict(pilot=200, span=6.0)
    if keyword is not True:
        if not isinstance(keyword, dict):
            raise ValueError("posterior_histograms= MUST be None, True or a dict(pilot=, span=), got %r"
                             % (keyword,))
        unknown = sorted(set(keyword) - set(cfg))
        if unknown:
            raise ValueError("posterior_histograms=: unknown key(s) %s (pilot, span)" % unknown)
        cfg.update(keyword)
    pilot, span = cfg["pilot"], cfg["span"]
    if isinstance(pilot, bool) or not isinstance(pilot, (int, np.integer)) or pilot < 2:
        raise ValueError("posterior_histograms=: pilot MUST be an integer >= 2, got %r" % (pilot,))
    if isinstance(span, bool) or not isinstance(span, (int, float, np.integer, np.floating)) \
            or not np.isfinite(span) or not span > 0:
        raise ValueError("posterior_histograms=: span MUST be a finite positive number, got %r" % (span,))
    if burn_in is None:
        raise ValueError("posterior_histograms= needs posterior_burn_in=: the histograms count the "
                         "samples the posterior moments take")
    return dict(pilot=int(pilot), span=float(span))


def pooled(parts, template=None):
    """The PosteriorMoments of several chains' together (``chains=R``)."""
    parts = list(parts)
    return PosteriorMoments(sum(p.count for p in parts),
                            lambda which: pool([p.moments(which) for p in parts])[1:], template)


def check_schedule(burn_in, every):
    """``Run``'s ``posterior_burn_in`` / ``posterior_every``: integers >= 1 (ValueError)."""
    for name, value in (("posterior_burn_in", burn_in), ("posterior_every", every)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError("%s= MUST be an integer, got %r" % (name, value))
        if value < 1:
            raise ValueError("%s= MUST be >= 1, got %d" % (name, value))
    return int(burn_in), int(every)
