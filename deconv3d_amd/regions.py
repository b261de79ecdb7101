# coding=utf-8
"""
Region posteriors of a run: the posterior of SETS of spaxels -- the flux of an aperture, the
flux-weighted centre and width of a ring, the integrated clean spectrum of a region with its
error bar -- kept on the device while the chain runs (include/deconv3d_hip.h: d3d_region_*;
``Run(regions=...)``).

Under an FSF wider than a spaxel neighbours trade flux: a spaxel's own ``(a, c, w, F)`` are
heavy-tailed while the sum over a set is well determined, and its standard deviation cannot be
had from the per-spaxel ones (the covariances are what matters).  The reference has the
per-spaxel mean of the saved chain only (lib/run.py:581-593).  This module holds the host side:
label-map builders, the keyword's checks, and :class:`RegionPosterior`, the lazily downloaded
series and spectra with their numpy summaries.
"""
from __future__ import annotations

import numpy as np

from .posterior import pool, std_from_m2


def blocks(shape, size):
    """Label map of square bins: ``shape = (H, W)`` cut into ``size`` x ``size`` blocks from the
    top left corner (those at the far edges may be smaller), numbered 1 .. K in row-major order."""
    H, W = (int(v) for v in shape)
    size = int(size)
    if H < 1 or W < 1 or size < 1:
        raise ValueError("blocks(%r, %r): a positive shape and size" % (shape, size))
    per_row = -(-W // size)
    y, x = np.mgrid[0:H, 0:W]
    return ((y // size) * per_row + x // size + 1).astype(np.int32)


def annuli(shape, centre, edges, pa=0., inclination=0.):
    """Label map of elliptical rings: ring k = 1 .. len(edges) - 1 holds the spaxels whose
    deprojected radius r lies in ``[edges[k-1], edges[k])``, 0 elsewhere.  ``centre = (y, x)`` in
    spaxels, ``pa`` the position angle of the major axis in degrees from the +y axis towards -x
    (north through east on a sky image), ``inclination`` in degrees (0: circles): with (u, v) the
    offsets along the major and minor axis, ``r = sqrt(u^2 + (v / cos i)^2)``."""
    H, W = (int(v) for v in shape)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if edges.size < 2 or not np.all(np.isfinite(edges)) or edges[0] < 0 or np.any(np.diff(edges) <= 0):
        raise ValueError("annuli: edges MUST be at least two increasing, finite, non-negative radii")
    cosi = np.cos(np.radians(float(inclination)))
    if not cosi > 1e-6:
        raise ValueError("annuli: inclination=%r is edge-on or beyond" % (inclination,))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dy, dx = y - float(centre[0]), x - float(centre[1])
    t = np.radians(float(pa))
    u = dy * np.cos(t) - dx * np.sin(t)
    v = dy * np.sin(t) + dx * np.cos(t)
    r = np.sqrt(u * u + (v / cosi) ** 2)
    ring = np.searchsorted(edges, r, side="right")
    return np.where((ring >= 1) & (ring < edges.size), ring, 0).astype(np.int32)


def compact(labels):
    """``(compacted, ids)``: the positive labels renumbered 1 .. K in ascending order of their
    value (int32), and the K original values."""
    labels = np.asarray(labels)
    ids = np.unique(labels[labels > 0])
    out = np.zeros(labels.shape, dtype=np.int32)
    live = labels > 0
    out[live] = np.searchsorted(ids, labels[live]) + 1
    return out, ids


def check_shape(labels, shape):
    """ValueError unless the label map has the (H, W) ``shape`` of the field."""
    if tuple(labels.shape) != tuple(shape):
        raise ValueError("regions=: labels MUST have the (%d, %d) shape of the field, got %s"
                         % (shape[0], shape[1], tuple(labels.shape)))


def check_regions(keyword, shape, burn_in):
    """``Run``'s ``regions=``: None (off: returns None), an (H, W) integer array of labels (0: no
    region, any positive value names one) or ``dict(labels=, spectra=True)``; ``shape``: the
    field's (H, W), or None when it is not known yet (:func:`check_shape` later).  Returns
    ``dict(labels=<compacted int32>, ids=<original values>, spectra=bool)``.  ValueError for a
    wrong shape, a non-integer dtype, negative labels, a map of zeros, unknown keys, or a missing
    ``posterior_burn_in``."""
    if keyword is None:
        return None
    cfg = dict(labels=None, spectra=True)
    if isinstance(keyword, dict):
        unknown = sorted(set(keyword) - set(cfg))
        if unknown:
            raise ValueError("regions=: unknown key(s) %s (labels, spectra)" % unknown)
        cfg.update(keyword)
        if cfg["labels"] is None:
            raise ValueError("regions=: the dict needs labels=")
    else:
        cfg["labels"] = keyword
    if not isinstance(cfg["spectra"], (bool, np.bool_)):
        raise ValueError("regions=: spectra MUST be True or False, got %r" % (cfg["spectra"],))
    labels = np.asarray(cfg["labels"])
    if labels.dtype.kind not in "iu":
        raise ValueError("regions=: labels MUST be integers, got dtype %s" % labels.dtype)
    if labels.ndim != 2:
        raise ValueError("regions=: labels MUST be an (H, W) map, got shape %s" % (labels.shape,))
    if shape is not None:
        check_shape(labels, shape)
    if (labels < 0).any():
        raise ValueError("regions=: negative labels (0 is no region, a positive value names one)")
    if not (labels > 0).any():
        raise ValueError("regions=: every label is 0, no region to follow")
    if burn_in is None:
        raise ValueError("regions= needs posterior_burn_in=: a region's series holds the samples the "
                         "posterior moments take")
    compacted, ids = compact(labels)
    return dict(labels=compacted, ids=ids, spectra=bool(cfg["spectra"]))


class RegionPosterior(object):
    """
    The samples of K regions' ``(F, C, S)`` -- summed flux, flux-weighted centre and width (the
    second moment of the summed line, so it holds the spread of the members' centres too) -- and
    the moments of their summed clean spectra.

    ``count``: samples taken (the spectra hold them all); ``get()`` returns ``(series (n, K, 3), spectrum mean (K, D) or None,
    spectrum M2 or None, sizes (K))`` and is called on first access of an attribute that needs it.
    ``ids`` (K): the labels' original values, ``sizes`` (K): unmasked members.  ``flux``,
    ``centre``, ``width``: the series (n, K) -- n may be smaller than ``count`` when the device
    series was full; ``*_mean`` / ``*_std`` (K) over the series (std with ddof = 1; NaN without
    enough samples); ``quantiles(qs)``: (K, 3, len(qs)) of F, C, S; ``flux_covariance()``: (K, K),
    where the anticorrelation between neighbouring regions shows; ``spectrum_mean`` /
    ``spectrum_std`` (K, D) (None without spectra).  A region without members or flux has F = 0
    and C = S = NaN in that sample.
    """

    def __init__(self, count, get, ids=None):
        self.count = int(count)
        self._get = get
        self._raw = None
        self._ids = None if ids is None else np.asarray(ids)

    @classmethod
    def from_engine(cls, engine, ids=None):
        return cls(engine.region_count()[0], engine.region_get, ids)

    def _data(self):
        if self._raw is None:
            series, mean, m2, sizes = self._get()
            self._raw = (np.asarray(series, dtype=np.float64).reshape(-1, len(sizes), 3),
                         None if mean is None else np.asarray(mean, dtype=np.float64),
                         None if m2 is None else np.asarray(m2, dtype=np.float64), np.asarray(sizes))
        return self._raw

    series = property(lambda self: self._data()[0])
    sizes = property(lambda self: self._data()[3])
    flux = property(lambda self: self.series[..., 0])
    centre = property(lambda self: self.series[..., 1])
    width = property(lambda self: self.series[..., 2])

    @property
    def ids(self):
        return np.arange(1, len(self.sizes) + 1) if self._ids is None else self._ids

    def _mean(self, k):
        s = self.series[..., k]
        return s.mean(axis=0) if s.shape[0] else np.full(s.shape[1], np.nan)

    def _std(self, k):
        s = self.series[..., k]
        return s.std(axis=0, ddof=1) if s.shape[0] > 1 else np.full(s.shape[1], np.nan)

    flux_mean = property(lambda self: self._mean(0))
    flux_std = property(lambda self: self._std(0))
    centre_mean = property(lambda self: self._mean(1))
    centre_std = property(lambda self: self._std(1))
    width_mean = property(lambda self: self._mean(2))
    width_std = property(lambda self: self._std(2))

    def quantiles(self, qs):
        """(K, 3, len(qs)): numpy's (linear) quantiles of the F, C and S series; NaN without samples."""
        qs = np.atleast_1d(np.asarray(qs, dtype=np.float64))
        if not qs.size or ((qs < 0.) | (qs > 1.)).any():
            raise ValueError("quantiles(%r): values inside [0, 1]" % (qs,))
        s = self.series
        if not s.shape[0]:
            return np.full((s.shape[1], 3, qs.size), np.nan)
        return np.moveaxis(np.quantile(s, qs, axis=0), 0, -1)

    def flux_covariance(self):
        """(K, K) sample covariance (ddof = 1) of the regions' fluxes; NaN with fewer than 2 samples."""
        f = self.flux
        if f.shape[0] < 2:
            return np.full((f.shape[1], f.shape[1]), np.nan)
        d = f - f.mean(axis=0)
        return d.T.dot(d) / (f.shape[0] - 1.0)

    def spectrum_moments(self):
        """``(count, mean, M2)`` of the spectra as :func:`deconv3d_amd.posterior.pool` takes them."""
        _, mean, m2, _ = self._data()
        if mean is None:
            raise ValueError("the regions' spectra were not kept (regions=dict(spectra=False))")
        return self.count, mean, m2

    @property
    def spectrum_mean(self):
        if self._data()[1] is None:
            return None
        n, mean, _ = self.spectrum_moments()
        return mean if n > 0 else np.full(mean.shape, np.nan)

    @property
    def spectrum_std(self):
        if self._data()[1] is None:
            return None
        n, _, m2 = self.spectrum_moments()
        return std_from_m2(n, m2)

    def save(self, prefix):
        """``<prefix>_posterior_regions.npz``: count, ids, sizes, the series flux / centre / width and,
        with spectra, spectrum_mean and spectrum_std."""
        out = dict(count=self.count, ids=self.ids, sizes=self.sizes, flux=self.flux, centre=self.centre,
                   width=self.width)
        if self.spectrum_mean is not None:
            out.update(spectrum_mean=self.spectrum_mean, spectrum_std=self.spectrum_std)
        np.savez("%s_posterior_regions.npz" % prefix, **out)


def pooled(parts):
    """The RegionPosterior of several chains' together (``chains=R``): the series concatenated chain
    by chain, the spectra pooled with :func:`deconv3d_amd.posterior.pool`."""
    parts = list(parts)

    def get():
        raws = [p._data() for p in parts]
        series = np.concatenate([r[0] for r in raws], axis=0)
        mean = m2 = None
        if raws[0][1] is not None:
            _, mean, m2 = pool([p.spectrum_moments() for p in parts])
        return series, mean, m2, raws[0][3]

    return RegionPosterior(sum(p.count for p in parts), get, parts[0]._ids)
