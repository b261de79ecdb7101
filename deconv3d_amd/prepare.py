# coding=utf-8
"""
Preparing a raw cube: continuum removal and channel noise, on the device.

:class:`Run` and :func:`deconv3d_amd.search.line_search` fit one emission line on a zero
baseline, and without ``variance=`` they take ONE constant for the whole cube,
``median_clip(data[2:-2, 2:-4, 2:4], 2.5)`` (lib/run.py:171-192).  A raw spectrum has stellar
continuum under the line, and its noise depends on the channel (sky lines).  ``prepare_cube``

1. takes the running median of every spectrum over ``continuum_window`` channels (the finite
   voxels of a window that shrinks at the ends) as the continuum and subtracts it;
2. takes ``sigma_z = 1.4826 MAD`` of every channel plane of the residual, over the spaxels of
   ``noise_mask``, as that channel's noise (NaN: fewer than two values, or a zero MAD);
3. with ``reject``, repeats both once without the voxels beyond ``reject * sigma_z`` -- the line
   itself, which would otherwise pull the median up;
4. returns ``sigma_z ** 2`` as the variance cube (``1e12``, the reference's "no information"
   value of lib/run.py:180, where sigma is NaN), or with ``variance=`` and ``rescale=True`` the
   given cube times ``sigma_z ** 2 / median_z(variance)``.

Both selections run on the device (``d3d_prepare``, ``d3d_channel_stats``) and are exact; the
host part below is checks and the arithmetic of step 4.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .cube import Cube

NO_INFORMATION = 1e12        # lib/run.py:180
KEYWORDS = ("continuum_window", "reject", "noise_mask", "rescale")


def check_settings(continuum_window=51, reject=3.0, rescale=False):
    """Validated ``(continuum_window, reject, rescale)``; raises before any device work."""
    try:
        window = int(continuum_window)
        if window != continuum_window or isinstance(continuum_window, bool):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("continuum_window= MUST be an odd integer from 3 to 257, got %r"
                         % (continuum_window,))
    if window < 3 or window > 257 or window % 2 == 0:
        raise ValueError("continuum_window= MUST be an odd integer from 3 to 257, got %d" % window)
    if reject is not None:
        try:
            reject = float(reject)
        except (TypeError, ValueError):
            raise ValueError("reject= MUST be a positive number of sigmas or None, got %r" % (reject,))
        if not reject > 0.:
            raise ValueError("reject= MUST be a positive number of sigmas or None, got %r" % (reject,))
    if not isinstance(rescale, (bool, np.bool_)):
        raise ValueError("rescale= MUST be True or False, got %r" % (rescale,))
    return window, reject, bool(rescale)


def check_keywords(prepare):
    """``Run(prepare=)`` / ``line_search(prepare=)``: ``None`` / ``False`` (off) -> ``None``;
    ``True`` or a dict of :func:`prepare_cube` keywords (``continuum_window``, ``reject``,
    ``noise_mask``, ``rescale``) -> a checked dict.  Raises before any device work."""
    if prepare is None or prepare is False:
        return None
    if prepare is not True and not isinstance(prepare, dict):
        raise ValueError("prepare= MUST be True or a dict of prepare_cube keywords, got %r" % (prepare,))
    cfg = {} if prepare is True else dict(prepare)
    unknown = sorted(set(cfg) - set(KEYWORDS))
    if unknown:
        raise ValueError("prepare= takes the keys %s, got %s" % (", ".join(KEYWORDS), unknown))
    window, reject, rescale = check_settings(cfg.get("continuum_window", 51), cfg.get("reject", 3.0),
                                             cfg.get("rescale", False))
    return dict(continuum_window=window, reject=reject, noise_mask=cfg.get("noise_mask"),
                rescale=rescale)


def settings_record(settings):
    """What a checkpoint keeps of the settings (``resume_state=`` compares it):
    ``[continuum_window, reject (NaN: none), rescale, spaxels of the noise mask (-1: all)]``."""
    return np.array([settings["continuum_window"],
                     np.nan if settings["reject"] is None else settings["reject"],
                     1. if settings["rescale"] else 0.,
                     settings["noise_spaxels"]], dtype=np.float64)


def check_resume(state, files, settings):
    """Refuses a checkpoint written with other preparation settings than this run's
    (``settings``: ``Prepared.settings`` or ``None``)."""
    saved = np.asarray(state["prepare_settings"], dtype=np.float64) if "prepare_settings" in files else None
    mine = None if settings is None else settings_record(settings)
    if saved is None and mine is None:
        return
    if saved is None or mine is None or not np.array_equal(saved, mine, equal_nan=True):
        raise ValueError("resume_state was written with the preparation settings %s (continuum_window, "
                         "reject, rescale, noise spaxels), this run has %s"
                         % ("none" if saved is None else tuple(saved),
                            "none" if mine is None else tuple(mine)))


def channel_variance(sigma, shape, variance=None, variance_median=None):
    """Step 4: ``sigma_z ** 2`` on every plane (``1e12`` where sigma is NaN), or the given
    ``variance`` times ``sigma_z ** 2 / variance_median[z]``, a channel left unchanged where
    either factor is NaN or zero."""
    sigma = np.asarray(sigma, dtype=np.float64)
    s2 = sigma ** 2
    if variance is None:
        plane = np.where(np.isnan(sigma), NO_INFORMATION, s2)
        return np.ones(shape) * plane[:, None, None]
    out = np.array(variance, dtype=np.float64)
    m = np.asarray(variance_median, dtype=np.float64)
    for z in range(shape[0]):
        if np.isnan(s2[z]) or np.isnan(m[z]) or s2[z] == 0. or m[z] == 0.:
            continue
        out[z] = variance[z] * s2[z] / m[z]
    return out


class Prepared(object):
    """Result of :func:`prepare_cube`: ``cube`` (a :class:`Cube` of the residual with the input's
    metadata), ``continuum`` and ``variance`` (D,H,W), per channel ``sigma`` (NaN: no
    information), ``channel_median`` (of the residual) and ``channel_count`` (voxels it was
    estimated from), and ``settings`` (the keywords as used)."""

    def __init__(self, cube, continuum, variance, sigma, channel_median, channel_count, settings):
        self.cube = cube
        self.continuum = continuum
        self.variance = variance
        self.sigma = sigma
        self.channel_median = channel_median
        self.channel_count = channel_count
        self.settings = settings


def _check_inputs(cube, noise_mask, variance, rescale):
    from .masks import read_hyperspectral_cube
    if isinstance(cube, np.ndarray):
        if not (np.issubdtype(cube.dtype, np.floating) or np.issubdtype(cube.dtype, np.integer)):
            raise TypeError("The cube MUST hold real numbers, got %s" % cube.dtype)
        cube = Cube(data=cube)
    cube = read_hyperspectral_cube(cube)
    data = np.asarray(cube.data)
    if data.ndim != 3:
        raise ValueError("The cube MUST have three axes (D, H, W), got shape %s" % (data.shape,))
    depth, height, width = data.shape
    if noise_mask is not None:
        noise_mask = np.asarray(noise_mask)
        if noise_mask.shape != (height, width):
            raise ValueError("noise_mask MUST have (%d, %d) shape, got %s."
                             % (height, width, str(noise_mask.shape)))
        noise_mask = noise_mask != 0
        if not noise_mask.any():
            raise ValueError("noise_mask selects no spaxel")
    if variance is not None:
        if isinstance(variance, str):
            variance = Cube.from_fits(variance)
        variance = variance.data if isinstance(variance, Cube) else variance
        if not isinstance(variance, np.ndarray):
            raise TypeError("Provided variance is not a Cube")
        if variance.shape != data.shape:
            raise ValueError("Provided variance has not the correct shape."
                             "Expected %s, got %s" % (str(data.shape), str(variance.shape)))
    elif rescale:
        raise ValueError("rescale=True needs the variance= cube it rescales")
    return cube, np.ascontiguousarray(data, dtype=np.float64), noise_mask, variance


def prepare_cube(cube, continuum_window=51, reject=3.0, noise_mask=None, variance=None, rescale=False,
                 device=0):
    """
    Continuum-free cube and per-channel variance of a raw ``cube`` (FITS path, Cube or (D,H,W)
    array).  ``continuum_window``: odd, 3 to 257 channels, well above the line's width.
    ``reject``: sigmas of the one rejection pass (``None``: none).  ``noise_mask``: (H,W) image,
    non-zero where the noise is to be estimated (the sky; default everywhere).  ``variance`` with
    ``rescale=True``: rescale that cube channel by channel instead of replacing it (without
    ``rescale`` a given variance is returned unchanged).  Returns a :class:`Prepared`.
    """
    window, reject, rescale = check_settings(continuum_window, reject, rescale)     # (before any device work)
    cube, data, noise_mask, variance = _check_inputs(cube, noise_mask, variance, rescale)
    with _lib.Engine(data.shape, (1, 1), device=device) as engine:
        continuum, residual, median, sigma, count = engine.prepare(data, window // 2, reject, noise_mask)
        if variance is None:
            out_variance = channel_variance(sigma, data.shape)
        elif rescale:
            variance = np.ascontiguousarray(variance, dtype=np.float64)
            v_median = engine.channel_stats(variance, noise_mask)[0]
            out_variance = channel_variance(sigma, data.shape, variance, v_median)
        else:
            out_variance = np.array(variance, dtype=np.float64)
    settings = dict(continuum_window=window, reject=reject, rescale=rescale, noise_mask=noise_mask,
                    noise_spaxels=-1 if noise_mask is None else int(noise_mask.sum()))
    prepared = Cube(data=residual, meta=cube.meta, x=cube.x, y=cube.y, z=cube.z)
    return Prepared(prepared, continuum, out_variance, sigma, median, count, settings)
