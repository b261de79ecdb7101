# coding=utf-8
"""
Matched-filter line search: a detection S/N map, a mask and a starting parameter map
before any chain runs.

The reference starts every spaxel from a uniform draw inside the bounds
(lib/run.py:310-314) and masks by spectrally summed flux (lib/masks.py:17-29).  Here every
spaxel's spectrum is correlated, on the device (``d3d_line_search``), with the
LSF-convolved unit line of the run's line model over a grid of centres and widths,
weighted by the variance cube::

    N_k = sum_z T_k[z] d[z] / var[z]      Q_k = sum_z T_k[z]^2 / var[z]
    s_k = N_k / sqrt(Q_k)                 (the S/N of the best-fit amplitude a_k = N_k / Q_k)

The host part below is plain numpy: grid defaults and checks, and the refinement of the
device's per-spaxel winner into ``(a, c, w)``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .instruments import Instrument
from .line_models import (LineModel, SingleGaussianLineModel, device_line_shape,
                          device_line_table, model_is_on_device)
from .math_utils import median_clip

DEFAULT_WIDTH_COUNT = 8
DEFAULT_JITTER = (0.5, 0.1)      # chains r > 0: channels in c, relative in w


def default_centres(depth):
    """Every integer channel."""
    return np.arange(int(depth), dtype=np.float64)


def default_widths(depth):
    """8 geometric widths from 0.75 channel to max(depth / 6, 1.5)."""
    return np.geomspace(0.75, max(depth / 6., 1.5), DEFAULT_WIDTH_COUNT)


def check_grid(centres=None, widths=None, depth=None):
    """Validated ``(centres, widths, step)``; ``None`` stays ``None`` until ``depth`` is known.
    ``centres`` must be finite and uniformly spaced (ascending), ``widths`` finite and positive."""
    if centres is None and depth is not None:
        centres = default_centres(depth)
    if widths is None and depth is not None:
        widths = default_widths(depth)
    step = 0.
    if centres is not None:
        centres = np.array(centres, dtype=np.float64).reshape(-1)
        if centres.size == 0 or not np.isfinite(centres).all():
            raise ValueError("centres= MUST be a non-empty sequence of finite channels")
        if centres.size > 1:
            d = np.diff(centres)
            step = float(centres[-1] - centres[0]) / (centres.size - 1)
            if not step > 0. or np.max(np.abs(d - step)) > 1e-9 * step:
                raise ValueError("centres= MUST be uniformly spaced and ascending: the sub-grid "
                                 "refinement interpolates between neighbours")
    if widths is not None:
        widths = np.array(widths, dtype=np.float64).reshape(-1)
        if widths.size == 0 or not np.isfinite(widths).all() or not (widths > 0.).all():
            raise ValueError("widths= MUST be a non-empty sequence of positive numbers")
    return centres, widths, step


def check_keywords(initial_search, initial_parameters=None, resume_state=None):
    """``Run(initial_search=)``: ``None`` / ``False`` (off) -> ``None``; ``True`` or a dict of
    ``line_search`` keywords (``centres``, ``widths``) plus ``jitter`` -> a checked dict.
    Raises before any device work."""
    if initial_search is None or initial_search is False:
        return None
    if initial_parameters is not None:
        raise ValueError("initial_search= and initial_parameters= both give chain 0's start: "
                         "pass one of them")
    if resume_state is not None:
        raise ValueError("initial_search= with resume_state=: a resumed chain continues from its "
                         "checkpoint, not from a searched map")
    cfg = {} if initial_search is True else dict(initial_search)
    unknown = sorted(set(cfg) - {"centres", "widths", "jitter"})
    if unknown:
        raise ValueError("initial_search= takes the keys centres, widths and jitter, got %s" % unknown)
    centres, widths, _ = check_grid(cfg.get("centres"), cfg.get("widths"))
    try:
        jitter = tuple(float(v) for v in cfg.get("jitter", DEFAULT_JITTER))
    except (TypeError, ValueError):
        raise ValueError("jitter MUST be two numbers: channels in c, relative in w")
    if len(jitter) != 2 or not all(np.isfinite(v) and v >= 0. for v in jitter):
        raise ValueError("jitter MUST be two non-negative numbers (channels in c, relative in w), "
                         "got %s" % (jitter,))
    return dict(centres=centres, widths=widths, jitter=jitter)


def refine(best, stat, centres, widths, min_boundaries=None, max_boundaries=None):
    """``(snr, parameters)`` from the device's ``best`` (H,W) and ``stat`` (H,W,4) =
    ``{N, Q, s(i_c - 1), s(i_c + 1)}``: ``a = N / Q``, ``w = widths[i_w]``, and
    ``c = centres[i_c] + step * delta`` with the vertex of the parabola through the three
    statistics, ``delta = (s- - s+) / (2 (s- - 2 s0 + s+))`` -- only where both neighbours are
    finite and the curvature is negative, clipped to half a step -- then everything clipped
    to the bounds.  ``best = -1``: NaN S/N and NaN parameters."""
    centres, widths, step = check_grid(centres, widths)
    best = np.asarray(best)
    stat = np.asarray(stat, dtype=np.float64)
    n_c = centres.size
    det = best >= 0
    k = np.where(det, best, 0)
    i_w, i_c = k // n_c, k % n_c
    with np.errstate(invalid="ignore", divide="ignore"):
        N, Q = stat[..., 0], stat[..., 1]
        s0 = N / np.sqrt(Q)
        sm, sp = stat[..., 2], stat[..., 3]
        den = sm - 2. * s0 + sp
        ok = det & np.isfinite(sm) & np.isfinite(sp) & (den < 0.)
        delta = np.clip(np.where(ok, 0.5 * (sm - sp) / np.where(ok, den, 1.), 0.), -0.5, 0.5)
        a = N / Q
    parameters = np.stack([a, centres[i_c] + step * delta, widths[i_w]], axis=-1)
    if min_boundaries is not None:
        parameters = np.maximum(parameters, np.asarray(min_boundaries, dtype=np.float64))
    if max_boundaries is not None:
        parameters = np.minimum(parameters, np.asarray(max_boundaries, dtype=np.float64))
    parameters[~det] = np.nan
    return np.where(det, s0, np.nan), parameters


class LineSearch(object):
    """Result of :func:`line_search`: ``snr`` (H,W) detection S/N of the best template (NaN:
    none, or masked), ``parameters`` (H,W,3) its refined ``(a, c, w)`` (NaN there),
    ``best_index`` (H,W) ``i_w * len(centres) + i_c`` or -1, ``stat`` the device's (H,W,4)
    ``{N, Q, s-, s+}``, the grid ``centres`` / ``widths``."""

    def __init__(self, best, stat, centres, widths, min_boundaries=None, max_boundaries=None):
        self.centres, self.widths, self.step = check_grid(centres, widths)
        self.best_index = np.asarray(best)
        self.stat = np.asarray(stat, dtype=np.float64)
        self.snr, self.parameters = refine(best, stat, self.centres, self.widths,
                                           min_boundaries, max_boundaries)

    @property
    def detected(self):
        return self.best_index >= 0

    def mask(self, threshold=5.):
        """1/0 image like ``masks.above_percentile``: 1 where the S/N reaches ``threshold``."""
        with np.errstate(invalid="ignore"):
            return np.where(self.snr >= threshold, 1.0, 0.0)


def _padded_length(depth):
    return 1 << max(1, int(depth - 1).bit_length())      # lib/convolution.py:137-141


def lsf_convolve_rows(lines, lsf):
    """``convolve_1d`` (lib/convolution.py:89-120) of every row of ``lines`` (n, D) in its
    closed form, out[k] = sum_t lsf[t] ext[(k + N/2 - h - t) mod N]; identity for ``lsf=None``
    (lib/run.py:675-676)."""
    lines = np.asarray(lines, dtype=np.float64)
    if lsf is None:
        return lines
    lsf = np.asarray(lsf, dtype=np.float64)
    depth = lines.shape[1]
    n = _padded_length(depth)
    diff = n - depth
    h = diff // 2 + 1 if diff & 1 else diff // 2
    ext = np.zeros((lines.shape[0], n))
    ext[:, :depth] = lines
    k = np.arange(depth)
    out = np.zeros_like(lines)
    for t in np.nonzero(lsf)[0]:
        out += lsf[t] * ext[:, (k + n // 2 - h - t) % n]
    return out


def host_bank(model, runner, centres, widths, lsf, depth):
    """(n_w * n_c, D) templates of a host-evaluated line model: its ``modelize`` at
    ``(1, c, w)``, LSF-convolved."""
    if len(model.parameters()) != 3 or model.gibbs_parameter_index() != 0:
        raise NotImplementedError(
            "line search: the line model %s is not an (amplitude, centre, width) model with a "
            "Gibbs-sampled amplitude" % type(model).__name__)
    x = np.arange(depth, dtype=np.float64)
    rows = [np.asarray(model.modelize(runner, x, np.array([1., c, w])), dtype=np.float64)
            for w in widths for c in centres]
    return lsf_convolve_rows(np.array(rows), lsf)


def search_engine(engine, model, runner, centres=None, widths=None, lsf=None):
    """Search on an :class:`_lib.Engine` whose taps, data and line shape are set.  ``runner``:
    what the model's bounds and ``modelize`` read (``cube``, ``fsf``)."""
    depth = engine.shape[0]
    centres, widths, _ = check_grid(centres, widths, depth)
    bank = None
    if not model_is_on_device(model):
        bank = host_bank(model, runner, centres, widths, lsf, depth)
    best, stat = engine.line_search(centres, widths, bank=bank)
    min_b = np.array(model.min_boundaries(runner), dtype=np.float64)
    max_b = np.array(model.max_boundaries(runner), dtype=np.float64)
    return LineSearch(best, stat, centres, widths, min_b, max_b)


def jittered_start(parameters, jitter, rng, min_boundaries, max_boundaries):
    """A dispersed copy of a searched map for chain r > 0: ``c + jitter[0] n`` and
    ``w (1 + jitter[1] n')``, n standard normal draws of ``rng``, clipped to the bounds."""
    out = np.array(parameters, dtype=np.float64)
    draws = rng.standard_normal(out.shape[:2] + (2,))
    out[..., 1] = out[..., 1] + jitter[0] * draws[..., 0]
    out[..., 2] = out[..., 2] * (1. + jitter[1] * draws[..., 1])
    return np.clip(out, min_boundaries, max_boundaries)


class _Runner(object):
    """What a LineModel reads of a runner (lib/line_models.py:79-90)."""

    def __init__(self, cube, fsf, lsf):
        self.cube, self.fsf, self.lsf = cube, fsf, lsf


def line_search(cube, instrument, variance=None, mask=None, model=SingleGaussianLineModel,
                centres=None, widths=None, device=0, prepare=None):
    """
    Matched-filter search of ``cube`` (FITS path or Cube) for the line of ``model`` as
    ``instrument`` sees it; ``variance``, ``mask``, ``model`` as :class:`Run` takes them
    (without a variance: the clipped noise estimate of lib/run.py:171-178).  ``centres``:
    uniformly spaced channels (default every integer channel); ``widths``: channels (default 8
    geometric steps from 0.75 to max(D / 6, 1.5)).  Returns a :class:`LineSearch`.  Masked
    spaxels are not detected; a NaN voxel only loses its weight.  ``prepare``: ``True`` or a dict
    of :func:`deconv3d_amd.prepare.prepare_cube` keywords -- search the continuum-free cube with
    its per-channel variance (or, ``rescale=True``, the given variance rescaled) instead.
    """
    from . import prepare as _prepare
    from .cube import Cube, read_fits
    from .masks import read_hyperspectral_cube
    centres, widths, _ = check_grid(centres, widths)          # (before any device work)
    prepare_cfg = _prepare.check_keywords(prepare)
    cube = read_hyperspectral_cube(cube)
    if prepare_cfg is not None:
        if prepare_cfg["rescale"] and variance is None:
            raise ValueError("prepare=dict(rescale=True) needs the variance= cube it rescales")
        prepared = _prepare.prepare_cube(
            cube, prepare_cfg["continuum_window"], prepare_cfg["reject"], prepare_cfg["noise_mask"],
            variance=variance if prepare_cfg["rescale"] else None, rescale=prepare_cfg["rescale"],
            device=device)
        cube = prepared.cube
        if variance is None or prepare_cfg["rescale"]:
            variance = prepared.variance
    if not isinstance(instrument, Instrument):
        raise TypeError("Provided instrument is not an Instrument")
    depth, height, width = cube.data.shape
    if mask is not None:
        if isinstance(mask, str):
            mask, _ = read_fits(mask)
        mask = np.array(mask, dtype=np.float64)
        if mask.shape != (height, width):
            raise ValueError("Mask MUST have (%d, %d) shape, got %s." % (height, width, str(mask.shape)))
    if variance is not None:
        if isinstance(variance, str):
            variance = Cube.from_fits(variance)
        variance = variance.data if isinstance(variance, Cube) else variance
        if not isinstance(variance, np.ndarray):
            raise TypeError("Provided variance is not a Cube")
        variance = np.where(variance == 0.0, 1e12, variance)
    else:
        _, clip_sigma, _ = median_clip(np.copy(cube.data[2:-2, 2:-4, 2:4]), 2.5)
        variance = np.ones(cube.data.shape) * (clip_sigma if clip_sigma != 0 else 1e-20) ** 2
    if variance.shape != cube.data.shape:
        raise ValueError("Provided variance has not the correct shape."
                         "Expected %s, got %s" % (str(cube.data.shape), str(variance.shape)))
    if not isinstance(model, LineModel):
        model = model()
        if not isinstance(model, LineModel):
            raise TypeError("Provided model is not a LineModel")
    lsf = instrument.lsf.as_vector(cube)
    lsf = None if lsf is None else np.asarray(lsf, dtype=np.float64)
    fsf = np.asarray(instrument.fsf.as_image(cube), dtype=np.float64)
    runner = _Runner(cube, fsf, lsf)
    with _lib.Engine(cube.data.shape, fsf.shape, device=device) as engine:
        engine.set_taps(fsf, lsf)
        engine.set_data(cube.data, variance, mask=mask)
        if model_is_on_device(model):
            engine.set_line_shape(*device_line_shape(model))
            table = device_line_table(model)
            if table is not None:
                engine.set_line_table(*table)
        return search_engine(engine, model, runner, centres, widths, lsf)
