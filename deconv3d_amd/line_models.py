# coding=utf-8
"""
Line-model plugin interface -- same names and contracts as the reference's
``lib/line_models.py`` (LineModel :4-61, SingleGaussianLineModel :64-109).

The device kernels implement ``SingleGaussianLineModel``,
``GaussianMultipletLineModel`` and ``TabulatedLineModel`` (amplitude Gibbs-sampled,
centre/width Metropolis-Hastings).  ``modelize`` below is the host evaluation of the same
curve, kept for API parity (plots, user scripts).
"""
import hashlib
import math
import struct

import numpy as np


class LineModel:
    """Interface of a spectral line model (lib/line_models.py:4-61)."""

    def __init__(self):
        pass

    def parameters(self):
        """Names of the parameters (unique strings)."""
        raise NotImplementedError()

    def gibbs_parameter_index(self):
        """Index of the Gibbs-sampled parameter (the amplitude), or None."""
        return None

    def min_boundaries(self, runner):
        raise NotImplementedError()

    def max_boundaries(self, runner):
        raise NotImplementedError()

    def post_jump(self, runner, old_parameters, new_parameters):
        """Optional hook mutating ``new_parameters`` after the Cauchy jump."""
        pass

    def modelize(self, runner, x, parameters):
        raise NotImplementedError()


class SingleGaussianLineModel(LineModel):
    """``a * exp(-(x-c)^2 / (2 w^2))`` with parameters ``['a', 'c', 'w']``."""

    def parameters(self):
        return ['a', 'c', 'w']

    def gibbs_parameter_index(self):
        return 0

    def min_boundaries(self, runner):
        return [0, 0, 0]

    def max_boundaries(self, runner):
        # lib/line_models.py:79-90: the FSF is normalised, so the amplitude
        # ceiling is max(data)/max(fsf); centre in [0, D-1], width in [0, D].
        # NaN voxels (masked spectra, lib/run.py:157-162) are ignored: the
        # reference's np.amax would make every bound NaN.
        data = runner.cube.data
        fsf_max = np.amax(runner.fsf)
        a_max = np.nanmax(data)
        if fsf_max > 0:
            a_max = a_max / fsf_max
        return [a_max, data.shape[0] - 1, data.shape[0]]

    def modelize(self, runner, x, parameters):
        return self.gaussian(np.asarray(x, dtype=np.float64),
                             parameters[0], parameters[1], parameters[2])

    @staticmethod
    def gaussian(x, a, c, w):
        return a * np.exp(-1. * (x - c) ** 2 / (2. * w ** 2))


class GaussianMultipletLineModel(LineModel):
    """
    K Gaussians of ONE centre and ONE width at fixed channel offsets with fixed
    flux ratios -- a multiplet with tied kinematics ([OII] 3726,3729, Halpha with
    the [NII] pair, the [SII] and [OIII] doublets)::

        a * sum_k ratios[k] * exp(-((x - c) - offsets[k])^2 / (2 w^2))

    The parameters are those of ``SingleGaussianLineModel``, ``['a', 'c', 'w']``
    with the same Gibbs index and bounds: ``c`` and ``a`` are the first
    component's centre and amplitude (``offsets[0] == 0``, ``ratios[0] == 1``).
    The line is still linear in ``a``, so the amplitude stays Gibbs-sampled, and
    the device kernels evaluate it themselves (``d3d_set_line_shape``).

    ``offsets``: channel offsets of the components from ``c``; ``ratios``: their
    flux ratios to ``a``.  1 to 4 components, every value finite, ratios >= 0,
    offsets distinct; anything else raises ``ValueError``.
    """

    MAX_COMPONENTS = 4

    def __init__(self, offsets, ratios):
        LineModel.__init__(self)
        try:
            off = [float(v) for v in np.atleast_1d(np.asarray(offsets, dtype=np.float64)).ravel()]
            rat = [float(v) for v in np.atleast_1d(np.asarray(ratios, dtype=np.float64)).ravel()]
        except (TypeError, ValueError):
            raise ValueError("offsets and ratios must be sequences of numbers")
        if len(off) != len(rat):
            raise ValueError("offsets and ratios must have the same length, got %d and %d"
                             % (len(off), len(rat)))
        if not 1 <= len(off) <= self.MAX_COMPONENTS:
            raise ValueError("a multiplet has 1 to %d components, got %d"
                             % (self.MAX_COMPONENTS, len(off)))
        if not all(math.isfinite(v) for v in off + rat):
            raise ValueError("offsets and ratios must be finite")
        if off[0] != 0. or rat[0] != 1.:
            raise ValueError("offsets[0] must be 0 and ratios[0] must be 1: c and a are the "
                             "first line's centre and amplitude")
        if any(r < 0. for r in rat):
            raise ValueError("ratios must be >= 0")
        if len(set(off)) != len(off):
            raise ValueError("offsets must be distinct")
        self.offsets = tuple(off)
        self.ratios = tuple(rat)

    @classmethod
    def from_rest_wavelengths(cls, cube, rest_wavelengths, ratios, redshift):
        """
        The multiplet of lines at ``rest_wavelengths`` (micrometres, the unit of
        ``Cube.z_step``; the first is the line of ``c``) observed at
        ``redshift`` in ``cube``: offsets ``(l_k - l_0) (1 + z) / cube.z_step``
        channels.  [OII] at z = 0.7 on a MUSE cube (1.25 A channels)::

            >>> import numpy as np
            >>> from deconv3d_amd import MUSE, GaussianMultipletLineModel
            >>> cube = MUSE().build_cube(np.zeros((64, 8, 8)))
            >>> oii = GaussianMultipletLineModel.from_rest_wavelengths(
            ...     cube, [0.372603, 0.372882], [1.0, 1.4], redshift=0.7)
            >>> round(oii.offsets[1], 2)
            3.79
        """
        lam = np.atleast_1d(np.asarray(rest_wavelengths, dtype=np.float64))
        if lam.size == 0:
            raise ValueError("a multiplet has 1 to %d components, got 0" % cls.MAX_COMPONENTS)
        offsets = (lam - lam[0]) * (1. + float(redshift)) / cube.z_step
        return cls(offsets, ratios)

    def parameters(self):
        return ['a', 'c', 'w']

    def gibbs_parameter_index(self):
        return 0

    def min_boundaries(self, runner):
        return [0, 0, 0]

    def max_boundaries(self, runner):
        # the single Gaussian's bounds (lib/line_models.py:79-90): c and a are the first line's
        return SingleGaussianLineModel.max_boundaries(self, runner)

    def modelize(self, runner, x, parameters):
        return self.multiplet(np.asarray(x, dtype=np.float64),
                              parameters[0], parameters[1], parameters[2])

    def multiplet(self, x, a, c, w):
        """``a * sum_k r_k exp(-((x - c) - d_k)^2 / (2 w^2))`` in component order -- the
        order of the device's unit_line (K == 1: SingleGaussianLineModel.gaussian, bit for bit)."""
        s = 0.
        for off, r in zip(self.offsets, self.ratios):
            s = s + r * np.exp(-1. * ((x - c) - off) ** 2 / (2. * w ** 2))
        return a * s


class TabulatedLineModel(GaussianMultipletLineModel):
    """
    Any line of the location-scale family ``a * phi((x - c) / w)``, ``phi`` read from a table
    -- an asymmetric Lyman alpha, Lorentzian wings, a fixed Gauss-Hermite shape, a P-Cygni
    profile -- and, with ``offsets`` / ``ratios`` (the multiplet's rules), a multiplet of it::

        a * sum_k ratios[k] * phi(((x - c) - offsets[k]) / w)

    ``profile``: 8 to 65537 samples of ``phi`` on the uniform grid ``u_j = -support + j h``,
    ``h = 2 support / (n - 1)``; the constructor divides them by the sample of largest
    magnitude, which must be positive, so that the peak is 1 and ``a`` stays the peak
    amplitude.  Negative lobes are allowed; non-finite samples, an all-zero table or a
    ``support`` that is not finite and > 0 raise ``ValueError``.  The parameters, the Gibbs
    index and the bounds are those of ``SingleGaussianLineModel``; the device kernels evaluate
    the line themselves (``d3d_set_line_table``).

    The curve IS the interpolant (:meth:`phi`): the Catmull-Rom cubic through the table padded
    with one zero on each side, 0 beyond the support.  ``flux_factor``: the trapezoid integral
    of the normalised table times ``sum(ratios)`` -- the integrated flux is
    ``F = a w flux_factor``.
    """

    MIN_SAMPLES, MAX_SAMPLES = 8, 65537

    def __init__(self, profile, support, offsets=(0.,), ratios=(1.,)):
        GaussianMultipletLineModel.__init__(self, offsets, ratios)
        try:
            tab = np.array(profile, dtype=np.float64)
            support = float(support)
        except (TypeError, ValueError):
            raise ValueError("profile must be a sequence of numbers and support a number")
        if tab.ndim != 1:
            raise ValueError("profile must be one-dimensional, got shape %s" % (tab.shape,))
        if not self.MIN_SAMPLES <= tab.size <= self.MAX_SAMPLES:
            raise ValueError("a line table has %d to %d samples, got %d"
                             % (self.MIN_SAMPLES, self.MAX_SAMPLES, tab.size))
        if not (math.isfinite(support) and support > 0.):
            raise ValueError("support must be finite and > 0, got %r" % support)
        if not np.isfinite(tab).all():
            raise ValueError("profile samples must be finite")
        peak = tab[np.argmax(np.abs(tab))]
        if peak == 0.:
            raise ValueError("profile is zero everywhere")
        if peak < 0.:
            raise ValueError("the sample of largest magnitude must be positive (a is the peak "
                             "amplitude), got %g" % peak)
        tab = tab / peak
        tab.setflags(write=False)
        self.table = tab
        self.support = support
        self.inv_h = (tab.size - 1) / (2. * support)
        padded = np.zeros(tab.size + 2)
        padded[1:-1] = tab
        self._padded = padded
        h = 2. * support / (tab.size - 1)
        # (integral of phi alone: what d3d_set_line_table takes; the device multiplies by the ratios)
        self.table_integral = float(h * (np.sum(tab) - 0.5 * (tab[0] + tab[-1])))
        self.flux_factor = self.table_integral * float(sum(self.ratios))

    @classmethod
    def from_function(cls, phi, support, samples=2049, **kw):
        """The table of ``samples`` values of the callable ``phi`` on ``[-support, support]``."""
        samples = int(samples)
        if samples < 2:
            raise ValueError("a line table has %d to %d samples, got %d"
                             % (cls.MIN_SAMPLES, cls.MAX_SAMPLES, samples))
        u = -float(support) + np.arange(samples) * (2. * float(support) / (samples - 1))
        return cls(np.array([phi(v) for v in u], dtype=np.float64), support, **kw)

    def phi(self, d, w):
        """``phi(d / w)``: the interpolant, one IEEE double operation per step in the order of
        the device's table_line (d3d_kernels.h).  ``w == 0``: the value at 0 where ``d == 0``,
        0 elsewhere (unit_gaussian's delta rule); NaN and anything beyond the support: 0."""
        d = np.asarray(d, dtype=np.float64)
        n = self.table.size
        with np.errstate(all="ignore"):
            if w != 0.:
                u = d / w
            else:
                u = np.where(d == 0., 0., np.nan)
            t = (u + self.support) * self.inv_h
            inside = (t >= 0.) & (t <= n - 1)
            tt = np.where(inside, t, 0.)
            j = np.minimum(np.floor(tt).astype(np.int64), n - 2)
            s = tt - j
            p = self._padded
            p0, p1, p2, p3 = p[j], p[j + 1], p[j + 2], p[j + 3]
            v = p1 + 0.5 * s * ((p2 - p0) + s * ((2. * p0 - 5. * p1 + 4. * p2 - p3)
                                                 + s * (3. * (p1 - p2) + (p3 - p0))))
        return np.where(inside, v, 0.)

    def modelize(self, runner, x, parameters):
        return self.tabulated(np.asarray(x, dtype=np.float64),
                              parameters[0], parameters[1], parameters[2])

    def tabulated(self, x, a, c, w):
        """``a * sum_k r_k phi(((x - c) - d_k) / w)`` in component order -- the order of the
        device's unit_line."""
        s = 0.
        for off, r in zip(self.offsets, self.ratios):
            s = s + r * self.phi((x - c) - off, w)
        return a * s

    def digest(self):
        """SHA-256 over ``n``, ``support`` and the sample bytes: what a checkpoint records."""
        h = hashlib.sha256()
        h.update(struct.pack("<qd", self.table.size, self.support))
        h.update(np.ascontiguousarray(self.table, dtype="<f8").tobytes())
        return h.hexdigest()


SINGLE_LINE_SHAPE = ((0.,), (1.,))


def model_is_on_device(model):
    """True when the HIP kernels evaluate ``model`` themselves:
    ``SingleGaussianLineModel``, ``GaussianMultipletLineModel`` or ``TabulatedLineModel`` (subclasses may change
    names and bounds, but not the curve, the jump hook or the Gibbs index).  Any other
    LineModel plugin is evaluated on the host (host_model.HostModelChain)."""
    if isinstance(model, TabulatedLineModel):
        curve = (type(model).modelize is TabulatedLineModel.modelize
                 and type(model).tabulated is TabulatedLineModel.tabulated
                 and type(model).phi is TabulatedLineModel.phi)
    elif isinstance(model, GaussianMultipletLineModel):
        curve = (type(model).modelize is GaussianMultipletLineModel.modelize
                 and type(model).multiplet is GaussianMultipletLineModel.multiplet)
    elif isinstance(model, SingleGaussianLineModel):
        curve = (type(model).modelize is SingleGaussianLineModel.modelize
                 and type(model).gaussian is SingleGaussianLineModel.gaussian)
    else:
        return False
    return (curve
            and type(model).post_jump is LineModel.post_jump
            and model.gibbs_parameter_index() == 0
            and len(model.parameters()) == 3)


def device_line_shape(model):
    """(offsets, ratios) of the device's unit line for a model that runs on the device."""
    # (the very attributes modelize sums over: the device cannot disagree with the host curve)
    if isinstance(model, GaussianMultipletLineModel):
        return tuple(model.offsets), tuple(model.ratios)
    return SINGLE_LINE_SHAPE


def device_line_table(model):
    """(table, support, flux_factor) of ``Engine.set_line_table`` for a model that runs on the
    device -- the normalised samples, their support and the integral of phi -- or None for a
    model of Gaussians."""
    # (the very table modelize interpolates: the device cannot disagree with the host curve)
    if isinstance(model, TabulatedLineModel):
        return model.table, model.support, model.table_integral
    return None
