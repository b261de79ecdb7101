"""
The tabulated line a * sum_k r_k phi(((x - c) - d_k) / w) restated for the tests, element by
element in plain Python floats (IEEE doubles) and independently of TabulatedLineModel.modelize:
the Catmull-Rom cubic through the table padded with one zero on each side, 0 beyond the support.
Test infrastructure only.
"""
import math

import numpy as np


def profile_G():
    """Gaussian exp(-u^2/2): n = 2049, support 8."""
    u = np.linspace(-8., 8., 2049)
    return np.exp(-u ** 2 / 2.), 8.


def profile_S():
    """Skewed exp(-u^2/2) (1 + erf(2u/sqrt 2)): n = 1025, support 6 (a mirrored u fails on it)."""
    u = np.linspace(-6., 6., 1025)
    return np.exp(-u ** 2 / 2.) * (1. + np.array([math.erf(2. * v / math.sqrt(2.)) for v in u])), 6.


def profile_L():
    """Lorentzian 1/(1+u^2): n = 4097, support 40 (reaches past the cube and past the support)."""
    u = np.linspace(-40., 40., 4097)
    return 1. / (1. + u ** 2), 40.


def profile_C():
    """8 coarse samples with negative lobes, support 3.5."""
    return np.array([0., -0.3, 0.2, 1., 0.6, 0.1, -0.1, 0.]), 3.5


PROFILES = {"G": profile_G, "S": profile_S, "L": profile_L, "C": profile_C}


def normalised(profile):
    """The table divided by its sample of largest magnitude."""
    tab = [float(v) for v in profile]
    peak = max(tab, key=abs)
    return [v / peak for v in tab]


def phi_scalar(tab, support, d, w):
    """phi(d / w) for one pair of floats; tab: the normalised samples (a list)."""
    n = len(tab)
    inv_h = (n - 1) / (2. * support)
    if w != 0.:             # (NaN included: the comparisons below are then false)
        u = d / w
    elif d == 0.:
        u = 0.
    else:
        return 0.
    t = (u + support) * inv_h
    if not (0. <= t <= n - 1):
        return 0.
    j = int(math.floor(t))
    if j > n - 2:
        j = n - 2
    s = t - j

    def sample(i):
        return tab[i] if 0 <= i < n else 0.

    p0, p1, p2, p3 = sample(j - 1), sample(j), sample(j + 1), sample(j + 2)
    a3 = 3. * (p1 - p2) + (p3 - p0)
    a2 = 2. * p0 - 5. * p1 + 4. * p2 - p3
    a1 = p2 - p0
    return p1 + 0.5 * s * (a1 + s * (a2 + s * a3))


def line(profile, support, offsets=(0.,), ratios=(1.,)):
    """The oracle's line(x, a, c, w) of the table (what O.gaussian_line is patched with)."""
    tab = normalised(profile)
    offsets = [float(v) for v in offsets]
    ratios = [float(v) for v in ratios]

    def f(x, a, c, w):
        x = np.asarray(x, dtype=np.float64)
        a, c, w = float(a), float(c), float(w)
        out = np.empty(x.shape)
        flat_x, flat_o = x.reshape(-1), out.reshape(-1)
        for i in range(flat_x.size):
            s = 0.
            for off, r in zip(offsets, ratios):
                s = s + r * phi_scalar(tab, support, (float(flat_x[i]) - c) - off, w)
            flat_o[i] = a * s
        return out if out.ndim else float(out)
    return f


def trapezoid(profile, support):
    """Trapezoid integral of the normalised table over [-support, support]."""
    tab = normalised(profile)
    h = 2. * support / (len(tab) - 1)
    return h * (math.fsum(tab) - 0.5 * (tab[0] + tab[-1]))
