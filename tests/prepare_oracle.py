"""
CPU restatement of the cube preparation of include/deconv3d_hip.h (d3d_running_median,
d3d_channel_stats, d3d_prepare) and of deconv3d_amd.prepare's variance step, in numpy, and the
planted raw cube the tests share: test infrastructure only, the package never imports it.
"""
import warnings

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import deconv3d_oracle as O


def _nanmedian(a, axis):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (an all-NaN slice is NaN)
        return np.nanmedian(a, axis=axis)


def running_median(cube, valid, h):
    """RM(cube, valid, h): the NaN-padded sliding window along z, np.nanmedian of it.
    ``valid=None``: the finite voxels."""
    cube = np.asarray(cube, dtype=np.float64)
    valid = np.isfinite(cube) if valid is None else (np.asarray(valid) != 0) & ~np.isnan(cube)
    x = np.where(valid, cube, np.nan)
    pad = np.full((h,) + cube.shape[1:], np.nan)
    win = sliding_window_view(np.concatenate([pad, x, pad], axis=0), 2 * h + 1, axis=0)
    return _nanmedian(win, -1)


def channel_stats(cube, select=None):
    """CS(cube, select) = (m, mad, n) per channel."""
    cube = np.asarray(cube, dtype=np.float64)
    D = cube.shape[0]
    keep = np.isfinite(cube)
    if select is not None:
        keep = keep & (np.asarray(select) != 0)[None]
    x = np.where(keep, cube, np.nan).reshape(D, -1)
    n = keep.reshape(D, -1).sum(axis=1).astype(np.int64)
    m = _nanmedian(x, 1)
    with np.errstate(invalid="ignore"):
        mad = _nanmedian(np.abs(x - m[:, None]), 1)
    return m, mad, n


def sigma_of(mad, n):
    return np.where((n < 2) | (mad == 0.), np.nan, 1.4826 * mad)


def prepare(cube, select, h, reject):
    """(continuum, residual, m, sigma, n) of the preparation contract."""
    cube = np.asarray(cube, dtype=np.float64)
    valid0 = np.isfinite(cube)
    with np.errstate(invalid="ignore"):
        cont = running_median(cube, valid0, h)
        res = cube - cont
        m, mad, n = channel_stats(res, select)
        sigma = sigma_of(mad, n)
        if reject is not None:
            inside = np.isnan(sigma)[:, None, None] | (np.abs(res) <= (reject * sigma)[:, None, None])
            cont = running_median(cube, valid0 & inside, h)
            res = cube - cont
            m, mad, n = channel_stats(res, select)
            sigma = sigma_of(mad, n)
    return cont, res, m, sigma, n


def variance(sigma, shape, given=None, select=None):
    """sigma_z**2 on every plane, 1e12 where sigma is NaN; with ``given`` (rescale=True):
    given[z] * sigma_z**2 / CS(given, select).m_z, the channel unchanged where either factor is
    NaN or zero."""
    s2 = sigma ** 2
    if given is None:
        return np.ones(shape) * np.where(np.isnan(sigma), 1e12, s2)[:, None, None]
    m = channel_stats(given, select)[0]
    out = np.array(given, dtype=np.float64)
    for z in range(shape[0]):
        if not (np.isnan(s2[z]) or np.isnan(m[z]) or s2[z] == 0. or m[z] == 0.):
            out[z] = given[z] * s2[z] / m[z]
    return out


class Planted(object):
    """The raw cube of the tests: narrow lines under a Gaussian FSF (FWHM 3) and LSF (sigma
    0.9088), a channel-dependent noise factor 1 + 2 U, a continuum 20 sigma U + (U - 0.5) 0.5
    sigma z per spaxel, the spectrum at (0, 0) all NaN and one more NaN voxel; the noise mask
    is r^2 > (H / 3)^2."""

    def __init__(self, D=96, H=12, W=12, seed=11):
        rng = np.random.default_rng(seed)
        self.fsf = O.gaussian_fsf_image(3.0)
        self.lsf = O.gaussian_lsf_vector(D, 0.9088)
        y, x = np.indices((H, W))
        r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
        a = 10. * np.exp(-r2 / (2. * (H / 5.) ** 2))
        c = D / 2. + (D / 8.) * np.tanh((x - W / 2.) / (W / 8.))
        w = rng.uniform(1., 1.8, size=(H, W))
        self.truth = np.dstack((a, c, w))
        self.mask = np.ones((H, W))
        self.clean = O.forward_full((D, H, W), self.truth, self.mask, self.fsf, self.lsf)
        self.sigma0 = 0.05 * 10. * np.max(self.fsf)
        self.factor = 1. + 2. * rng.random(D)
        self.sigma = self.sigma0 * self.factor                       # true per-channel sigma
        noise = rng.normal(0., 1., size=(D, H, W)) * self.sigma[:, None, None]
        z = np.arange(D, dtype=np.float64)[:, None, None]
        self.continuum = (20. * self.sigma0 * rng.random((H, W))[None]
                          + (rng.random((H, W))[None] - 0.5) * 0.5 * self.sigma0 * z)
        self.line_cube = self.clean + noise                          # continuum-free, true variance
        self.true_variance = np.ones((D, H, W)) * (self.sigma ** 2)[:, None, None]
        self.raw = self.line_cube + self.continuum
        self.raw[:, 0, 0] = np.nan
        self.raw[D // 3, H // 2, W // 2 + 1] = np.nan
        self.noise_mask = (r2 > (H / 3.) ** 2).astype(np.uint8)
        self.shape = (D, H, W)
