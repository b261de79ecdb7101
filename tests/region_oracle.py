"""
Numpy restatement of the region posteriors' contract (include/deconv3d_hip.h, "region posteriors"):
the members of a region, the order of every sum, the two-pass width and the Welford fold.  Every
step is one IEEE double operation in the written order, so (F, C, S) are the device's bit for bit.
Test infrastructure only.
"""
import numpy as np

CHUNK = 64


def members(labels, mask, K):
    """Per region k = 1..K the flat indices of its unmasked spaxels in row-major order."""
    lab = np.asarray(labels).reshape(-1)
    live = np.asarray(mask).reshape(-1) == 1
    return [np.flatnonzero((lab == k) & live) for k in range(1, K + 1)]


def fold_by_halves(terms):
    """A chunk's partial: its (at most 64) terms, absent ones +0.0, folded v[:32] + v[32:], then 16, ... 1."""
    v = np.zeros(CHUNK)
    v[:len(terms)] = terms
    n = CHUNK // 2
    while n >= 1:
        v = v[:n] + v[n:2 * n]
        n //= 2
    return v[0]


def chunked_sum(terms):
    """A region's scalar sum: chunk partials by halves, the partials one after the other from +0.0."""
    acc = np.float64(0.0)
    for m in range(0, len(terms), CHUNK):
        acc = acc + fold_by_halves(terms[m:m + CHUNK])
    return acc


def scalars(params, labels, mask, K, flux_k):
    """(K, 3) = (F, C, S) of one sample: params (H, W, 3), F_i = (a_i w_i) flux_k."""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 3)
    out = np.empty((K, 3))
    with np.errstate(all="ignore"):
        for k, idx in enumerate(members(labels, mask, K)):
            a, c, w = p[idx, 0], p[idx, 1], p[idx, 2]
            Fi = (a * w) * flux_k
            F = chunked_sum(Fi)
            if F == 0.0:
                out[k] = (0.0, np.nan, np.nan)
                continue
            C = chunked_sum(Fi * c) / F
            d = c - C
            S = np.sqrt(chunked_sum(Fi * (w * w + d * d)) / F)
            out[k] = (F, C, S)
    return out


def series(chain, labels, mask, K, flux_k):
    """(n, K, 3): scalars of every sample of ``chain`` (n, H, W, 3)."""
    return np.stack([scalars(p, labels, mask, K, flux_k) for p in chain])


def spectra(params, labels, mask, K, D, unit_line):
    """(K, D): s_k(z) = sum_i a_i unit_line(z, c_i, w_i) -- per chunk the members one after the other
    from +0.0, the chunk partials one after the other from +0.0.  ``unit_line(z, c, w)``: the model's
    unit profile over the channel vector z."""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 3)
    z = np.arange(D, dtype=np.float64)
    out = np.zeros((K, D))
    for k, idx in enumerate(members(labels, mask, K)):
        total = np.zeros(D)
        for m in range(0, len(idx), CHUNK):
            part = np.zeros(D)
            for i in idx[m:m + CHUNK]:
                part = part + p[i, 0] * unit_line(z, p[i, 1], p[i, 2])
            total = total + part
        out[k] = total
    return out


def welford(samples):
    """(mean, M2) of a stack of samples (n, ...), folded one after the other from zeros."""
    mean = np.zeros(samples[0].shape)
    m2 = np.zeros(samples[0].shape)
    for n, s in enumerate(samples, 1):
        delta = s - mean
        mean = mean + delta / n
        m2 = m2 + delta * (s - mean)
    return mean, m2


def gaussian_unit_line(offsets=(0.,), ratios=(1.,)):
    """unit_line of K Gaussians of one centre and width (the device's unit_line, MULTI or not)."""
    def line(z, c, w):
        w2 = 2.0 * w * w
        s = np.zeros_like(z)
        for off, ratio in zip(offsets, ratios):
            d = (z - c) - off
            g = np.exp(-(d * d) / w2)
            s = s + ratio * g if len(offsets) > 1 else g
        return s
    return line
