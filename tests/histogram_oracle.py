"""
Numpy restatement of the posterior histograms' contract (include/deconv3d_hip.h: d3d_hist_*;
DESIGN.md section 8g): every floating-point step is one IEEE double operation in the order the
kernels take it, so that counters compare as integers and the extracted maps to a few roundings.
Test infrastructure only.

A SERIES is one (spaxel, quantity) pair; the arrays carry the quantities (a, c, w, F) on their
last axis, as the map of d3d_post_get.
"""
import numpy as np

BINS = 64


def flux_factor(ratios):
    """F = (a w) flux_k: sqrt(2 pi) times the ratios summed from 0 in their order."""
    total = 0.0
    for r in np.asarray(ratios, dtype=np.float64).reshape(-1):
        total += float(r)
    return float(np.sqrt(2.0 * np.pi)) * total


def series(params, flux_k):
    """(..., 3) parameters -> (..., 4): a, c, w, F = (a w) flux_k."""
    params = np.asarray(params, dtype=np.float64)
    a, w = params[..., 0], params[..., 2]
    return np.concatenate((params, ((a * w) * flux_k)[..., None]), axis=-1)


def bounds(min_b, max_b, flux_k):
    """(L, U) of the four quantities."""
    min_b, max_b = np.asarray(min_b, dtype=np.float64), np.asarray(max_b, dtype=np.float64)
    L = np.append(min_b, min_b[0] * min_b[2] * flux_k)
    U = np.append(max_b, max_b[0] * max_b[2] * flux_k)
    return L, U


def welford(samples):
    """(mean, M2) of samples (n, ...) by the recurrence of the device's moments."""
    mean = np.zeros(samples.shape[1:])
    m2 = np.zeros(samples.shape[1:])
    for n, m in enumerate(np.asarray(samples, dtype=np.float64), 1):
        delta = m - mean
        mean = mean + delta / float(n)
        m2 = m2 + delta * (m - mean)
    return mean, m2


def freeze(mean, m2, pilot, span, L, U, mask=None):
    """(lo, hi) of every series from the moments of the first `pilot` samples; NaN where masked."""
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(m2 / float(pilot - 1))
        half = span * sd
        lo, hi = mean - half, mean + half
        lo = np.where(lo > L, lo, L)
        hi = np.where(hi < U, hi, U)
        whole = ~(sd > 0.0) | ~(hi > lo)
    lo, hi = np.where(whole, L, lo), np.where(whole, U, hi)
    if mask is not None:
        dead = np.asarray(mask) != 1
        lo[dead] = np.nan
        hi[dead] = np.nan
    return lo, hi


def count(samples, lo, hi):
    """Bin samples (n, ..., 4) into ranges (..., 4): (bins (..., 4, 64), tails (..., 4, 2)) uint32.
    A series whose range has !(hi > lo) -- NaN, or coinciding bounds -- is never counted."""
    samples = np.asarray(samples, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = hi > lo
    bins = np.zeros(lo.shape + (BINS,), dtype=np.uint32)
    tails = np.zeros(lo.shape + (2,), dtype=np.uint32)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = float(BINS) / (hi - lo)
    for v in samples:
        with np.errstate(invalid="ignore"):
            b = np.floor((v - lo) * scale)
            under, over = live & (b < 0.0), live & (b >= float(BINS))
            inside = live & (b >= 0.0) & (b < float(BINS))
        tails[..., 0] += under
        tails[..., 1] += over
        where = np.nonzero(inside)
        np.add.at(bins, where + (b[where].astype(np.int64),), 1)
    return bins, tails


def _parts(bins, tails, rng):
    cnt = np.asarray(bins).astype(np.int64)
    below, above = np.asarray(tails)[..., 0].astype(np.int64), np.asarray(tails)[..., 1].astype(np.int64)
    cum = np.cumsum(cnt, axis=-1)
    lo, hi = rng[..., 0], rng[..., 1]
    return cnt, cum, below, above, below + cum[..., -1] + above, lo, hi, (hi - lo) / float(BINS)


def quantile(bins, tails, rng, q):
    """Quantile q of every histogram: NaN for an empty one, lo / hi when q n falls in a tail, else
    linear inside the first bin b with below + cum[b] >= q n."""
    cnt, cum, below, above, n, lo, hi, width = _parts(bins, tails, rng)
    t = q * n.astype(np.float64)
    crossed = (below[..., None] + cum).astype(np.float64) >= t[..., None]
    b = np.argmax(crossed, axis=-1)
    cum_b = np.take_along_axis(cum, b[..., None], axis=-1)[..., 0]
    cnt_b = np.take_along_axis(cnt, b[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = lo + (b.astype(np.float64) + (t - (below + cum_b - cnt_b).astype(np.float64))
                  / cnt_b.astype(np.float64)) * width
    r = np.where(t > (n - above).astype(np.float64), hi, r)
    r = np.where(t <= below.astype(np.float64), lo, r)
    return np.where(n == 0, np.nan, r)


def mode(bins, tails, rng):
    """Centre of the lowest bin with the largest count; NaN when every bin is empty."""
    cnt, cum, _, _, _, lo, _, width = _parts(bins, tails, rng)
    b = np.argmax(cnt, axis=-1)
    with np.errstate(invalid="ignore"):
        m = lo + (b.astype(np.float64) + 0.5) * width
    return np.where(cum[..., -1] == 0, np.nan, m)


def outside(bins, tails, rng):
    """(below + above) / n; NaN for an empty histogram."""
    _, _, below, above, n, _, _, _ = _parts(bins, tails, rng)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n == 0, np.nan, (below + above).astype(np.float64) / n.astype(np.float64))
