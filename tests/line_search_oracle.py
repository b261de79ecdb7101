"""
CPU restatement of the matched-filter statistic of d3d_line_search (include/deconv3d_hip.h),
built from the oracle's line and LSF: test infrastructure only, the package never imports it.
"""
import numpy as np

from oracle import deconv3d_oracle as O


def default_grid(D):
    """The defaults of deconv3d_amd.search restated: integer channels, 8 geometric widths."""
    return np.arange(D, dtype=np.float64), np.geomspace(0.75, max(D / 6., 1.5), 8)


def template_bank(D, lsf, centres, widths, model=None):
    """[n_w * n_c][D]: the LSF-convolved unit line at (centres[i_c], widths[i_w]), row
    i_w * n_c + i_c; ``model``: a LineModel whose modelize gives the line (default: the
    oracle's Gaussian)."""
    x = np.arange(D, dtype=np.float64)
    rows = []
    for w in widths:
        for c in centres:
            line = O.gaussian_line(x, 1., c, w) if model is None else \
                np.asarray(model.modelize(None, x, [1., c, w]), dtype=np.float64)
            rows.append(O.spectral_convolve(line, lsf))
    return np.array(rows)


def prepare(data, var):
    """(d, iv) as d3d_set_data leaves them: NaN voxel -> d = 0, iv = 0; zero variance -> 1e12."""
    nan = np.isnan(data)
    d = np.where(nan, 0., data)
    v = np.where(var == 0., 1e12, var)
    return d, np.where(nan, 0., 1. / v)


def statistic(data, var, mask, bank, n_c):
    """(best (H,W) int32, stat (H,W,4), gap): the statistic of the header, and the smallest
    relative gap between the best and the second-best valid candidate of any detected spaxel
    (inf when every detected spaxel has one valid candidate)."""
    D, H, W = data.shape
    d, iv = prepare(data, np.broadcast_to(var, data.shape))
    X = (d * iv).reshape(D, H * W)
    V = iv.reshape(D, H * W)
    N = bank @ X
    Q = (bank * bank) @ V
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(Q > 0., N / np.sqrt(Q), 0.)
    valid = (Q > 0.) & (N > 0.)
    sv = np.where(valid, s, -np.inf)
    best = np.argmax(sv, axis=0)                    # (first maximum: the lowest k)
    found = valid.any(axis=0) & (np.asarray(mask).reshape(-1) == 1)
    n_cand = bank.shape[0]
    stat = np.zeros((H * W, 4))
    gap = np.inf
    for p in np.nonzero(found)[0]:
        k = best[p]
        ic = k % n_c
        stat[p] = (N[k, p], Q[k, p],
                   s[k - 1, p] if ic > 0 else np.nan,
                   s[k + 1, p] if ic + 1 < n_c else np.nan)
        if n_cand > 1:
            others = np.delete(sv[:, p], k)
            second = others.max()
            if np.isfinite(second):
                gap = min(gap, (sv[k, p] - second) / sv[k, p])
    best = np.where(found, best, -1).astype(np.int32)
    return best.reshape(H, W), stat.reshape(H, W, 4), gap
