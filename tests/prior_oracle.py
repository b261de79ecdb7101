# coding=utf-8
"""
Helper (not a test): the oracle's MH-within-Gibbs update with the smoothness prior between
4-neighbours of include/deconv3d_hip.h: d3d_prior_begin,

    log p(theta) = -1/2 sum_<i,j> sum_k lam_k (theta_i,k - theta_j,k)^2,   k = (a, c, w),

over the adjacent pairs of spaxels with mask == 1.  ``mh_update`` restates
``oracle.mh_update`` (lib/run.py:369-519) line by line, with the oracle's own
``window_limits``, ``local_contribution``, ``half_chi2``, ``philox_pair`` and
``truncated_normal``, and changes it in two places: the prior's term of the log acceptance
ratio (lib/run.py:426-438) and of the amplitude's conditional (lib/run.py:491-496).  With
``lam = 0`` both terms are exact zeros and the update is the oracle's, bit for bit.
"""
import math

import numpy as np

from oracle import deconv3d_oracle as O


def neighbours(mask, y, x):
    """N(i): the 4-neighbours of (y, x) inside the map with mask == 1 (up, down, left, right)."""
    H, W = mask.shape
    out = []
    for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
        if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] == 1:
            out.append((ny, nx))
    return out


def energy(params, mask):
    """(E_a, E_c, E_w, pairs): sums of squared differences over the horizontally and vertically
    adjacent pairs of spaxels with mask == 1, and the number of pairs."""
    p = np.asarray(params, dtype=np.float64)
    m = np.asarray(mask) == 1
    e = np.zeros(3)
    pairs = 0
    for a, b, ma, mb in ((p[:, :-1], p[:, 1:], m[:, :-1], m[:, 1:]),
                         (p[:-1, :], p[1:, :], m[:-1, :], m[1:, :])):
        both = ma & mb
        d = (a - b)[both]
        e += np.sum(d * d, axis=0) if d.size else 0.
        pairs += int(np.sum(both))
    return float(e[0]), float(e[1]), float(e[2]), pairs


def mh_update(st, y, x, sweep, lam):
    """oracle.mh_update with the prior of weights lam = (lam_a, lam_c, lam_w).  The neighbours'
    parameters are those of ``st.params`` now: the time of the decision."""
    lam = np.asarray(lam, dtype=np.float64)
    D, H, W = st.data.shape
    fh, fw = st.fsf.shape
    gy0, gx0, Wg = st.origin
    sp = (y + gy0) * Wg + (x + gx0)
    p_old = st.params[y, x].copy()

    ua, uc = O.philox_pair(st.seed, sp, sweep, O.BLK_JUMP_AC)
    uw, uacc = O.philox_pair(st.seed, sp, sweep, O.BLK_JUMP_W)
    u = np.array([ua, uc, uw])
    p_new = p_old + st.amp * np.tan(np.pi * (u - 0.5))
    oob = bool((p_new < st.min_b).any() or (p_new > st.max_b).any())

    (y0, y1, x0, x1), (ly0, ly1, lx0, lx1) = O.window_limits(y, x, H, W, fh, fw)
    c_new = O.local_contribution(p_new, D, st.fsf, st.lsf)[:, ly0:ly1, lx0:lx1]
    c_old = O.local_contribution(p_old, D, st.fsf, st.lsf)[:, ly0:ly1, lx0:lx1]
    e_old = st.err[:, y0:y1, x0:x1]
    v = st.var[:, y0:y1, x0:x1]

    ul = e_old + c_old
    e_new = ul - c_new
    ar_old = O.half_chi2(e_old, v)
    ar_new = O.half_chi2(e_new, v)
    # ---- the prior's term of the ratio: the amplitude does not move in the proposal ----
    nb = [st.params[ny, nx] for ny, nx in neighbours(st.mask, y, x)]
    prior = 0.
    for theta in nb:
        for k in (1, 2):
            prior += lam[k] * (p_new[k] - p_old[k]) * (p_new[k] + p_old[k] - 2. * theta[k])
    delta = (ar_old - ar_new) - 0.5 * prior
    st.dlog[y, x] = delta

    accepted = (math.log(uacc) < delta) and not oob
    p_end = p_new.copy() if accepted else p_old.copy()
    if accepted:
        st.accepted += 1

    p_one = p_end.copy()
    p_one[0] = 1.
    ek = O.local_contribution(p_one, D, st.fsf, st.lsf)[:, ly0:ly1, lx0:lx1]
    _, _, s_ee, s_eu = O.gibbs_moments(ek, ul, v, st.ra)
    # ---- the prior's term of the amplitude's conditional ----
    s_ee = s_ee + lam[0] * len(nb)
    s_eu = s_eu + lam[0] * sum(theta[0] for theta in nb)
    ro = st.ra / (1. + st.ra * s_ee)
    mu = ro * s_eu
    blk = [O.BLK_GIBBS]

    def draw():
        pair = O.philox_pair(st.seed, sp, sweep, blk[0])
        blk[0] += 1
        return pair

    r = O.truncated_normal(st.min_b[0], st.max_b[0], mu, math.sqrt(ro), draw)
    p_end[0] = r
    st.err[:, y0:y1, x0:x1] = ul - ek * r
    st.params[y, x] = p_end
    st.last = (p_old, p_end.copy())
    return accepted


def mh_sweep(st, sweep, lam, order=None):
    """One sweep in device colour order (or a given order), as oracle.mh_sweep."""
    fh, fw = st.fsf.shape
    if order is None:
        order = O.colour_order(st.mask, fh, fw)
    n = 0
    for (y, x) in order:
        mh_update(st, y, x, sweep, lam)
        n += 1
    return n
