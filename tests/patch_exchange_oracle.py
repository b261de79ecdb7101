"""
Numpy restatement of the exchange of PATCHES of spaxels between tempered rungs
(include/deconv3d_hip.h: d3d_temper_set_patch) on top of tests/tempering_oracle.py and oracle/:
the tiles of a round and their colours, the difference cube delta of a patch, the five terms of
the log ratio, the uniforms, and the exchange itself.  Test infrastructure only.
"""
import math

import numpy as np

from oracle import deconv3d_oracle as O
from tests import prior_oracle as PO
from tests import tempering_oracle as TO


# ---- tiles and colours ----------------------------------------------------------------------------

def origin_shift(seed, round_, p):
    """(oy, ox) = (w0 mod p, w1 mod p), w = Philox4x32-10 at {0xFFFFFFFE, round, 0, 1}."""
    w = O.philox4x32_10((0xFFFFFFFE, int(round_) & 0xFFFFFFFF, 0, 1),
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return int(w[0]) % p, int(w[1]) % p


def tile_counts(H, W, p, oy, ox):
    return (H - 1 + p - oy) // p + 1, (W - 1 + p - ox) // p + 1


def colour_counts(fh, fw, p):
    """my, mx = 1 + ceil((fh - 1) / p), 1 + ceil((fw - 1) / p)."""
    return 1 + -(-(fh - 1) // p), 1 + -(-(fw - 1) // p)


def tile_of(y, x, p, oy, ox):
    return (y + p - oy) // p, (x + p - ox) // p


def tile_rect(ty, tx, p, oy, ox, H, W):
    """(y0, y1, x0, x1) of tile (ty, tx) clipped to the field (possibly empty)."""
    return (max(0, ty * p - p + oy), min(H, ty * p + oy), max(0, tx * p - p + ox), min(W, tx * p + ox))


def footprint(rect, fh, fw, H, W):
    """The tile dilated by the FSF's half sizes, clipped to the field."""
    fhh, fhw = (fh - 1) // 2, (fw - 1) // 2
    y0, y1, x0, x1 = rect
    return max(0, y0 - fhh), min(H, y1 + fhh), max(0, x0 - fhw), min(W, x1 + fhw)


def colour_schedule(nty, ntx, my, mx):
    """The tiles of a round, one list per colour, in ascending cy * mx + cx."""
    return [[(ty, tx) for ty in range(cy, nty, my) for tx in range(cx, ntx, mx)]
            for cy in range(my) for cx in range(mx)]


def patch_of(mask, rect):
    y0, y1, x0, x1 = rect
    return [(y, x) for y in range(y0, y1) for x in range(x0, x1) if mask[y, x] == 1]


def patch_uniform(seed, round_, i, tile):
    """The ``.x`` uniform of Philox at {0xFFFFFFFF, round, i, 2 + tile}."""
    r = O.philox4x32_10((0xFFFFFFFF, int(round_) & 0xFFFFFFFF, i, (2 + tile) & 0xFFFFFFFF),
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return O.u64_to_unit((r[1] << 32) | r[0])


# ---- delta and the five terms ---------------------------------------------------------------------

def contribution(st, y, x, params, line=None):
    """O.contribution_of_spaxel; ``line(x, a, c, w)`` replaces the single Gaussian."""
    D, H, W = st.data.shape
    if line is None:
        return O.contribution_of_spaxel(x, y, params, W, H, D, st.fsf, st.lsf)
    conv = O.spectral_convolve(line(np.arange(D), params[0], params[1], params[2]), st.lsf)
    local = st.fsf * conv[:, None, None]
    (y0, y1, x0, x1), (ly0, ly1, lx0, lx1) = O.window_limits(y, x, H, W, st.fsf.shape[0], st.fsf.shape[1])
    sim = np.zeros((D, H, W))
    sim[:, y0:y1, x0:x1] = local[:, ly0:ly1, lx0:lx1]
    return sim


def patch_delta(si, sj, patch, line=None):
    """delta = sum_{s in P} [contribution(s, x_i[s]) - contribution(s, x_j[s])], a whole cube."""
    delta = np.zeros(si.data.shape)
    for (y, x) in patch:
        delta += contribution(si, y, x, si.params[y, x], line) - contribution(sj, y, x, sj.params[y, x], line)
    return delta


def ivar_of(st):
    """The rung's own 1/variance, 0 at NaN voxels (d3d_set_data)."""
    return np.where(np.isnan(st.data), 0., 1. / st.var)


def residual_of(st):
    return np.where(np.isnan(st.data), 0., st.err)


def prior_term(pi, pj, mask, rect, lam):
    """Delta_prior over the pairs <s, t>, s in the patch, t unmasked outside the tile."""
    if lam is None:
        return 0., 0.
    y0, y1, x0, x1 = rect
    total = mag = 0.
    for (y, x) in patch_of(mask, rect):
        for (ny, nx) in PO.neighbours(mask, y, x):
            if y0 <= ny < y1 and x0 <= nx < x1:
                continue
            for k in range(3):
                parts = ((pj[y, x, k] - pi[ny, nx, k]) ** 2, -(pi[y, x, k] - pi[ny, nx, k]) ** 2,
                         (pi[y, x, k] - pj[ny, nx, k]) ** 2, -(pj[y, x, k] - pj[ny, nx, k]) ** 2)
                total += lam[k] * math.fsum(parts)
                mag += abs(lam[k]) * sum(abs(v) for v in parts)
    return -0.5 * total, 0.5 * mag


def five_terms(si, sj, rect, lam=None, line=None):
    """(terms (5), magnitudes (5), delta): sum ivar_i e_i delta, sum ivar_j e_j delta, 1/2 sum ivar_i
    delta^2, 1/2 sum ivar_j delta^2, Delta_prior; the magnitudes are the sums of the absolute
    summands (the scale of each term's rounding error)."""
    delta = patch_delta(si, sj, patch_of(si.mask, rect), line)
    vi, vj, ei, ej = ivar_of(si), ivar_of(sj), residual_of(si), residual_of(sj)
    parts = (vi * ei * delta, vj * ej * delta, 0.5 * vi * delta ** 2, 0.5 * vj * delta ** 2)
    t4, m4 = prior_term(si.params, sj.params, si.mask, rect, lam)
    terms = np.array([float(np.sum(v, dtype=np.longdouble)) for v in parts] + [t4])
    mags = np.array([float(np.sum(np.abs(v))) for v in parts] + [m4])
    return terms, mags, delta


def log_ratio(t):
    """Delta = (-(t0 + t2) - (t3 - t1)) + t4: the device's expression, in its order."""
    return (-(t[0] + t[2]) - (t[3] - t[1])) + t[4]


def full_log_target(st, lam=None):
    """log of the rung's tempered target up to a constant: -1/2 chi2 under the rung's variance plus
    the smoothness prior's log density."""
    v = -O.half_chi2(st.err, st.var)
    if lam is not None:
        e = PO.energy(st.params, st.mask)
        v -= 0.5 * sum(lam[k] * e[k] for k in range(3))
    return v


def trade(si, sj, patch, delta):
    """The accepted proposal: e_i += delta, e_j -= delta, the patch's parameters trade places."""
    si.err = si.err + delta
    sj.err = sj.err - delta
    for (y, x) in patch:
        a = si.params[y, x].copy()
        si.params[y, x] = sj.params[y, x]
        sj.params[y, x] = a


class PatchLadder(TO.Ladder):
    """TO.Ladder whose rounds trade patches: ``swap_patches`` is one round of the rule."""

    def __init__(self, case, betas, seed, inits=None, jump_amplitude=0.1, lam=None, line=None):
        TO.Ladder.__init__(self, case, betas, seed, inits=inits, jump_amplitude=jump_amplitude)
        self.lam = None if lam is None else np.asarray(lam, dtype=np.float64)
        self.line = line
        n = len(self.betas)
        self.patch_attempts = np.zeros(n - 1, dtype=np.int64)
        self.patch_accepts = np.zeros(n - 1, dtype=np.int64)
        self.patch_history = []

    def sweep(self, s):
        for st in self.states:
            if self.lam is None:
                O.mh_sweep(st, s)
            else:
                PO.mh_sweep(st, s, self.lam)

    def swap_patches(self, round_, p):
        """One round.  Returns dict(oy, ox, nty, ntx, my, mx, energy (n, before the round), terms
        (n-1, nty, ntx, 5), mags (the same shape), u, logu, delta_log (n-1, nty, ntx; NaN where not
        proposed), decided (1, 0, -1), footprints (the accepted (pair, footprint rect) list))."""
        st0 = self.states[0]
        D, H, W = st0.data.shape
        fh, fw = st0.fsf.shape
        n = len(self.betas)
        oy, ox = origin_shift(self.seed, round_, p)
        nty, ntx = tile_counts(H, W, p, oy, ox)
        my, mx = colour_counts(fh, fw, p)
        shape = (n - 1, nty, ntx)
        rec = dict(oy=oy, ox=ox, nty=nty, ntx=ntx, my=my, mx=mx, energy=self.energies(),
                   terms=np.full(shape + (5,), np.nan), mags=np.full(shape + (5,), np.nan),
                   u=np.full(shape, np.nan), logu=np.full(shape, np.nan), delta_log=np.full(shape, np.nan),
                   decided=-np.ones(shape, dtype=np.int32), footprints=[])
        for tiles in colour_schedule(nty, ntx, my, mx):
            for i in TO.proposed_pairs(n, round_):
                si, sj = self.states[i], self.states[i + 1]
                for (ty, tx) in tiles:
                    rect = tile_rect(ty, tx, p, oy, ox, H, W)
                    patch = patch_of(si.mask, rect)
                    if not patch:
                        continue
                    terms, mags, delta = five_terms(si, sj, rect, self.lam, self.line)
                    u = patch_uniform(self.seed, round_, i, ty * ntx + tx)
                    logu, dl = math.log(u), log_ratio(terms)
                    ok = 1 if logu < dl else 0
                    rec["terms"][i, ty, tx], rec["mags"][i, ty, tx] = terms, mags
                    rec["u"][i, ty, tx], rec["logu"][i, ty, tx], rec["delta_log"][i, ty, tx] = u, logu, dl
                    rec["decided"][i, ty, tx] = ok
                    self.patch_attempts[i] += 1
                    if ok:
                        self.patch_accepts[i] += 1
                        trade(si, sj, patch, delta)
                        rec["footprints"].append((i, footprint(rect, fh, fw, H, W)))
        self.patch_history.append(rec)
        return rec


def decision_margin(rec):
    """The smallest |log u - Delta| over the proposed tiles of a round (inf: none proposed)."""
    m = np.abs(rec["logu"] - rec["delta_log"])[rec["decided"] >= 0]
    return float(m.min()) if m.size else math.inf


# ---- the toy of the detailed-balance test ---------------------------------------------------------

def toy_patch_transition_matrix(values, coupling, betas, lam):
    """Exact transition matrix of ONE patch proposal between rungs 0 and 1 on a toy of two coupled
    sites, of which site 0 is the patch.  A rung's state is (a0, a1) with a_k in ``values``; its
    energy is E(a) = (a0 - 1)^2 + (a1 + 1)^2 + coupling a0 a1 (the overlap of two footprints), its
    prior log density -1/2 lam (a0 - a1)^2, its target exp(-beta E + log prior).  The proposal trades
    a0 between the rungs; it is accepted with probability min(1, exp(Delta)) where Delta is the
    LOCAL expression of the rule: the likelihood part from the change of E written with the
    difference d = a0_i - a0_j, the prior part from the four squared differences."""
    states = [(a, b) for a in values for b in values]
    idx = {s: k for k, s in enumerate(states)}
    k = len(states)
    T = np.zeros((k * k, k * k))
    for si in states:
        for sj in states:
            d = si[0] - sj[0]       # the patch's difference; E is quadratic in a0: exact local forms
            # E(sj[0], si[1]) - E(si) and E(si[0], sj[1]) - E(sj), in terms of d (the "e delta" and "delta^2" terms)
            dEi = -d * (2. * (si[0] - 1.) + coupling * si[1]) + d * d
            dEj = d * (2. * (sj[0] - 1.) + coupling * sj[1]) + d * d
            prior = -0.5 * lam * ((sj[0] - si[1]) ** 2 - (si[0] - si[1]) ** 2
                                  + (si[0] - sj[1]) ** 2 - (sj[0] - sj[1]) ** 2)
            delta = -betas[0] * dEi - betas[1] * dEj + prior
            acc = min(1., math.exp(delta))
            ni, nj = (sj[0], si[1]), (si[0], sj[1])
            T[idx[si] * k + idx[sj], idx[ni] * k + idx[nj]] += acc
            T[idx[si] * k + idx[sj], idx[si] * k + idx[sj]] += 1. - acc
    return T, states


def toy_patch_target(values, coupling, betas, lam):
    def logp(s, beta):
        return -beta * ((s[0] - 1.) ** 2 + (s[1] + 1.) ** 2 + coupling * s[0] * s[1]) - 0.5 * lam * (s[0] - s[1]) ** 2
    states = [(a, b) for a in values for b in values]
    pi = np.array([math.exp(logp(si, betas[0]) + logp(sj, betas[1])) for si in states for sj in states])
    return pi / pi.sum()


# ---- the cases of the GPU mechanics test ----------------------------------------------------------
# key: (parity case, p, betas, amplitude scales of the starts, smoothness sigmas or None, line, seed).
# tests/test_patch_exchange_cpu.py checks on this oracle that every proposed tile of every case
# decides with |log u - Delta| > 1e-6, so that the device's decisions compare one for one; a case
# that does not gets another seed.
DOUBLET = ((0., 3.8), (1., 1.4))
B3, B5 = (1., 0.5, 0.25), (1., 0.6, 0.35, 0.2, 0.1)
GPU_CASES = {
    "c1": ("c1", 4, B5, (1., 0.02, 0.3, 0.05, 0.6), None, None, 77),
    "odd_depth": ("odd_depth", 3, B5, (1., 0.02, 0.3, 0.05, 0.6), None, None, 77),
    "asym": ("asym", 2, B3, (1., 0.02, 0.3), None, None, 77),
    "rect_fsf": ("rect_fsf", 2, B3, (1., 0.02, 0.3), None, None, 77),
    "nolsf": ("nolsf", 1, B3, (1., 0.02, 0.3), (None, 2., 0.5), None, 77),
    "d30": ("d30", 16, (1., 0.98, 0.96), (0.02, 1., 0.021), None, None, 28),      # (seed: one tile in both rounds)
    "big_tile": ("asym", 16, B3, (0.02, 1., 0.3), None, None, 77),   # tiles beyond the staged form's LDS
    "deep601": ("deep601", 2, B3, (1., 0.02, 0.3), None, None, 77),
    "doublet": ("d30", 3, B3, (1., 0.02, 0.3), None, "doublet", 77),
    "tabulated": ("d30", 3, B3, (1., 0.02, 0.3), None, "table", 77),
}
ROUNDS = (0, 1)


def doublet_line(x, a, c, w):
    x = np.asarray(x, dtype=np.float64)
    return a * sum(r * np.exp(-((x - c) - off) ** 2 / (2. * w * w)) for off, r in zip(*DOUBLET))


def deep_case():
    """601 channels on 6 x 7 spaxels: deeper than one pass of a workgroup over z."""
    rng = np.random.default_rng(601)
    D, H, W = 601, 6, 7
    fsf = O.gaussian_fsf_image(1.2)
    lsf = O.muse_like_lsf(D)
    truth = np.dstack((1. + 9. * rng.random((H, W)), D * (0.25 + 0.5 * rng.random((H, W))),
                       0.8 + 2. * rng.random((H, W))))
    mask = np.ones((H, W))
    mask[2, 3] = 0
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    sigma = 0.05 * np.max(clean) + 1e-3
    data = clean + rng.normal(0., sigma, size=(D, H, W))
    var = (sigma * (0.5 + rng.random((D, H, W)))) ** 2
    min_b, max_b = O.model_min_boundaries(), O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(name="deep601", D=D, H=H, W=W, fsf=fsf, lsf=lsf, truth=truth, mask=mask, data=data, var=var,
                min_b=min_b, max_b=max_b, init=init)


def lam_of(sigmas):
    """lam_k = 1 / sigma_k^2 (0 for None) of a smoothness=(sigma_a, sigma_c, sigma_w)."""
    return None if sigmas is None else np.array([0. if s is None else 1. / (s * s) for s in sigmas])


_INPUTS, _ROUNDS = {}, {}


def case_inputs(key):
    """dict(case, p, betas, inits, sigmas, lam, line (the oracle's line function or None), kind, seed)
    of a GPU case: ``c1`` with ONE constant variance, ``odd_depth`` with three NaN voxels."""
    if key in _INPUTS:
        return _INPUTS[key]
    from tests.cases import make_case
    from tests import tabulated_oracle as TB
    name, p, betas, scales, sigmas, kind, seed = GPU_CASES[key]
    case = deep_case() if name == "deep601" else dict(make_case(name))
    if key == "c1":
        case["var"] = np.full(case["data"].shape, float(np.median(case["var"])))
    if key == "odd_depth":
        case["data"] = case["data"].copy()
        for z, y, x in ((0, 0, 0), (7, 5, 4), (20, 11, 9)):
            case["data"][z, y, x] = np.nan
        # (lib/run.py:153-162, d3d_set_data: a spaxel with a NaN voxel is masked; the voxel itself
        # stays in its neighbours' footprints with 1/var = 0)
        case["mask"] = case["mask"] * ~np.isnan(case["data"]).any(axis=0)
    line = None
    if kind == "doublet":
        line = doublet_line
    elif kind == "table":
        line = TB.line(*TB.profile_S())
    inits = TO.scaled_starts(case, scales)
    if sigmas is not None:      # (the rungs differ in c and w too: the prior's term is not zero)
        rng = np.random.default_rng(seed)
        for init in inits:
            init[..., 1] = np.clip(init[..., 1] + rng.normal(0., 1., init.shape[:2]), case["min_b"][1], case["max_b"][1])
            init[..., 2] = np.clip(init[..., 2] * (1. + 0.3 * rng.random(init.shape[:2])), case["min_b"][2],
                                   case["max_b"][2])
    _INPUTS[key] = dict(case=case, p=p, betas=betas, inits=inits, sigmas=sigmas,
                        lam=lam_of(sigmas), line=line, kind=kind, seed=seed)
    return _INPUTS[key]


def initial_errors(inp):
    """The residual of every rung's start, with the case's line."""
    case = inp["case"]
    out = []
    for init in inp["inits"]:
        if inp["line"] is None:
            out.append(O.compute_error_in_one_step(case["data"], init, case["mask"], case["fsf"], case["lsf"]))
            continue
        sim = np.zeros(case["data"].shape)
        for (y, x) in O.spaxel_iterator(case["mask"]):
            conv = O.spectral_convolve(inp["line"](np.arange(case["D"]), *init[y, x]), case["lsf"])
            sim[:, y, x] = conv
        out.append(case["data"] - O.spatial_convolve(sim, case["fsf"]))
    return out


def oracle_rounds(key):
    """The rounds ROUNDS of a GPU case on the oracle, from the starts: (ladder, [record of each
    round with ``before`` / ``after`` = every rung's (params, err) copies])."""
    if key in _ROUNDS:
        return _ROUNDS[key]
    inp = case_inputs(key)
    lad = PatchLadder(inp["case"], inp["betas"], inp["seed"], inits=inp["inits"], lam=inp["lam"], line=inp["line"])
    if inp["line"] is not None:
        for st, err in zip(lad.states, initial_errors(inp)):
            st.err = err
    recs = []
    for k in ROUNDS:
        before = [(st.params.copy(), st.err.copy()) for st in lad.states]
        rec = lad.swap_patches(k, inp["p"])
        rec["before"] = before
        rec["after"] = [(st.params.copy(), st.err.copy()) for st in lad.states]
        recs.append(rec)
    _ROUNDS[key] = (lad, recs)
    return _ROUNDS[key]


COARSE = dict(name="nolsf", betas=(1., 0.5, 0.25), p=2, scales=(1., 0.02, 1.), seed=77, sweeps=6)
_COARSE = []


def coarse_schedule():
    """`nolsf`, betas (1, 0.5, 0.25), p = 2, rung 1 started from amplitudes 50 times smaller: sweep
    s = 1 .. 6 of every rung, round s - 1 after each.  (ladder, the rounds' records), computed once."""
    if not _COARSE:
        from tests.cases import make_case
        case = make_case(COARSE["name"])
        lad = PatchLadder(case, COARSE["betas"], COARSE["seed"], inits=TO.scaled_starts(case, COARSE["scales"]))
        recs = []
        for s in range(1, COARSE["sweeps"] + 1):
            lad.sweep(s)
            recs.append(lad.swap_patches(s - 1, COARSE["p"]))
        _COARSE.append((lad, recs))
    return _COARSE[0]


SWEEP_CASES = ("c1", "asym", "nolsf")
_SWEEPS = {}


def sweep_schedule(key):
    """A case of GPU_CASES through sweeps 1, 2, the rounds ROUNDS, sweeps 3 .. 5 (with the case's
    prior): (ladder, the rounds' records), computed once."""
    if key not in _SWEEPS:
        inp = case_inputs(key)
        assert inp["line"] is None
        lad = PatchLadder(inp["case"], inp["betas"], inp["seed"], inits=inp["inits"], lam=inp["lam"])
        for s in (1, 2):
            lad.sweep(s)
        recs = [lad.swap_patches(k, inp["p"]) for k in ROUNDS]
        for s in (3, 4, 5):
            lad.sweep(s)
        _SWEEPS[key] = (lad, recs)
    return _SWEEPS[key]
