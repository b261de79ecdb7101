"""
Numpy restatement of the replica exchange between tempered chains (include/deconv3d_hip.h:
d3d_temper_swap): R oracle states of one cube, rung r with the variance divided by betas[r],
advanced by the oracle's sweep; the energy of a state under the untempered variance; the swap
rule with its Philox uniform.  Test infrastructure only.
"""
import math

import numpy as np

from oracle import deconv3d_oracle as O


def swap_uniform(seed, round_, i):
    """The ``.x`` uniform of Philox4x32-10 at counter {0xFFFFFFFF, round, i, 1}: O.philox_pair
    fixes the counter's fourth word to 0 (the chains' streams), the exchange uses 1."""
    r = O.philox4x32_10((0xFFFFFFFF, int(round_) & 0xFFFFFFFF, i, 1),
                        (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return O.u64_to_unit((r[1] << 32) | r[0])


def energy(st, beta):
    """E = (1/2 sum err^2 / (var / beta)) / beta of a rung's state: minus log L under the
    untempered variance, whatever rung the state sits at."""
    return O.half_chi2(st.err, st.var) / beta


def reference_energy(err, var, beta, data=None):
    """E = (1/2 sum err^2 / (var / beta)) / beta of a downloaded residual, summed in extended
    precision (np.longdouble), in another order than the device's; ``var`` is the UNTEMPERED
    variance (a cube or one number).  Voxels where ``data`` is NaN are skipped: the device gives
    them 1/var = 0 (d3d_set_data)."""
    terms = np.asarray(err, dtype=np.float64) ** 2 / (np.asarray(var, dtype=np.float64) / beta)
    if data is not None:
        terms = terms[~np.isnan(data)]
    return float(0.5 * np.sum(terms, dtype=np.longdouble) / np.longdouble(beta))


def sources(decided):
    """src (n): after a round rung r holds the state that rung src[r] held before it."""
    n = len(decided) + 1
    src = list(range(n))
    for i in range(n - 1):
        if decided[i] == 1:
            src[i], src[i + 1] = i + 1, i
    return src


class Book(object):
    """What d3d_temper_get must report after the rounds it was shown: labels, attempts, accepts."""

    def __init__(self, n):
        self.n = n
        self.labels = list(range(n))
        self.attempts = np.zeros(n - 1, dtype=np.int64)
        self.accepts = np.zeros(n - 1, dtype=np.int64)
        self.rounds = 0

    def enter(self, round_, decided):
        """One round's decisions; AssertionError where a pair's -1 does not follow the parity."""
        proposed = proposed_pairs(self.n, round_)
        for i in range(self.n - 1):
            assert (decided[i] == -1) == (i not in proposed), (round_, i, decided[i])
            if decided[i] == -1:
                continue
            self.attempts[i] += 1
            if decided[i] == 1:
                self.accepts[i] += 1
                self.labels[i], self.labels[i + 1] = self.labels[i + 1], self.labels[i]
        self.rounds += 1


def caps_case(D, H, W, seed=5):
    """Noise plus three blobs of one line, a 3 x 3 Gaussian FSF, a short LSF, per-voxel variance.
    The recipe of the grid-cap test (128 x 184 x 184 on the device; tests/test_tempering_cpu.py
    runs it at 16 x 15 x 14 on the oracle)."""
    rng = np.random.default_rng(seed)
    g = np.exp(-0.5 * (np.arange(-1, 2) / 0.8) ** 2)
    fsf = np.outer(g, g) / np.sum(np.outer(g, g))
    lsf = O.gaussian_lsf_vector(D, 0.7)
    z = np.arange(D)[:, None, None]
    y, x = np.indices((H, W))
    data = rng.normal(0., 1., size=(D, H, W))
    for _ in range(3):
        cy, cx, cz = rng.random(3) * (H, W, D)
        data += 8. * np.exp(-0.5 * (((y - cy) / (H / 5.)) ** 2 + ((x - cx) / (W / 5.)) ** 2)) \
            * np.exp(-0.5 * ((z - cz) / 2.) ** 2)
    var = (0.5 + rng.random((D, H, W))) ** 2
    min_b, max_b = O.model_min_boundaries(), O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=np.ones((H, W)), min_b=min_b,
                max_b=max_b, init=init)


def scaled_starts(case, scales):
    """One start per rung: the case's, its amplitudes times ``scales[r]``."""
    return [case["init"] * np.array([s, 1., 1.]) for s in scales]


def proposed_pairs(n, round_):
    p = int(round_) & 1
    return [i for i in range(n - 1) if i % 2 == p]


def decide(betas, energies, seed, round_):
    """decided (n-1: 1, 0, -1 = not proposed), u and log u of one round."""
    n = len(betas)
    decided = -np.ones(n - 1, dtype=np.int32)
    u = np.full(n - 1, np.nan)
    logu = np.full(n - 1, np.nan)
    for i in proposed_pairs(n, round_):
        u[i] = swap_uniform(seed, round_, i)
        logu[i] = math.log(u[i])
        delta = (betas[i] - betas[i + 1]) * (energies[i] - energies[i + 1])
        decided[i] = 1 if logu[i] < delta else 0
    return decided, u, logu


class Ladder(object):
    """R ``O.MHState`` s of one case: rung r has ``var / betas[r]`` and seed ``seed + r``."""

    def __init__(self, case, betas, seed, inits=None, jump_amplitude=0.1):
        self.betas = [float(b) for b in betas]
        self.seed = seed
        self.states = [
            O.MHState(case["data"], case["var"] / b, case["mask"], case["fsf"], case["lsf"],
                      case["init"] if inits is None else inits[r], case["min_b"], case["max_b"],
                      jump_amplitude=jump_amplitude,
                      gibbs_apriori_variance=float(case["max_b"][0] ** 2), seed=seed + r)
            for r, b in enumerate(self.betas)]
        n = len(self.betas)
        self.labels = list(range(n))
        self.attempts = np.zeros(n - 1, dtype=np.int64)
        self.accepts = np.zeros(n - 1, dtype=np.int64)
        self.history = []      # (round, energies, decided) of every round

    def sweep(self, s):
        for st in self.states:
            O.mh_sweep(st, s)

    def energies(self):
        return np.array([energy(st, b) for st, b in zip(self.states, self.betas)])

    def swap(self, round_):
        """One round: accepted pairs trade residual and parameters, everything else stays."""
        E = self.energies()
        decided, u, logu = decide(self.betas, E, self.seed, round_)
        for i in proposed_pairs(len(self.betas), round_):
            self.attempts[i] += 1
            if decided[i] == 1:
                self.accepts[i] += 1
                a, b = self.states[i], self.states[i + 1]
                a.err, b.err = b.err, a.err
                a.params, b.params = b.params, a.params
                self.labels[i], self.labels[i + 1] = self.labels[i + 1], self.labels[i]
        self.history.append((round_, E, decided))
        return decided, u, logu, E


def toy_transition_matrix(energies, betas):
    """Exact transition matrix of ONE proposed pair (rungs 0, 1) on a toy whose states have the
    given energies: configuration (s0, s1) = the state at rung 0, the state at rung 1; the swap
    (s0, s1) -> (s1, s0) is accepted with probability P(log u < delta) = min(1, exp(delta))."""
    k = len(energies)
    T = np.zeros((k * k, k * k))
    for s0 in range(k):
        for s1 in range(k):
            delta = (betas[0] - betas[1]) * (energies[s0] - energies[s1])
            acc = min(1., math.exp(delta))
            T[s0 * k + s1, s1 * k + s0] += acc
            T[s0 * k + s1, s0 * k + s1] += 1. - acc
    return T


def toy_target(energies, betas):
    """pi(s0, s1) proportional to exp(-betas[0] E[s0] - betas[1] E[s1])."""
    k = len(energies)
    pi = np.array([math.exp(-betas[0] * energies[s0] - betas[1] * energies[s1])
                   for s0 in range(k) for s1 in range(k)])
    return pi / pi.sum()
