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
