"""
CPU tests (no GPU) of parallel tempering (Run(tempering=...), deconv3d_amd/tempering.py,
tests/tempering_oracle.py): the keyword is validated and the ladder built, chains != 1, a
host-evaluated model and a checkpoint written with another ladder are refused, all before any
device work; the report's arithmetic; where a call of the sweep loop ends; the C entry points are
declared, bound and cite the reference lines they generalise; and the oracle's swap rule keeps the
joint tempered distribution of a toy invariant, by exact enumeration.
"""
import math
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, tempering
from tests import tempering_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_temper_create", "d3d_temper_swap", "d3d_temper_get", "d3d_temper_last", "d3d_temper_destroy")


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- keywords and the ladder ------------------------------------------------------------------

@pytest.mark.parametrize("value", [
    (1., 0.5), "1,0.5", 2, dict(), dict(betas=(1., 0.5), rungs=2, beta_min=0.5), dict(betas=(1.,)),
    dict(betas=(0.9, 0.5)), dict(betas=(1., 1.)), dict(betas=(1., 0.5, 0.6)), dict(betas=(1., 0.)),
    dict(betas=(1., -0.5)), dict(betas=(1., float("nan"))), dict(betas=(1., float("inf"))), dict(betas="hot"),
    dict(betas=(1., "x")), dict(rungs=3), dict(beta_min=0.1), dict(rungs=1, beta_min=0.1),
    dict(rungs=2.5, beta_min=0.1), dict(rungs=True, beta_min=0.1), dict(rungs=3, beta_min=1.),
    dict(rungs=3, beta_min=0.), dict(rungs=3, beta_min=float("nan")), dict(rungs=65, beta_min=0.1),
    dict(betas=(1., 0.5), swap_every=0), dict(betas=(1., 0.5), swap_every=1.5),
    dict(betas=(1., 0.5), swap_every=True), dict(betas=(1., 0.5), every=2),
    dict(betas=tuple(0.99 ** r for r in range(65))),
])
def test_run_refuses_bad_keywords_before_any_device_work(value):
    with pytest.raises(ValueError, match="tempering"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, tempering=value)


def test_keywords_become_a_ladder():
    assert tempering.check_keywords(None) is None
    assert tempering.check_keywords(dict(betas=[1, 0.5, 0.2])) == dict(betas=(1., 0.5, 0.2), swap_every=1)
    assert tempering.check_keywords(dict(betas=np.array([1., 0.25]), swap_every=7)) == \
        dict(betas=(1., 0.25), swap_every=7)
    got = tempering.check_keywords(dict(rungs=4, beta_min=0.05, swap_every=np.int64(3)))
    assert got["swap_every"] == 3 and len(got["betas"]) == 4
    assert got["betas"][0] == 1. and got["betas"][-1] == 0.05
    assert got["betas"] == tuple(0.05 ** (r / 3.) for r in range(4))
    ratios = np.array(got["betas"][1:]) / np.array(got["betas"][:-1])
    np.testing.assert_allclose(ratios, ratios[0], rtol=1e-14)                # geometric
    assert tempering.geometric_ladder(2, 0.3) == (1., 0.3)
    assert len(tempering.check_keywords(dict(rungs=64, beta_min=0.01))["betas"]) == 64


# ---- refusals -----------------------------------------------------------------------------------

def test_run_refuses_chains_with_tempering():
    with pytest.raises(ValueError, match=r"tempering= with chains=3: the rungs take the chains' place"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, chains=3, tempering=dict(betas=(1., 0.5)))


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="tempering=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, tempering=dict(betas=(1., 0.5)))


def state_of(betas=None, swap_every=1, n_chains=None):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0,
                 n_chains=(1 if betas is None else len(betas)) if n_chains is None else n_chains)
    if betas is not None:
        state.update(tempering.state_record(dict(betas=tuple(betas), swap_every=swap_every)))
    return state


@pytest.mark.parametrize("saved, kw, what", [
    ((1., 0.5), dict(tempering=dict(betas=(1., 0.25))), r"betas=\(1, 0.5\); this run has betas=\(1, 0.25\)"),
    ((1., 0.5), dict(tempering=dict(betas=(1., 0.5), swap_every=2)), "swap_every=1; this run has swap_every=2"),
    ((1., 0.5), dict(chains=2), "this run has none"),
    ((1., 0.5), dict(tempering=dict(betas=(1., 0.5, 0.25))), r"holds 2 chain\(s\), this run has chains=3"),
    (None, dict(tempering=dict(betas=(1., 0.5))), r"holds 1 chain\(s\)"),
])
def test_run_refuses_a_state_written_with_another_ladder(saved, kw, what):
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(saved), **kw)


def test_resume_checks_the_ladder_and_the_cadence():
    cfg = tempering.check_keywords(dict(betas=(1., 0.3), swap_every=4))
    state = state_of((1., 0.3), swap_every=4)
    tempering.check_resume(state, state, cfg)
    tempering.check_resume(state_of(), state_of(), None)
    with pytest.raises(ValueError, match="written without tempering=; this run asks for betas="):
        tempering.check_resume(state_of(n_chains=2), state_of(n_chains=2), cfg)
    rec = tempering.state_record(cfg)
    np.testing.assert_array_equal(rec["tempering_betas"], [1., 0.3])
    assert int(rec["swap_every"]) == 4


# ---- the loop's arithmetic ----------------------------------------------------------------------

def test_a_call_ends_at_every_sweep_an_exchange_follows():
    """Sweeps 1 .. 40 in calls of at most 8, origin 13, swap_every 5: every sweep s with
    (s + 13) % 5 == 0 ends a call and no other call reports a round; the rounds are (s + 13) // 5."""
    for origin, every, per_call in ((13, 5, 8), (0, 1, 64), (0, 7, 3), (100, 4, 4)):
        it, rounds, ends = 1, [], []
        while it < 41:
            n, rnd = tempering.calls_until_swap(min(per_call, 41 - it), it, origin, every)
            assert 1 <= n <= per_call
            last = it + n - 1
            assert all((s + origin) % every != 0 for s in range(it, last))    # none skipped inside
            if rnd is not None:
                assert (last + origin) % every == 0 and rnd == (last + origin) // every
                rounds.append(rnd)
                ends.append(last)
            else:
                assert (last + origin) % every != 0
            it += n
        assert ends == [s for s in range(1, 41) if (s + origin) % every == 0]
        assert rounds == sorted(set(rounds))                                  # no uniform drawn twice


# ---- the report ---------------------------------------------------------------------------------

def test_report_arithmetic(tmp_path):
    rep = tempering.TemperingReport((1., 0.5, 0.1), 2, 9, attempts=[5, 0], accepts=[2, 0],
                                    energy_n=[9, 9, 1], energy_mean=[10., 20., 30.],
                                    energy_m2=[32., 0., 0.], labels=[1, 0, 2])
    np.testing.assert_array_equal(rep.betas, [1., 0.5, 0.1])
    assert rep.rounds == 9 and rep.swap_every == 2
    assert rep.swap_rates[0] == 0.4 and np.isnan(rep.swap_rates[1])           # nothing proposed: NaN
    np.testing.assert_array_equal(rep.energy_mean, [10., 20., 30.])
    assert rep.energy_std[0] == 2. and rep.energy_std[1] == 0. and np.isnan(rep.energy_std[2])
    np.testing.assert_array_equal(rep.labels, [1, 0, 2])
    rep.save(str(tmp_path / "t"))
    got = np.load(str(tmp_path / "t_tempering.npz"))
    for key in ("betas", "swap_attempts", "swap_accepts", "swap_rates", "energy_mean", "energy_std", "labels"):
        np.testing.assert_array_equal(got[key], getattr(rep, key))
    assert int(got["rounds"]) == 9
    empty = tempering.TemperingReport((1., 0.5), 1, 0, [0], [0], [0, 0], [0., 0.], [0., 0.], [0, 1])
    assert np.isnan(empty.energy_mean).all() and np.isnan(empty.energy_std).all()


# ---- the C ABI ----------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("replica exchange between tempered chains"):text.index("spatial tiling")]
    assert "lib/run.py:426-438" in section
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.TEMPER_PROTOTYPES
        assert "int %s(" % name in section
    for name in ("swap", "get", "last", "close"):
        assert callable(getattr(_lib.TemperGroup, name))
    make = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\bd3d_temper\.hip\b", make, flags=re.M)
    import __graft_entry__ as entry
    assert "d3d_temper.hip" in entry.SOURCES                                   # d3d_source_hash covers it


# ---- the oracle's rule --------------------------------------------------------------------------

def test_swap_uniform_is_philox_with_the_fourth_counter_word_1():
    from oracle import deconv3d_oracle as O
    u = TO.swap_uniform(12345, 7, 2)
    r = O.philox4x32_10((0xFFFFFFFF, 7, 2, 1), (12345, 0))
    assert u == O.u64_to_unit((r[1] << 32) | r[0]) and 0. < u < 1.
    assert u != O.philox_pair(12345, 0xFFFFFFFF, 7, 2)[0]                      # (word 0: a chain's stream)
    assert TO.proposed_pairs(4, 0) == [0, 2] and TO.proposed_pairs(4, 1) == [1]
    assert TO.proposed_pairs(5, 3) == [1, 3] and TO.proposed_pairs(2, 1) == []


@pytest.mark.parametrize("betas", [(1., 0.3), (1., 0.05)])
def test_detailed_balance_of_the_rule_on_a_toy_by_exact_enumeration(betas):
    """Two rungs, three states of energies (0, 1.3, 4): pi(s0, s1) ~ exp(-b0 E[s0] - b1 E[s1]).
    The rule's transition matrix satisfies pi_x T_xy == pi_y T_yx for every pair of configurations,
    hence pi T == pi; with the opposite sign of delta it does not."""
    E = (0., 1.3, 4.)
    pi = TO.toy_target(E, betas)
    T = TO.toy_transition_matrix(E, betas)
    np.testing.assert_allclose(T.sum(axis=1), 1., rtol=0, atol=1e-15)
    flow = pi[:, None] * T
    np.testing.assert_allclose(flow, flow.T, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(pi @ T, pi, rtol=1e-13)
    wrong = TO.toy_transition_matrix(E, betas[::-1])                           # delta with the sign flipped
    assert np.max(np.abs(pi @ wrong - pi)) > 1e-3
    # and decide() takes the decision the matrix describes: u below / above the acceptance probability
    for s0, s1 in ((0, 2), (2, 0), (1, 2)):
        delta = (betas[0] - betas[1]) * (E[s0] - E[s1])
        for rnd in range(0, 40, 2):
            decided, u, logu = TO.decide(betas, (E[s0], E[s1]), 99, rnd)
            assert decided[0] == (1 if math.log(u[0]) < delta else 0) and logu[0] == math.log(u[0])
            if delta >= 0.:
                assert decided[0] == 1
        assert TO.decide(betas, (E[s0], E[s1]), 99, 1)[0][0] == -1             # odd round: pair 0 rests


# ---- the helpers of the GPU tests ---------------------------------------------------------------

def test_reference_energy_sources_and_book():
    rng = np.random.default_rng(3)
    err, var = rng.normal(size=(5, 4, 3)), 0.5 + rng.random((5, 4, 3))
    data = rng.normal(size=(5, 4, 3))
    want = math.fsum((0.5 * err ** 2 / var).ravel())
    for beta in (1., 0.3):                    # E does not depend on the rung the state sits at
        assert abs(TO.reference_energy(err, var, beta) - want) <= 4e-16 * want
        assert abs(TO.reference_energy(err, var, beta, data) - want) <= 4e-16 * want
    assert abs(TO.reference_energy(err, 0.7, 0.3) - math.fsum((0.5 * err ** 2 / 0.7).ravel())) <= 1e-15 * want
    data[2, 1, 0] = np.nan                    # a NaN voxel is skipped, whatever its residual
    err[2, 1, 0] = 1e9
    keep = ~np.isnan(data)
    got = TO.reference_energy(err, var, 0.3, data)
    assert abs(got - math.fsum((0.5 * err ** 2 / var)[keep])) <= 4e-16 * got
    assert TO.sources([1, -1, 0]) == [1, 0, 2, 3] and TO.sources([-1, 1, -1]) == [0, 2, 1, 3]
    assert TO.sources([-1]) == [0, 1] and TO.sources([1, -1, 1, -1]) == [1, 0, 3, 2, 4]
    book = TO.Book(4)
    book.enter(0, [1, -1, 0])
    book.enter(1, [-1, 1, -1])
    book.enter(2 ** 32 + 2, [0, -1, 1])
    assert book.labels == [1, 2, 3, 0] and book.rounds == 3
    np.testing.assert_array_equal(book.attempts, [2, 1, 2])
    np.testing.assert_array_equal(book.accepts, [1, 1, 1])
    with pytest.raises(AssertionError):
        book.enter(3, [0, -1, 0])             # an odd round proposes pair 1 alone


def test_scaled_starts_make_both_outcomes_of_the_grid_cap_case_certain():
    """The recipe of the 128 x 184 x 184 device test at 16 x 15 x 14: two sweeps after a start from
    amplitudes 50 times smaller a rung lies lower than one started from the drawn map, whichever
    of the two is hotter.  delta > 0 is accepted whatever u; delta < -5 is refused unless
    u < exp(-5), and the difference grows with the number of spaxels (161 times as many there)."""
    case = TO.caps_case(16, 15, 14)
    assert case["fsf"].shape == (3, 3) and abs(case["fsf"].sum() - 1.) < 1e-15
    for betas, scales, rounds, want in (((1., .5), (1., .02), (0, 1, 2), [[1], [-1], [0]]),
                                        ((1., .5, .25), (1., .02, 1.), (0, 1), [[1, -1], [-1, 0]])):
        starts = TO.scaled_starts(case, scales)
        np.testing.assert_array_equal(starts[1][..., 1:], case["init"][..., 1:])
        np.testing.assert_array_equal(starts[1][..., 0], case["init"][..., 0] * .02)
        lad = TO.Ladder(case, betas, 77, inits=starts)
        for s in (1, 2):
            lad.sweep(s)
        for k, row in zip(rounds, want):
            decided, u, logu, E = lad.swap(k)
            assert list(decided) == row
            for i in TO.proposed_pairs(len(betas), k):
                delta = (betas[i] - betas[i + 1]) * (E[i] - E[i + 1])
                assert delta > 0. if decided[i] == 1 else delta < -5.
