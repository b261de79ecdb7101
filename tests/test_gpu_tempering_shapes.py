"""
Replica exchange (csrc/d3d_temper.hip) at the shapes, rung counts, seeds and transports that
tests/test_gpu_tempering.py does not reach.  Engine level: one helper (check_round) holds every
round of every case here to the same bars.

Tolerances, each the project's own for the same quantity:
  * energies against the reference sum, and d3d_chi2_map's total against beta_r E_r:
    rtol 1e-12 (test_gpu_tempering.py::test_exchange_mechanics);
  * log u within 4 ulp of log(u); u, the exchanged parameters and residuals, labels and counters
    bit for bit (test_exchange_mechanics);
  * the carried residual against one rebuilt from the parameters: 1e-11 x the data peak, and the
    parameters against the tempering oracle's replay: rtol = atol = 1e-9
    (test_gpu_tempering.py::test_state_is_consistent_after_exchanges);
  * a rung's parameters read through its own stream right after d3d_temper_swap returns: bit for
    bit those read after the leader's stream was waited for (the event dependency);
  * batched against alone: bit for bit
    (test_gpu_run.py::test_every_end_of_sweep_hook_at_once_batched_and_alone_across_a_call_boundary).

d3d_chi2_map's total is 1/2 sum err^2 / var_r with var_r = var / beta_r (k_chi2_map halves it), so
it equals beta_r E_r: a second device sum in another order than k_temper_energy's.

Dp is always even, so the odd-element branches of k_temper_energy and of swap_span on the cube
cannot be reached and are not tested; the odd tail of swap_span on the parameter map is (d30).
"""
import functools

import numpy as np
import pytest

from deconv3d_amd import _lib, ensemble
from oracle import deconv3d_oracle as O
from tests import tempering_oracle as TO
from tests.cases import make_case
from tests.test_gpu_posterior import bounded_case
from tests.test_gpu_run import every_hook_case
from tests.test_gpu_tempering import BETAS, make_engines, snapshot, ulps

pytestmark = pytest.mark.gpu

E_RTOL = 1e-12
RESIDUAL_BAR = 1e-11
PARAM_TOL = 1e-9


def close_all(engines):
    for e in engines:
        e.close()


def check_round(tag, case, betas, seed, k, before, last, after, got, book, chi2=None, history=None):
    """One round against the references.  ``before`` / ``after``: every rung's (parameters,
    SLOT_ERR); ``last`` / ``got``: d3d_temper_last / _get after the round; ``book``: the counters
    so far (TO.Book, updated here); ``chi2``: d3d_chi2_map's totals before the round.  Returns
    (accepted, rejected) pairs of the round."""
    n = len(betas)
    b = np.array(betas)
    want_E = np.array([TO.reference_energy(err, case["var"], betas[r], case["data"])
                       for r, (_, err) in enumerate(before)])
    rel = np.abs(last["energy"] / want_E - 1.)
    print("%s round %d: max rel err of E %.3g (bar %.1g)%s; decided %s"
          % (tag, k, rel.max(), E_RTOL, "" if chi2 is None else
             ", of the chi2 total %.3g" % np.max(np.abs(np.array(chi2) / (b * want_E) - 1.)), last["decided"]))
    assert np.isfinite(last["energy"]).all()
    np.testing.assert_allclose(last["energy"], want_E, rtol=E_RTOL, atol=0)
    if chi2 is not None:
        np.testing.assert_allclose(chi2, b * want_E, rtol=E_RTOL, atol=0)
    n_acc = n_rej = 0
    book.enter(k, last["decided"])                 # (the -1 pattern follows the round's parity)
    for i in range(n - 1):
        if last["decided"][i] == -1:
            assert np.isnan(last["u"][i]) and np.isnan(last["logu"][i])
            continue
        assert last["u"][i] == TO.swap_uniform(seed, k, i)                          # bit for bit
        assert ulps(last["logu"][i], np.log(last["u"][i])) <= 4.
        delta = (b[i] - b[i + 1]) * (last["energy"][i] - last["energy"][i + 1])
        assert last["decided"][i] == (1 if last["logu"][i] < delta else 0)          # the device's own E, logu
        n_acc += int(last["decided"][i] == 1)
        n_rej += int(last["decided"][i] == 0)
    src = TO.sources(last["decided"])
    for r in range(n):
        np.testing.assert_array_equal(after[r][0], before[src[r]][0], err_msg="%s params %d" % (tag, r))
        np.testing.assert_array_equal(after[r][1], before[src[r]][1], err_msg="%s residual %d" % (tag, r))
    np.testing.assert_array_equal(got["labels"], book.labels)
    np.testing.assert_array_equal(got["attempts"], book.attempts)
    np.testing.assert_array_equal(got["accepts"], book.accepts)
    assert got["rounds"] == book.rounds
    np.testing.assert_array_equal(got["energy_n"], book.rounds)
    if history is not None:
        history.append(last["energy"])
        E = np.array(history)
        np.testing.assert_allclose(got["energy_mean"], E.mean(axis=0), rtol=1e-13)
    return n_acc, n_rej


def run_rounds(tag, engines, case, betas, seed, rounds, chi2=True):
    """The rounds ``rounds`` of a new group over ``engines``, each through check_round.  Returns
    (accepted, rejected, the `last` of every round, the final `get`)."""
    book, history, lasts = TO.Book(len(betas)), [], []
    n_acc = n_rej = 0
    with _lib.TemperGroup(engines, betas, seed=seed) as group:
        before = snapshot(engines)
        for k in rounds:
            totals = [e.chi2_map()[1] for e in engines] if chi2 else None
            group.swap(k)
            # before anything waits for the leader's stream: the other rungs' own streams must wait
            # for the exchange on the device (d3d_get_params synchronises the rung's stream alone)
            early = [e.get_params() for e in engines[1:]]
            last, after, got = group.last(), snapshot(engines), group.get()
            for r, params in enumerate(early, 1):
                np.testing.assert_array_equal(params, after[r][0], err_msg="%s: rung %d read before the exchange" % (tag, r))
            a, r = check_round(tag, case, betas, seed, k, before, last, after, got, book, totals, history)
            n_acc, n_rej = n_acc + a, n_rej + r
            lasts.append(last)
            before = after
    return n_acc, n_rej, lasts, got


scaled_starts = TO.scaled_starts


# ---- A1. the grid caps ---------------------------------------------------------------------------

# A rung started from amplitudes 50 times smaller sits, two sweeps later, at a lower energy than
# one started from the drawn map (the line centres and widths it accepted in sweep 1 were judged
# against a nearly empty model).  (1, .02): the hotter rung 1 lies lower, delta > 0, log u < 0 <
# delta whatever u: pair 0 is accepted in round 0, and with the states traded delta < 0 by the
# same amount in round 2: refused unless u < exp(delta).  (1, .02, 1): round 1 proposes pair 1
# with the hottest rung highest: refused likewise.  The differences grow with the cube.
CAPS = {2: ((1., .5), (1., .02), (0, 1, 2)), 3: ((1., .5, .25), (1., .02, 1.), (0, 1))}


@pytest.mark.parametrize("n", [2, 3])
def test_grid_caps_bind_in_the_energy_and_the_exchange(n):
    """128 x 184 x 184 = 4 333 568 elements: more than 1024 workgroups x 256 lanes x 4 double2 of
    k_temper_energy (2 097 152) and than 2048 x 256 x 4 of k_temper_exchange (4 194 304), so
    every lane takes more grid-stride steps than the grid was sized for."""
    D, H, W = 128, 184, 184
    assert D * H * W > 2048 * 256 * 4 * 2 and D % 2 == 0
    case = TO.caps_case(D, H, W)
    betas, scales, rounds = CAPS[n]
    engines = make_engines(case, betas, inits=scaled_starts(case, scales))
    try:
        _lib.mh_sweeps_batch(engines, 2, first_sweep=1)
        n_acc, n_rej, lasts, _ = run_rounds("caps n=%d" % n, engines, case, betas, 77, rounds)
    finally:
        close_all(engines)
    assert n_acc >= 1 and n_rej >= 1, (n_acc, n_rej)


# ---- A2. the odd tail of the parameter map ---------------------------------------------------------

def odd_tail_starts(case):
    """The caps case's scaled starts (pairs 0 and 2 are accepted in round 0), and a width of the
    LAST spaxel -- the odd 297th double -- of its own in every rung: whether that spaxel is masked
    or refuses its proposals, the traded element differs between the rungs of a pair."""
    starts = scaled_starts(case, (1., .02, 1., .02))
    for r, start in enumerate(starts):
        start[-1, -1, 2] += 0.01 * r
    return starts


@pytest.mark.parametrize("uniform", [False, True])
def test_odd_parameter_tail_is_exchanged(uniform):
    """d30: 9 x 11 spaxels, 297 doubles of parameters -- 148 double2 and one double."""
    case = dict(make_case("d30"))
    assert (case["H"] * case["W"] * 3) % 2 == 1
    if uniform:
        case["var"] = np.full(case["data"].shape, float(np.median(case["var"])))
    engines = make_engines(case, BETAS, inits=odd_tail_starts(case))
    try:
        _lib.mh_sweeps_batch(engines, 3, first_sweep=1)
        assert engines[0].variance_is_uniform() == uniform
        tails = [e.get_params()[-1, -1, 2] for e in engines]
        assert len(set(tails)) == 4, tails
        n_acc, n_rej, lasts, _ = run_rounds("d30 uniform=%s" % uniform, engines, case, BETAS, 77, range(4))
    finally:
        close_all(engines)
    assert n_acc >= 1 and n_rej >= 1, (n_acc, n_rej)
    assert list(lasts[0]["decided"]) == [1, -1, 1]


# ---- A3. both words of the seed, the low word of the round ----------------------------------------------

def test_seed_and_round_words():
    seed = (5 << 32) | 77
    rounds = (0, 1, 2 ** 32 + 2, 2 ** 32 + 3)
    case = make_case("nolsf")
    engines = make_engines(case, BETAS, seed=seed)
    try:
        _lib.mh_sweeps_batch(engines, 2, first_sweep=1)
        _, _, lasts, _ = run_rounds("seed words", engines, case, BETAS, seed, rounds)
    finally:
        close_all(engines)
    for k, last in zip(rounds, lasts):
        for i in TO.proposed_pairs(len(BETAS), k):
            # Philox keyed with both words, the counter with the round's low word alone
            r = O.philox4x32_10((0xFFFFFFFF, k % 2 ** 32, i, 1), (77, 5))
            assert last["u"][i] == O.u64_to_unit((r[1] << 32) | r[0])
            assert last["u"][i] != TO.swap_uniform(77, k, i)                   # (the upper word keys)
            assert last["u"][i] == TO.swap_uniform(seed, k % 2 ** 32, i)       # the documented wrap
    assert TO.proposed_pairs(4, 2 ** 32 + 2) == [0, 2] and TO.proposed_pairs(4, 2 ** 32 + 3) == [1]


# ---- A4. rung counts ---------------------------------------------------------------------------------

def ladder(n):
    return tuple(0.05 ** (r / float(n - 1)) for r in range(n))


@pytest.mark.parametrize("n", [2, 5, 64])
def test_rung_counts(n):
    """2: an odd round proposes nothing (no exchange launch).  5: odd.  64 = TEMPER_MAX: 2.5 KiB of
    kernel arguments, the whole E[] array of k_temper_decide."""
    case = make_case("nolsf")
    betas = ladder(n)
    assert betas[0] == 1. and abs(betas[-1] - 0.05) < 1e-15
    engines = make_engines(case, betas)
    try:
        _lib.mh_sweeps_batch(engines, 2, first_sweep=1)
        n_acc, n_rej, lasts, got = run_rounds("n=%d" % n, engines, case, betas, 77, range(4))
    finally:
        close_all(engines)
    print("n = %d: %d accepted, %d refused" % (n, n_acc, n_rej))
    if n == 2:      # (check_round has shown that nothing changed and that the moments advanced)
        assert [list(last["decided"]) for last in lasts][1::2] == [[-1], [-1]]
        np.testing.assert_array_equal(got["energy_n"], [4, 4])
        np.testing.assert_array_equal(got["attempts"], [2])
    if n == 64:
        assert sorted(got["labels"]) == list(range(64))
        assert n_acc >= 1 and n_rej >= 1, (n_acc, n_rej)
        np.testing.assert_array_equal(got["attempts"], [2] * 63)


# ---- B. the state after exchanges, per transport and depth class -------------------------------------------

def nan_case():
    """`c1` with the three NaN voxels of test_gpu_posterior's `nan_masked`."""
    case = dict(make_case("c1"))
    case["data"] = case["data"].copy()
    case["data"][3, 2, 5] = case["data"][17, 9, 9] = case["data"][31, 15, 0] = np.nan
    return case


def as_the_device_sees(case):
    """NaN voxels: data 0 and 1/var 0, their spaxels masked (d3d_set_data)."""
    nan = np.isnan(case["data"])
    if not nan.any():
        return case
    out = dict(case)
    out["data"] = np.where(nan, 0., case["data"])
    out["var"] = np.where(nan, np.inf, case["var"])
    out["mask"] = np.where(nan.any(axis=0), 0, case["mask"])
    return out


@functools.lru_cache(maxsize=None)
def state_case(name):
    if name.startswith("D"):     # test_gpu_posterior's `deep` recipe: 6 x 7 spaxels, the MUSE-like LSF
        D = int(name[1:])
        return bounded_case(D, 6, 7, O.gaussian_fsf_image(1.0), O.muse_like_lsf(D), 9)
    if name == "nan":
        return nan_case()
    return make_case(name)


STATE_ROUNDS = 4


def state_starts(name):
    """The three small cubes see both outcomes from the case's own start (the oracle alone says
    so).  On the 6 x 7 cubes the Gibbs draw forgets a scaled amplitude within a sweep and the rungs
    refuse all six proposals, so rungs 1 and 3 start from the truth (synthetic_case's first draw)
    and rungs 0 and 2 from the case's start: three sweeps later the hotter rung of pairs 0 and 2
    lies far lower (accepted in round 0), and the two rungs that then hold the poor states, 2
    and 3, are refused in round 2."""
    if not name.startswith("D"):
        return None
    case = state_case(name)
    truth = O.synthetic_truth(case["D"], case["H"], case["W"], np.random.default_rng(9))
    return [case["init"], truth, case["init"], truth]


@functools.lru_cache(maxsize=None)
def oracle_state(name):
    """3 sweeps, 4 rounds, 3 sweeps on the tempering oracle (once per case, left unchanged)."""
    lad = TO.Ladder(as_the_device_sees(state_case(name)), BETAS, 77, inits=state_starts(name))
    for s in (1, 2, 3):
        lad.sweep(s)
    for k in range(STATE_ROUNDS):
        lad.swap(k)
    for s in (4, 5, 6):
        lad.sweep(s)
    return lad


@pytest.mark.parametrize("name", ["c1", "odd_depth", "nan", "D301", "D601", "D1101"])
def test_state_after_exchanges_by_transport_and_depth(name):
    """Small cubes: the sweeps through d3d_mh_sweeps_batch.  Beyond 256 channels the batch refuses
    and every rung is swept by its own thread on its own stream (ensemble.sweep_chains), z-blocked
    beyond 512 channels, the deep form beyond 1024: the exchange then follows, and is followed by,
    work on other streams than the leader's."""
    case = state_case(name)
    seen = as_the_device_sees(case)
    D = case["D"]
    engines = make_engines(case, BETAS, inits=state_starts(name))
    try:
        if D > 256:
            with pytest.raises(NotImplementedError, match="256 channels"):
                _lib.mh_sweeps_batch(engines, 3, first_sweep=1)

            def sweep(n, first):
                return ensemble.sweep_chains(engines, n, first)
        else:
            def sweep(n, first):
                return _lib.mh_sweeps_batch(engines, n, first_sweep=first)
        if D > 512:     # the z-blocked sweep kernels run: option on, the LSF fits, one pending layer
            for e in engines:
                assert e.get_option("mh_zblocks") == 1 and e.get_option("lsf_fits") == 1 and e.mh_layers() == 1
        sweep(3, 1)
        n_acc, n_rej, lasts, _ = run_rounds(name, engines, case, BETAS, 77, range(STATE_ROUNDS))
        sweep(3, 4)
        end = snapshot(engines)
    finally:
        close_all(engines)
    lad = oracle_state(name)
    live = seen["mask"] == 1
    if name == "nan":
        assert int(np.sum(case["mask"] == 1)) - int(np.sum(live)) == 3
    for k, last in enumerate(lasts):
        np.testing.assert_array_equal(last["decided"], lad.history[k][2], err_msg="round %d" % k)
    peak = np.max(np.abs(seen["data"]))
    for r, (params, err) in enumerate(end):
        rebuilt = O.compute_error_in_one_step(seen["data"], params, seen["mask"], case["fsf"], case["lsf"])
        worst = np.max(np.abs(err - rebuilt))
        print("%s rung %d: carried - rebuilt residual %.3g of the data peak (bar %.1g); parameters: max |d| %.3g"
              % (name, r, worst / peak, RESIDUAL_BAR, np.max(np.abs(params[live] - lad.states[r].params[live]))))
        assert worst <= RESIDUAL_BAR * peak, r
        np.testing.assert_allclose(params[live], lad.states[r].params[live], rtol=PARAM_TOL, atol=PARAM_TOL,
                                   err_msg="rung %d" % r)
    assert n_acc >= 1 and n_rej >= 1, (name, n_acc, n_rej)


# ---- A6. two pending layers ----------------------------------------------------------------------------

PENDING_BETAS = tuple(0.5 ** (r / 15.) for r in range(16))
# (starts scaled as in the caps case: of round 0's pairs, (0, 1), (4, 5), ... have the hotter rung
# lower and are accepted, (2, 3), (6, 7), ... the reverse and are refused; the oracle alone gives
# |delta| of 680 to 1130 for either after 2 and 3 sweeps)
PENDING_SCALES = (1., .02, .02, 1.) * 4


@pytest.mark.parametrize("n_batched", [2, 3])
def test_exchange_flushes_two_pending_layers_in_every_rung(n_batched):
    """16 rungs of `tile_a` fill the chip in one launch per colour class: two pending layers, both
    still pending after an even number of colour launches (2 sweeps of 35 classes), one after an
    odd number (3 sweeps).  d3d_download_slot(SLOT_ERR) itself flushes, so nothing is downloaded
    from the ladder under test before its round: the reference comes from a second ladder of the
    same seeds, its residual rebuilt from its parameters (d3d_residual, which drops the pending
    layers instead of applying them)."""
    case = make_case("tile_a")
    betas, n = PENDING_BETAS, len(PENDING_BETAS)
    peak = np.max(np.abs(case["data"]))
    starts = scaled_starts(case, PENDING_SCALES)
    engines, twins = make_engines(case, betas, inits=starts), []
    try:
        twins = make_engines(case, betas, inits=starts)
        _lib.mh_sweeps_batch(twins, n_batched, first_sweep=1)
        before = [(e.get_params(), e.residual()) for e in twins]
        _lib.mh_sweeps_batch(engines, n_batched, first_sweep=1)
        assert all(e.get_option("batch_layers") == 2 for e in engines)
        with _lib.TemperGroup(engines, betas, seed=77) as group:
            group.swap(0)
            last, got = group.last(), group.get()
            after = snapshot(engines)
            want_E = np.array([TO.reference_energy(err, case["var"], betas[r]) for r, (_, err) in enumerate(before)])
            print("pending %d: max rel err of E %.3g (bar %.1g); decided %s"
                  % (n_batched, np.max(np.abs(last["energy"] / want_E - 1.)), E_RTOL, last["decided"]))
            np.testing.assert_allclose(last["energy"], want_E, rtol=E_RTOL, atol=0)
            book = TO.Book(n)
            book.enter(0, last["decided"])
            src = TO.sources(last["decided"])
            b = np.array(betas)
            for i in TO.proposed_pairs(n, 0):
                assert last["u"][i] == TO.swap_uniform(77, 0, i)
                delta = (b[i] - b[i + 1]) * (last["energy"][i] - last["energy"][i + 1])
                assert last["decided"][i] == (1 if last["logu"][i] < delta else 0)
            for r in range(n):
                np.testing.assert_array_equal(after[r][0], before[src[r]][0], err_msg="params %d" % r)
                worst = np.max(np.abs(after[r][1] - before[src[r]][1]))
                assert worst <= RESIDUAL_BAR * peak, (r, worst / peak)
            np.testing.assert_array_equal(got["labels"], book.labels)
            np.testing.assert_array_equal(got["accepts"], book.accepts)
            # one more sweep: the carried residual is still the parameters'
            _lib.mh_sweeps_batch(engines, 1, first_sweep=n_batched + 1)
            for r, (params, err) in enumerate(snapshot(engines)):
                rebuilt = O.compute_error_in_one_step(case["data"], params, case["mask"], case["fsf"], case["lsf"])
                assert np.max(np.abs(err - rebuilt)) <= RESIDUAL_BAR * peak, r
                assert not np.array_equal(params, after[r][0])
        assert book.accepts.sum() >= 1 and (book.attempts - book.accepts).sum() >= 1, last["decided"]
    finally:
        close_all(engines + twins)


# ---- B. every end-of-sweep hook at once, batched and alone ------------------------------------------------

HOOK_BETAS = (1., 0.9, 0.8)


def hooks_schedule(case, D, batched):
    """12 sweeps, an exchange after every second one (round s // 2 after sweep s): refresh every
    5th sweep, jump-scale steps (window 3, up to sweep 9), the smoothness prior on c in every
    rung, the posterior moments (sweeps 6, 8, 10, 12) on rung 0 alone, snapshots every 2nd sweep."""
    H, W, seed = case["H"], case["W"], 500
    engines = []
    try:
        for r, beta in enumerate(HOOK_BETAS):
            eng = _lib.Engine((D, H, W), case["fsf"].shape)
            engines.append(eng)
            eng.set_taps(case["fsf"], case["lsf"])
            eng.set_data(case["data"], case["var"] / beta, mask=case["mask"])
            eng.set_params(case["init"])
            eng.mh_config(case["min_b"], case["max_b"], 0.1, 40.0, seed=seed + r, refresh_every=5)
            eng.adapt_begin(window=3, last_sweep=9)
            eng.prior_begin([0., 1. / 2.0 ** 2, 0.])
            if r == 0:
                eng.post_begin()
                eng.post_schedule(6, 2)
            eng.residual(fetch=False)
        chains = [np.full((7, H, W, 3), np.nan) for _ in engines]
        dlogs = [np.full((7, H, W), np.nan) for _ in engines]
        accepted, lasts = [], []
        with _lib.TemperGroup(engines, HOOK_BETAS, seed=seed) as group:
            for first in range(1, 12, 2):
                if batched:
                    accepted.append(_lib.mh_sweeps_batch(engines, 2, first, 2, chains, dlogs))
                else:
                    accepted.append([e.mh_sweeps(2, first, 2, chains[r], dlogs[r]) for r, e in enumerate(engines)])
                group.swap((first + 1) // 2)
                last = group.last()
                lasts.append(last)
            got = group.get()
        out = []
        for r, eng in enumerate(engines):
            out += [chains[r][1:], dlogs[r][1:], eng.get_params(), eng.get_dlog()]
            out += [np.asarray(a) for a in eng.adapt_get()]
            assert np.isnan(chains[r][0]).all() and not np.isnan(chains[r][1:][:, case["mask"] == 1]).any()
        for which in (0, 1, 2):
            out += list(engines[0].post_get(which))
        out += [np.asarray(engines[0].post_count()), np.asarray(accepted)]
        out += [got[key] for key in ("labels", "attempts", "accepts", "energy_n", "energy_mean", "energy_m2")]
        for last in lasts:
            out += [last[key] for key in ("energy", "u", "logu", "decided")]
        scales = [eng.adapt_get() for eng in engines]
        return out, scales, int(engines[0].post_count()), got, lasts
    finally:
        close_all(engines)


@pytest.mark.parametrize("D", [16, 21])
def test_every_hook_at_once_with_exchanges_batched_and_alone(D):
    case = every_hook_case(D, False)
    alone, scales, count, got, lasts = hooks_schedule(case, D, False)
    batched = hooks_schedule(case, D, True)[0]
    assert len(alone) == len(batched) == 3 * 8 + 6 + 2 + 6 + 4 * 6
    for i, (a, b) in enumerate(zip(batched, alone)):
        assert np.array_equal(a, b, equal_nan=True), "array %d" % i
    # not degenerate: both outcomes, the scales moved three times, four samples, and the scales
    # stayed with the rung (the rungs that traded states hold different ones)
    decided = np.concatenate([last["decided"] for last in lasts])
    print("hooks D = %d: decided %s, labels %s" % (D, decided, got["labels"]))
    assert np.sum(decided == 1) >= 1 and np.sum(decided == 0) >= 1
    assert got["rounds"] == 6 and count == 4
    live = case["mask"] == 1
    for r in range(3):
        assert int(scales[r][2]) == 3 and int(scales[r][3]) == 3
        assert len(np.unique(scales[r][0][live])) > 1
    assert not np.array_equal(scales[0][0], scales[1][0]) and not np.array_equal(scales[1][0], scales[2][0])
