"""
CPU tests (no GPU) of the exchange of patches of spaxels between tempered rungs
(Run(tempering=dict(..., patch=p)), deconv3d_amd/tempering.py, tests/patch_exchange_oracle.py):
the keyword, its refusals and its checkpoint record; the tile arithmetic of a round; the local log
ratio against the difference of the full tempered log targets; the whole-field tile against the
whole-cube rule; detailed balance of the rule on a toy by exact enumeration; and, for every case
of tests/test_gpu_patch_exchange.py, that no proposed tile decides within 1e-6 of log u = Delta.
"""
import itertools
import math
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, tempering
from oracle import deconv3d_oracle as O
from tests import patch_exchange_oracle as PX
from tests import prior_oracle as PO
from tests import tempering_oracle as TO
from tests.cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_temper_set_patch", "d3d_temper_last_patches", "d3d_temper_get_patches")


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- keyword, refusals, checkpoint record -----------------------------------------------------------

def test_patch_keyword():
    assert "patch" in tempering.KEYS
    assert tempering.check_keywords(dict(betas=(1., 0.5), patch=2)) == dict(betas=(1., 0.5), swap_every=1, patch=2)
    assert tempering.check_keywords(dict(betas=(1., 0.5), patch=np.int64(10), swap_every=3))["patch"] == 10
    assert tempering.check_keywords(dict(rungs=3, beta_min=0.25, patch=1))["patch"] == 1
    # None is the whole-cube exchange: the dict of a run that never named the key
    assert tempering.check_keywords(dict(betas=(1., 0.5), patch=None)) == dict(betas=(1., 0.5), swap_every=1)


@pytest.mark.parametrize("patch", [0, -1, 1.5, True, "2", (2, 2)])
def test_run_refuses_a_bad_patch_before_any_device_work(patch):
    with pytest.raises(ValueError, match="tempering patch= MUST be an integer >= 1"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, tempering=dict(betas=(1., 0.5), patch=patch))


def test_the_refusals_of_tempering_stay_with_patch():
    with pytest.raises(ValueError, match=r"tempering= with chains=3: the rungs take the chains' place"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, chains=3, tempering=dict(betas=(1., 0.5), patch=2))

    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="tempering=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40,
                tempering=dict(betas=(1., 0.5), patch=2))
    with pytest.raises(ValueError, match="unknown key"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, tempering=dict(betas=(1., 0.5), patches=2))


def state_of(cfg):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=len(cfg["betas"]))
    state.update(tempering.state_record(cfg))
    return state


def test_checkpoint_record_and_resume():
    whole = tempering.check_keywords(dict(betas=(1., 0.5)))
    two = tempering.check_keywords(dict(betas=(1., 0.5), patch=2))
    three = tempering.check_keywords(dict(betas=(1., 0.5), patch=3))
    assert int(tempering.state_record(two)["tempering_patch"]) == 2
    assert int(tempering.state_record(whole)["tempering_patch"]) == 0
    assert int(tempering.state_record(dict(betas=(1., 0.5), swap_every=1))["tempering_patch"]) == 0   # a cfg without the key
    for cfg in (whole, two):
        tempering.check_resume(state_of(cfg), state_of(cfg), cfg)
    for saved, now, what in ((two, three, "patch=2; this run has patch=3"), (two, whole, "patch=2; this run has patch=None"),
                             (whole, two, "patch=None; this run has patch=2")):
        with pytest.raises(ValueError, match="resume_state was written with tempering " + what):
            tempering.check_resume(state_of(saved), state_of(saved), now)
    # a state of before the key: whole cubes
    old = state_of(whole)
    del old["tempering_patch"]
    tempering.check_resume(old, old, whole)
    with pytest.raises(ValueError, match="patch=None; this run has patch=2"):
        tempering.check_resume(old, old, two)
    with pytest.raises(ValueError, match="patch=2; this run has patch=3"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(two),
                tempering=dict(betas=(1., 0.5), patch=3))


def test_report_counts_patches_and_has_no_labels():
    rep = tempering.TemperingReport((1., 0.5, 0.25), 1, 4, [0, 0], [0, 0], [4, 4, 4], [1., 2., 3.], [0., 0., 0.],
                                    [0, 1, 2], last_round=4, patch=2, patch_attempts=[40, 30], patch_accepts=[10, 0])
    assert rep.patch == 2 and rep.labels is None
    np.testing.assert_array_equal(rep.patch_attempts, [40, 30])
    np.testing.assert_array_equal(rep.patch_rates, [0.25, 0.])
    whole = tempering.TemperingReport((1., 0.5), 1, 0, [0], [0], [0, 0], [0., 0.], [0., 0.], [0, 1])
    assert whole.patch is None and not whole.patch_attempts.any() and np.isnan(whole.patch_rates).all()
    np.testing.assert_array_equal(whole.labels, [0, 1])


def test_entries_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "deconv3d_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(d3d_temper \*t" % name, header), name
        assert name in _lib.SYMBOLS and name in _lib.TEMPER_PROTOTYPES
    assert "labels stay as created" in header


# ---- the tile arithmetic ------------------------------------------------------------------------------

@pytest.mark.parametrize("H, W, fh, fw", [(8, 9, 7, 7), (10, 12, 3, 7), (16, 16, 9, 9), (5, 13, 1, 5)])
@pytest.mark.parametrize("p", [1, 2, 3, 10, 16])
def test_tiles_partition_the_field_and_colours_keep_footprints_apart(H, W, fh, fw, p):
    rng = np.random.default_rng(H * 100 + W + p)
    mask = (rng.random((H, W)) > 0.15).astype(float)
    my, mx = PX.colour_counts(fh, fw, p)
    assert my == 1 + math.ceil((fh - 1) / p) and mx == 1 + math.ceil((fw - 1) / p)
    for oy, ox in itertools.product(range(p), range(p)):
        nty, ntx = PX.tile_counts(H, W, p, oy, ox)
        owner = -np.ones((H, W), dtype=int)
        for ty in range(nty):
            for tx in range(ntx):
                for (y, x) in PX.patch_of(mask, PX.tile_rect(ty, tx, p, oy, ox, H, W)):
                    assert owner[y, x] == -1 and PX.tile_of(y, x, p, oy, ox) == (ty, tx)
                    owner[y, x] = ty * ntx + tx
        assert np.all((owner >= 0) == (mask == 1))       # every unmasked spaxel in exactly one tile
        ty_max, tx_max = PX.tile_of(H - 1, W - 1, p, oy, ox)
        assert ty_max == nty - 1 and tx_max == ntx - 1
        colours = PX.colour_schedule(nty, ntx, my, mx)
        assert sorted(t for c in colours for t in c) == [(ty, tx) for ty in range(nty) for tx in range(ntx)]
        for tiles in colours:
            cover = np.zeros((H, W), dtype=int)           # footprints of one colour
            grown = np.zeros((H, W), dtype=int)           # the tiles grown by one spaxel (adjacency)
            for (ty, tx) in tiles:
                rect = PX.tile_rect(ty, tx, p, oy, ox, H, W)
                if rect[0] >= rect[1] or rect[2] >= rect[3]:
                    continue
                y0, y1, x0, x1 = PX.footprint(rect, fh, fw, H, W)
                cover[y0:y1, x0:x1] += 1
                grown[max(0, rect[0] - 1):rect[1] + 1, max(0, rect[2] - 1):rect[3] + 1] += 1
            assert cover.max(initial=0) <= 1
            if fh >= 3 and fw >= 3:
                assert grown.max(initial=0) <= 1


def test_p_at_least_the_field_and_a_shift_beyond_it_is_one_tile():
    H, W, p = 9, 11, 16
    for oy, ox in itertools.product(range(p), range(p)):
        nty, ntx = PX.tile_counts(H, W, p, oy, ox)
        live = [(ty, tx) for ty in range(nty) for tx in range(ntx)
                if PX.patch_of(np.ones((H, W)), PX.tile_rect(ty, tx, p, oy, ox, H, W))]
        assert (len(live) == 1) == ((oy == 0 or oy >= H) and (ox == 0 or ox >= W))


def test_origin_shift_and_uniforms_use_their_own_counter_words():
    seed = 77
    assert PX.origin_shift(seed, 3, 1) == (0, 0)
    shifts = {PX.origin_shift(seed, k, 10) for k in range(40)}
    assert len(shifts) > 20 and all(0 <= a < 10 and 0 <= b < 10 for a, b in shifts)
    us = [PX.patch_uniform(seed, 3, 0, t) for t in range(50)]
    assert len(set(us)) == 50 and TO.swap_uniform(seed, 3, 0) not in us      # (word 1 is the whole-cube swap)


# ---- the local log ratio is the change of the full tempered log targets ----------------------------------

def hybrid_check(key, rounds=1):
    """Every proposed tile of a case's first round: Delta of the five terms against the difference
    of the full log targets (1/2 chi2 of residuals rebuilt from the hybrid maps, the whole prior)."""
    inp = PX.case_inputs(key)
    case, lam = inp["case"], inp["lam"]
    lad = PX.PatchLadder(case, inp["betas"], inp["seed"], inits=inp["inits"], lam=lam)
    D, H, W = case["data"].shape
    worst = 0.
    oy, ox = PX.origin_shift(inp["seed"], 0, inp["p"])
    nty, ntx = PX.tile_counts(H, W, inp["p"], oy, ox)
    for i in TO.proposed_pairs(len(inp["betas"]), 0):
        si, sj = lad.states[i], lad.states[i + 1]
        base = PX.full_log_target(si, lam) + PX.full_log_target(sj, lam)
        for ty in range(nty):
            for tx in range(ntx):
                rect = PX.tile_rect(ty, tx, inp["p"], oy, ox, H, W)
                patch = PX.patch_of(case["mask"], rect)
                if not patch:
                    continue
                terms, _, delta = PX.five_terms(si, sj, rect, lam)
                hi, hj = si.params.copy(), sj.params.copy()
                for (y, x) in patch:
                    hi[y, x], hj[y, x] = sj.params[y, x], si.params[y, x]
                full = 0.
                for st, hyb in ((si, hi), (sj, hj)):
                    err = O.compute_error_in_one_step(case["data"], hyb, case["mask"], case["fsf"], case["lsf"])
                    full += -O.half_chi2(err, st.var)
                    if lam is not None:
                        e = PO.energy(hyb, case["mask"])
                        full -= 0.5 * sum(lam[k] * e[k] for k in range(3))
                want = full - base
                got = PX.log_ratio(terms)
                # the carried residual after the trade against the rebuilt one
                scale = np.nanmax(np.abs(case["data"]))
                rebuilt = O.compute_error_in_one_step(case["data"], hi, case["mask"], case["fsf"], case["lsf"])
                assert np.nanmax(np.abs((si.err + delta) - rebuilt)) <= 1e-13 * scale
                worst = max(worst, abs(got - want) / abs(want))
    return worst


@pytest.mark.parametrize("key", ["nolsf", "rect_fsf", "odd_depth"])
def test_local_log_ratio_is_the_full_difference(key):
    """Bar: 1e-9 relative (the full difference cancels two 1/2 chi2 of ~1e5 to 1e7: 1e-16 x 1e7 over
    Deltas of 1 and more leaves 1e-9)."""
    worst = hybrid_check(key)
    print(key, "worst |Delta_local - Delta_full| / |Delta_full| = %.3g" % worst)
    assert worst <= 1e-9


def test_one_tile_over_the_whole_field_is_the_whole_cube_rule():
    inp = PX.case_inputs("d30")
    case = inp["case"]
    lad = PX.PatchLadder(case, inp["betas"], inp["seed"], inits=inp["inits"])
    D, H, W = case["data"].shape
    E, b = lad.energies(), inp["betas"]
    for i in (0, 1):
        terms, _, _ = PX.five_terms(lad.states[i], lad.states[i + 1], (0, H, 0, W))
        want = (b[i] - b[i + 1]) * (E[i] - E[i + 1])
        assert abs(PX.log_ratio(terms) - want) <= 1e-9 * abs(want)
    _, recs = PX.oracle_rounds("d30")
    for rec in recs:                                       # the GPU case: one tile in both rounds
        assert (rec["nty"], rec["ntx"]) == (1, 1) and (rec["decided"] >= 0).sum() == 1
    assert sorted(int(rec["decided"].max()) for rec in recs) == [0, 1]        # a rejection and a whole swap


# ---- detailed balance, by exact enumeration -------------------------------------------------------------

@pytest.mark.parametrize("coupling, lam", [(0., 0.), (0.7, 0.), (0.7, 1.3), (-1.1, 0.4)])
def test_patch_rule_keeps_the_joint_tempered_distribution_invariant(coupling, lam):
    values, betas = (-1.5, -0.2, 0.4, 1.1, 2.3), (1., 0.3)
    T, _ = PX.toy_patch_transition_matrix(values, coupling, betas, lam)
    pi = PX.toy_patch_target(values, coupling, betas, lam)
    np.testing.assert_allclose(T.sum(axis=1), 1., rtol=0, atol=1e-14)
    flow = pi[:, None] * T
    np.testing.assert_allclose(flow, flow.T, rtol=1e-12, atol=1e-18)          # detailed balance
    np.testing.assert_allclose(pi @ T, pi, rtol=1e-12, atol=1e-18)
    assert (np.diag(T) < 1. - 1e-6).sum() > 100                               # (the proposal does move)
    # a wrong sign of the prior's term breaks it (the test can fail)
    if lam:
        Tw, _ = PX.toy_patch_transition_matrix(values, coupling, betas, -lam)
        assert np.max(np.abs(pi @ Tw - pi)) > 1e-4


# ---- the GPU cases decide far from log u = Delta ------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(PX.GPU_CASES))
def test_gpu_case_decisions_are_comparable(key):
    _, recs = PX.oracle_rounds(key)
    n_acc = n_rej = 0
    for k, rec in zip(PX.ROUNDS, recs):
        margin = PX.decision_margin(rec)
        print(key, "round", k, "tiles", rec["nty"], rec["ntx"], "colours", rec["my"], rec["mx"],
              "accepted", int((rec["decided"] == 1).sum()), "rejected", int((rec["decided"] == 0).sum()),
              "margin %.3g" % margin)
        assert margin > 1e-6
        n_acc += int((rec["decided"] == 1).sum())
        n_rej += int((rec["decided"] == 0).sum())
    assert n_acc >= 1 and (n_rej >= 1 or key == "deep601")         # (deep601: both outcomes are not its point)
    if key == "nolsf":                                      # the prior's term is in play
        t4 = np.concatenate([rec["terms"][..., 4][rec["decided"] >= 0] for rec in recs])
        assert np.all(t4 != 0.)
    if key == "c1":
        assert (recs[0]["my"], recs[0]["mx"]) == (3, 3)     # nine colours
    if key == "rect_fsf":
        assert recs[0]["my"] != recs[0]["mx"]


def test_coarse_ladder_swaps_where_whole_cubes_do_not():
    """The schedule of the GPU test: `nolsf`, betas (1, 0.5, 0.25), p = 2, six sweeps with a round
    after each.  In the rounds where the whole-cube rule, from the same energies, accepts no
    proposed pair, every proposed pair accepts at least one patch; every margin > 1e-6."""
    lad, recs = PX.coarse_schedule()
    shown = set()
    for k, rec in enumerate(recs):
        whole, _, _ = TO.decide(lad.betas, rec["energy"], lad.seed, k)
        assert PX.decision_margin(rec) > 1e-6
        for i in TO.proposed_pairs(3, k):
            print("round", k, "pair", i, "whole", whole[i], "patches accepted", int((rec["decided"][i] == 1).sum()),
                  "of", int((rec["decided"][i] >= 0).sum()))
            if whole[i] == 0:
                assert (rec["decided"][i] == 1).sum() >= 1
                shown.add(i)
    assert shown == {0, 1}


@pytest.mark.parametrize("key", PX.SWEEP_CASES)
def test_sweep_schedule_decisions_are_comparable(key):
    """The schedule of the GPU test of the state after more sweeps: both outcomes, every margin > 1e-6."""
    _, recs = PX.sweep_schedule(key)
    decided = np.concatenate([rec["decided"].ravel() for rec in recs])
    print(key, "accepted", int((decided == 1).sum()), "rejected", int((decided == 0).sum()),
          "margins", [PX.decision_margin(rec) for rec in recs])
    assert all(PX.decision_margin(rec) > 1e-6 for rec in recs)
    assert (decided == 1).any() and (decided == 0).any()
