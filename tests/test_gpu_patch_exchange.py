"""
Exchange of patches of spaxels between tempered rungs on the device (csrc/d3d_temper.hip:
k_temper_patch, d3d_temper_set_patch; Run(tempering=dict(..., patch=p))) against its numpy
restatement (tests/patch_exchange_oracle.py): the per-tile record of a round, the traded
parameters and residuals, the state after more sweeps, the whole-cube round left as it was, the
Run plumbing, a coarse ladder that swaps where whole cubes do not, and the cold rung's energy.
"""
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, prior
from oracle import deconv3d_oracle as O
from tests import patch_exchange_oracle as PX
from tests import tabulated_oracle as TB
from tests import tempering_oracle as TO
from tests.cases import make_case
from tests.test_gpu_tempering import make_engines, run_inputs, run_kw, snapshot, tempered_case, ulps

pytestmark = pytest.mark.gpu

TERM_BAR = 1e-10          # of the sum of the absolute summands of each term (the project's chi2 bar)
RESIDUAL_BAR = 1e-11      # of the data peak (tests/test_gpu_tempering.py)


def engines_of(inp, options=None, refresh_every=0):
    """One engine per rung of a case of PX.GPU_CASES: variance / beta_r, seed + r, the case's line,
    prior and starts, a fresh residual."""
    case = inp["case"]
    engines = make_engines(case, inp["betas"], options=options, seed=inp["seed"], inits=inp["inits"],
                           refresh_every=refresh_every)
    for r, eng in enumerate(engines):
        if inp["kind"] == "doublet":
            eng.set_line_shape(*PX.DOUBLET)
        elif inp["kind"] == "table":
            model = d3d.TabulatedLineModel(*TB.profile_S())
            eng.set_line_shape(model.offsets, model.ratios)
            eng.set_line_table(model.table, model.support, model.table_integral)
        if inp["lam"] is not None:
            eng.prior_begin(inp["lam"])
        if inp["kind"] is not None:
            eng.set_params(inp["inits"][r])
            eng.residual(fetch=False)
    return engines


def round_of(group, engines, k):
    before = snapshot(engines)
    group.swap(k)
    return dict(before=before, patches=group.last_patches(), last=group.last(), after=snapshot(engines),
                get=group.get(), counts=group.get_patches())


@functools.lru_cache(maxsize=None)
def device_rounds(key):
    inp = PX.case_inputs(key)
    engines = engines_of(inp)
    try:
        with _lib.TemperGroup(engines, inp["betas"], seed=inp["seed"], patch=inp["p"]) as group:
            assert group.patch == inp["p"] and not group.get_patches()["attempts"].any()
            return [round_of(group, engines, k) for k in PX.ROUNDS]
    finally:
        for e in engines:
            e.close()


def rebuilt_residual(inp, params):
    return PX.initial_errors(dict(inp, inits=[params]))[0]


def check_record(got, rec, seed, k, n):
    """The device's per-tile record of round k against the oracle's: geometry, the five terms, u,
    log u, the decisions from the device's own numbers and equal to the oracle's.  Returns the worst
    error of a term in units of the sum of its absolute summands."""
    for name in ("oy", "ox", "nty", "ntx", "my", "mx"):
        assert got[name] == rec[name], name
    worst = 0.
    for i in range(n - 1):
        for ty in range(rec["nty"]):
            for tx in range(rec["ntx"]):
                at = (i, ty, tx)
                if rec["decided"][at] == -1:
                    assert got["decided"][at] == -1 and np.isnan(got["u"][at]) and np.isnan(got["logu"][at])
                    assert np.isnan(got["terms"][at]).all()
                    continue
                for t in range(5):
                    err, mag = abs(got["terms"][at][t] - rec["terms"][at][t]), rec["mags"][at][t]
                    assert err <= TERM_BAR * mag, (at, t, got["terms"][at][t], rec["terms"][at][t], mag)
                    if mag > 0.:
                        worst = max(worst, err / mag)
                assert got["u"][at] == PX.patch_uniform(seed, k, i, ty * rec["ntx"] + tx)       # bit for bit
                assert ulps(got["logu"][at], np.log(got["u"][at])) <= 4.
                own = 1 if got["logu"][at] < PX.log_ratio(got["terms"][at]) else 0
                assert got["decided"][at] == own == rec["decided"][at], at
    return worst


# ---- 1. mechanics ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(PX.GPU_CASES))
def test_patch_exchange_mechanics(key):
    """Worst errors on the MI355X: every term within 1.1e-15 of the sum of its
    absolute summands, the carried residual within 5.8e-15 of the data peak of a rebuilt one."""
    inp = PX.case_inputs(key)
    case, n, p = inp["case"], len(inp["betas"]), inp["p"]
    D, H, W = case["data"].shape
    fh, fw = case["fsf"].shape
    _, recs = PX.oracle_rounds(key)
    got = device_rounds(key)
    peak = np.nanmax(np.abs(case["data"]))
    attempts, accepts = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    worst_term = worst_res = 0.
    for k, rnd, rec in zip(PX.ROUNDS, got, recs):
        pat = rnd["patches"]
        worst_term = max(worst_term, check_record(pat, rec, inp["seed"], k, n))
        # the whole-cube record: the energies of the states before the round, no decision
        want_E = np.array([TO.reference_energy(err, case["var"], inp["betas"][r], case["data"])
                           for r, (_, err) in enumerate(rnd["before"])])
        np.testing.assert_allclose(rnd["last"]["energy"], want_E, rtol=1e-12, atol=0)
        assert (rnd["last"]["decided"] == -1).all() and np.isnan(rnd["last"]["u"]).all()
        # parameters: the accepted patches traded, everything else untouched, bit for bit
        want_params = [b[0].copy() for b in rnd["before"]]
        inside = [np.zeros((H, W), dtype=bool) for _ in range(n)]
        for i in range(n - 1):
            for ty in range(pat["nty"]):
                for tx in range(pat["ntx"]):
                    if pat["decided"][i, ty, tx] == -1:
                        continue
                    attempts[i] += 1
                    if pat["decided"][i, ty, tx] != 1:
                        continue
                    accepts[i] += 1
                    rect = PX.tile_rect(ty, tx, p, pat["oy"], pat["ox"], H, W)
                    for (y, x) in PX.patch_of(case["mask"], rect):
                        want_params[i][y, x] = rnd["before"][i + 1][0][y, x]
                        want_params[i + 1][y, x] = rnd["before"][i][0][y, x]
                    y0, y1, x0, x1 = PX.footprint(rect, fh, fw, H, W)
                    inside[i][y0:y1, x0:x1] = True
                    inside[i + 1][y0:y1, x0:x1] = True
        for r in range(n):
            np.testing.assert_array_equal(rnd["after"][r][0], want_params[r], err_msg="params %d" % r)
            before, after = rnd["before"][r][1], rnd["after"][r][1]
            np.testing.assert_array_equal(after[:, ~inside[r]], before[:, ~inside[r]], err_msg="residual %d" % r)
            if inside[r].any():
                assert not np.array_equal(after[:, inside[r]], before[:, inside[r]])
            rebuilt = rebuilt_residual(inp, rnd["after"][r][0])
            res = np.nanmax(np.abs(after - rebuilt)) / peak
            worst_res = max(worst_res, res)
            assert res <= RESIDUAL_BAR, (r, res)
            # and the oracle's own trade
            np.testing.assert_allclose(rnd["after"][r][0], rec["after"][r][0], rtol=0, atol=0)
        # counters: patches per pair; the whole-cube ones stand still, labels as created
        np.testing.assert_array_equal(rnd["counts"]["attempts"], attempts)
        np.testing.assert_array_equal(rnd["counts"]["accepts"], accepts)
        assert rnd["get"]["rounds"] == k + 1 and not rnd["get"]["attempts"].any() and not rnd["get"]["accepts"].any()
        np.testing.assert_array_equal(rnd["get"]["labels"], np.arange(n))
        np.testing.assert_array_equal(rnd["get"]["energy_n"], k + 1)
    print(key, "worst term error / sum of |summands| %.3g, worst carried - rebuilt residual / peak %.3g, "
          "attempts %s accepts %s" % (worst_term, worst_res, attempts, accepts))
    assert accepts.sum() >= 1


# ---- 2. the state stays consistent: more batched sweeps after the rounds --------------------------------

@functools.lru_cache(maxsize=None)
def device_sweeps(key, mh_small):
    inp = PX.case_inputs(key)
    engines = engines_of(inp, options=None if mh_small == 1 else {"mh_small": mh_small})
    try:
        _lib.mh_sweeps_batch(engines, 2, first_sweep=1)
        with _lib.TemperGroup(engines, inp["betas"], seed=inp["seed"], patch=inp["p"]) as group:
            decided = []
            for k in PX.ROUNDS:
                group.swap(k)
                decided.append(group.last_patches()["decided"])
            _lib.mh_sweeps_batch(engines, 3, first_sweep=3)
            return decided, snapshot(engines)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("key, mh_small", [("c1", 1), ("asym", 1), ("asym", 0), ("nolsf", 1)])
def test_state_is_consistent_after_patch_rounds(key, mh_small):
    """Sweeps 1, 2, rounds 0, 1, sweeps 3 .. 5: a stale proposal table, an unflushed pending layer
    or a residual that drifted from the parameters would show."""
    inp = PX.case_inputs(key)
    case = inp["case"]
    lad, recs = PX.sweep_schedule(key)
    decided, end = device_sweeps(key, mh_small)
    for k, rec in enumerate(recs):
        np.testing.assert_array_equal(decided[k], rec["decided"], err_msg="round %d" % k)
    live = case["mask"] == 1
    for r, (params, err) in enumerate(end):
        rebuilt = O.compute_error_in_one_step(case["data"], params, case["mask"], case["fsf"], case["lsf"])
        assert np.max(np.abs(err - rebuilt)) <= RESIDUAL_BAR * np.max(np.abs(case["data"])), r
        np.testing.assert_allclose(params[live], lad.states[r].params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="rung %d" % r)


# ---- 3. patch = 0 and no call at all: the whole-cube round as it was ----------------------------------------

def test_patch_zero_is_the_whole_cube_round_bit_for_bit():
    case = tempered_case("odd_depth")
    betas, seed = (1., 0.5, 0.2, 0.05), 77
    runs = []
    for how in ("never", "zero", "back"):
        engines = make_engines(case, betas, seed=seed)
        try:
            _lib.mh_sweeps_batch(engines, 3, first_sweep=1)
            with _lib.TemperGroup(engines, betas, seed=seed, patch=0 if how == "zero" else None) as group:
                if how == "back":
                    group.set_patch(2)
                    group.set_patch(0)
                assert group.patch is None
                lasts = []
                for k in range(4):
                    group.swap(k)
                    lasts.append(group.last())
                with pytest.raises(RuntimeError, match="exchanged no patches"):
                    group.last_patches()
                assert not group.get_patches()["attempts"].any()
                runs.append((lasts, snapshot(engines), group.get()))
                with pytest.raises(ValueError, match="patch size -1"):
                    group.set_patch(-1)
        finally:
            for e in engines:
                e.close()
    lad = TO.Ladder(case, betas, seed)
    for s in (1, 2, 3):
        lad.sweep(s)
    for k in range(4):
        decided, u, _, E = lad.swap(k)
        np.testing.assert_array_equal(runs[0][0][k]["decided"], decided)
        np.testing.assert_array_equal(runs[0][0][k]["u"], u)
        np.testing.assert_allclose(runs[0][0][k]["energy"], E, rtol=1e-9)
    assert sum(int((last["decided"] == 1).sum()) for last in runs[0][0]) >= 1
    for lasts, snap, got in runs[1:]:
        for a, b in zip(lasts, runs[0][0]):
            for name in ("energy", "u", "logu", "decided"):
                np.testing.assert_array_equal(a[name], b[name])
        for (pa, ea), (pb, eb) in zip(snap, runs[0][1]):
            np.testing.assert_array_equal(pa, pb)
            np.testing.assert_array_equal(ea, eb)
        for name in ("attempts", "accepts", "labels", "energy_mean", "energy_m2"):
            np.testing.assert_array_equal(got[name], runs[0][2][name])


# ---- 4. Run ---------------------------------------------------------------------------------------------

RUN_BETAS, BURN, EVERY = (1., 0.5, 0.25), 4, 2
ADAPT = dict(adapt_sweeps=4, adapt_window=2)


def run_schedule_kw(case, **more):
    return run_kw(case, tempering=dict(betas=RUN_BETAS, swap_every=2, patch=2), smoothness=dict(c=1.),
                  posterior_burn_in=BURN, posterior_every=EVERY, **dict(ADAPT, **more))


def replay(run, first, last):
    """The schedule of Run(tempering=dict(patch=2)) on the C ABI: one batched sweep per call, round
    s // 2 after every even sweep s."""
    n, (H, W) = len(RUN_BETAS), run.mask.shape
    engines = []
    try:
        for r, beta in enumerate(RUN_BETAS):
            eng = _lib.Engine(run.cube.data.shape, run.fsf.shape)
            engines.append(eng)
            eng.set_taps(run.fsf, run.lsf)
            eng.set_data(run.cube.data, run.variance_cube / beta, mask=run.mask)
            eng.set_params(run.chains[r][0])
            eng.mh_config(run.min_boundaries, run.max_boundaries, run.jumping_amplitude,
                          run.gibbs_apriori_variance, seed=31 + r, refresh_every=1000)
            if r == 0:
                eng.post_begin()
                eng.post_schedule(BURN, EVERY)
            eng.adapt_begin(0.25, ADAPT["adapt_window"], ADAPT["adapt_sweeps"], 2.0, (1e-3, 1e3))
            eng.prior_begin(prior.lam_of(run.smoothness))
        for eng in engines:
            eng.residual(fetch=False)
        chains = [np.full((last + 1, H, W, 3), np.nan) for _ in range(n)]
        dlogs = [np.full((last + 1, H, W), np.nan) for _ in range(n)]
        with _lib.TemperGroup(engines, RUN_BETAS, seed=31, patch=2) as group:
            for s in range(first, last + 1):
                _lib.mh_sweeps_batch(engines, 1, s, 1, chains, dlogs)
                if s % 2 == 0:
                    group.swap(s // 2)
            return dict(chains=chains, dlogs=dlogs, get=group.get(), counts=group.get_patches(),
                        patches=group.last_patches(), moments=engines[0].post_get(0), count=engines[0].post_count())
    finally:
        for e in engines:
            e.close()


def test_run_with_patch_is_its_schedule_on_the_c_abi():
    case, inst, cube = run_inputs()
    run = d3d.Run(cube, inst, max_iterations=12, **run_schedule_kw(case))
    assert run._batched and len(run.chains) == 3
    want = replay(run, 1, 11)
    for r in range(3):
        np.testing.assert_array_equal(run.chains[r][1:], want["chains"][r][1:], err_msg="chain %d" % r)
        np.testing.assert_array_equal(run.all_likelihoods[r][1:], want["dlogs"][r][1:], err_msg="dlog %d" % r)
    rep = run.tempering
    assert rep.patch == 2 and rep.labels is None and rep.rounds == 5 and rep.last_round == 5
    assert not rep.swap_attempts.any()
    np.testing.assert_array_equal(rep.patch_attempts, want["counts"]["attempts"])
    np.testing.assert_array_equal(rep.patch_accepts, want["counts"]["accepts"])
    np.testing.assert_array_equal(rep.energy_mean, want["get"]["energy_mean"])
    for name in ("terms", "u", "logu", "decided"):
        np.testing.assert_array_equal(rep.last_patches[name], want["patches"][name])
    assert rep.patch_attempts.min() > 0 and rep.patch_accepts.sum() > 0
    np.testing.assert_array_equal(rep.patch_rates, rep.patch_accepts / rep.patch_attempts)
    assert run.posterior.count == want["count"] == 4
    for a, b in zip(run.posterior.moments(0)[1:], want["moments"]):
        np.testing.assert_array_equal(a, b)


def test_checkpoint_round_trip_continues_the_rounds_and_refuses_another_patch(tmp_path):
    case, inst, cube = run_inputs()
    prefix = str(tmp_path / "ck")
    temper = dict(betas=RUN_BETAS, swap_every=2, patch=2)
    first = d3d.Run(cube, inst, max_iterations=8, write_every=4, checkpoint=prefix, tempering=temper, **run_kw(case))
    assert first.tempering.rounds == 3 and first.tempering.last_round == 3 and first.tempering.patch == 2
    state = np.load(prefix + "_state.npz")
    assert int(state["tempering_patch"]) == 2 and int(state["iteration"]) == 8
    maps = np.load(prefix + "_parameters.npy")
    for other in (dict(temper, patch=3), dict(temper, patch=None), dict(betas=RUN_BETAS, swap_every=2)):
        with pytest.raises(ValueError, match="resume_state was written with tempering patch=2"):
            d3d.Run(cube, inst, max_iterations=6, initial_parameters=maps, resume_state=prefix + "_state.npz",
                    tempering=other, **run_kw(case))
    again = d3d.Run(cube, inst, max_iterations=6, initial_parameters=maps, resume_state=prefix + "_state.npz",
                    tempering=temper, **run_kw(case))
    assert again.sweep_origin == 7
    rep = again.tempering
    assert rep.rounds == 3 and rep.last_round == 6                     # rounds 4, 5, 6: the numbering continues
    pat = rep.last_patches
    H, W = case["mask"].shape
    assert (pat["oy"], pat["ox"]) == PX.origin_shift(31, 6, 2)
    at = np.argwhere(pat["decided"] >= 0)[0]
    assert pat["u"][tuple(at)] == PX.patch_uniform(31, 6, int(at[0]), int(at[1]) * pat["ntx"] + int(at[2]))


# ---- 5. the coarse ladder swaps ------------------------------------------------------------------------------

def test_coarse_ladder_accepts_patches_where_the_whole_cube_rule_accepts_none():
    cfg = PX.COARSE
    case = make_case(cfg["name"])
    lad, recs = PX.coarse_schedule()
    engines = make_engines(case, cfg["betas"], seed=cfg["seed"], inits=TO.scaled_starts(case, cfg["scales"]))
    shown = set()
    try:
        with _lib.TemperGroup(engines, cfg["betas"], seed=cfg["seed"], patch=cfg["p"]) as group:
            for s in range(1, cfg["sweeps"] + 1):
                _lib.mh_sweeps_batch(engines, 1, first_sweep=s)
                group.swap(s - 1)
                pat, E = group.last_patches(), group.last()["energy"]
                np.testing.assert_array_equal(pat["decided"], recs[s - 1]["decided"], err_msg="round %d" % (s - 1))
                whole, _, _ = TO.decide(cfg["betas"], E, cfg["seed"], s - 1)      # from the same energies
                for i in TO.proposed_pairs(3, s - 1):
                    n_acc = int((pat["decided"][i] == 1).sum())
                    print("round", s - 1, "pair", i, "whole cube", whole[i], "patches", n_acc, "of",
                          int((pat["decided"][i] >= 0).sum()))
                    if whole[i] == 0:
                        assert n_acc >= 1
                        shown.add(i)
    finally:
        for e in engines:
            e.close()
    assert shown == {0, 1}


# ---- 6. the cold rung still samples the posterior ------------------------------------------------------------

N_SWEEPS = 16        # DESIGN.md section 8i's recipe: the smallest of 16, 32, ... at which the replicates scatter < 5 %


def test_cold_rung_energy_agrees_with_untempered_replicates():
    """`nolsf` started at the truth, betas (1, 0.7, 0.4), p = 2, a round after every sweep: the mean
    1/2 chi2 of rung 0 over the second half against 8 untempered replicates of the same length,
    within 3 replicate sigmas times sqrt(1 + 1/8)."""
    case, inst, cube = run_inputs("nolsf")
    kw = run_kw(case, initial_parameters=case["truth"], max_iterations=N_SWEEPS, refresh_every=0)

    def energy(run):
        half = run.chain[N_SWEEPS // 2:N_SWEEPS]
        shape = case["data"].shape
        return float(np.mean([0.5 * np.sum((case["data"] - run.simulate_convolved(shape, p)) ** 2 / case["var"])
                              for p in half]))

    reps = np.array([energy(d3d.Run(cube, inst, sweeps_per_call=N_SWEEPS, **dict(kw, seed=1000 + 17 * j)))
                     for j in range(8)])
    mean, sd = reps.mean(), reps.std(ddof=1)
    run = d3d.Run(cube, inst, tempering=dict(betas=(1., 0.7, 0.4), swap_every=1, patch=2), **kw)
    got = energy(run)
    print("N = %d: untempered replicates mean %.3f sd %.3f (%.2f %% of the mean); rung 0 with patch exchange %.3f = "
          "%+.2f sd; patch rates %s, rung energies %s" % (N_SWEEPS, mean, sd, 100. * sd / mean, got, (got - mean) / sd,
                                                        run.tempering.patch_rates, run.tempering.energy_mean))
    assert sd < 0.05 * mean
    assert run.tempering.patch_accepts.sum() > 0
    assert abs(got - mean) <= 3. * sd * np.sqrt(1. + 1. / 8.)
