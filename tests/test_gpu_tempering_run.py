"""
Run(tempering=...) with the keywords the README says it works with.

  * Run against a replay of its documented schedule on the C ABI (the engines as
    Run._create_engines and Run._arm make them, d3d_mh_sweeps_batch or one thread per rung,
    d3d_temper_swap): chains, jump scales, rung 0's moments and the report bit for bit.
  * The posterior is rung 0 BEFORE the exchange: the moments against numpy over the chain's own
    slots at MAP_RTOL = 1e-12, MEAN_RTOL = 1e-12 and STD_RTOL = 2e-12 of the peak
    (test_gpu_posterior.py::test_run_accumulates_the_chain_slots), the histogram counters exactly
    and the quantiles at EXTRACT_RTOL = 1e-13 of the range against tests/histogram_oracle.py
    (test_gpu_histograms.py::test_run_keeps_histograms_beside_the_moments, check_extraction).
  * No swap due: rung r is the lone Run of variance / beta_r and seed + r, bit for bit
    (test_gpu_tempering.py::test_run_with_no_swap_due_runs_the_rungs_as_they_are_alone).
  * prepare= and initial_search=: the carried residual against one rebuilt from the parameters at
    1e-11 x the data peak (test_gpu_tempering.py::test_state_is_consistent_after_exchanges).
  * A resumed run continues the uninterrupted one bit for bit.

Two keyword values differ from a first sketch of these cases because Run refuses them:
posterior_histograms needs pilot >= 2 (so pilot = 2), and posterior_burn_in may not lie before
adapt_sweeps (so adapt_sweeps = 4 with adapt_window = 2: two scale steps, the second at the sweep
the first accumulated exchange follows).
"""
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, ensemble, prior
from oracle import deconv3d_oracle as O
from tests import histogram_oracle as HO
from tests import tabulated_oracle as TAB
from tests import tempering_oracle as TO
from tests.test_gpu_histograms import EXTRACT_RTOL
from tests.test_gpu_multiplet import SHAPES, run_inputs
from tests.test_gpu_posterior import MAP_RTOL, MEAN_RTOL, STD_RTOL, close
from tests.test_gpu_prepare import run_inputs as raw_inputs

pytestmark = pytest.mark.gpu

BETAS = (1., .7, .5)
SEED = 31
BURN, EVERY, PILOT, SPAN = 4, 2, 2, 6.
ADAPT = dict(adapt_sweeps=4, adapt_window=2)
RESIDUAL_BAR = 1e-11


@functools.lru_cache(maxsize=None)
def schedule_case(name):
    """(instrument, cube, variance, model, starts).  The starts make an accepted swap of rung 0
    certain within the accumulated span: rung 0 begins with every line centre 5 channels off the
    truth, rungs 1 and 2 at the truth, so after sweep 4 (round 2, pair 0) the hotter rung 1 lies
    far lower: delta > 0, accepted whatever u."""
    if name == "doublet":
        inst, cube, var, truth = run_inputs(32, 16, 16, *SHAPES["doublet"], seed=5)
        model = d3d.GaussianMultipletLineModel(*SHAPES["doublet"])
    elif name == "table":
        inst, cube, var, truth = run_inputs(32, 16, 16, [0.], [1.], seed=5)
        model = d3d.TabulatedLineModel(*TAB.profile_G())
    else:                            # beyond 256 channels the batch refuses: one thread per rung
        inst, cube, var, truth = run_inputs(300, 6, 7, *SHAPES["doublet"], seed=5, fsf=O.gaussian_fsf_image(1.0))
        model = d3d.GaussianMultipletLineModel(*SHAPES["doublet"])
    off = truth.copy()
    off[..., 1] += 5.
    return inst, cube, var, model, np.stack([off, truth, truth])


def schedule_kw(var, model, starts):
    return dict(variance=var, model=model, initial_parameters=starts, seed=SEED, min_acceptance_rate=0.,
                max_iterations=12, tempering=dict(betas=BETAS, swap_every=2), smoothness=dict(c=1.),
                posterior_burn_in=BURN, posterior_every=EVERY,
                posterior_histograms=dict(pilot=PILOT, span=SPAN), **ADAPT)


@functools.lru_cache(maxsize=None)
def schedule_run(name):
    inst, cube, var, model, starts = schedule_case(name)
    return d3d.Run(cube, inst, **schedule_kw(var, model, starts))


def replay(run, batched):
    """The schedule of Run(tempering=...) on the C ABI: sweeps 1 .. 11 one per call, the exchange of
    round s // 2 after every even sweep s.  Returns what Run hands back, and every round's `last`."""
    n, H, W = len(BETAS), run.mask.shape[0], run.mask.shape[1]
    engines = []
    try:
        for r, beta in enumerate(BETAS):
            eng = _lib.Engine(run.cube.data.shape, run.fsf.shape)
            engines.append(eng)
            eng.set_taps(run.fsf, run.lsf)
            eng.set_data(run.cube.data, run.variance_cube / beta, mask=run.mask)
            eng.set_line_shape(*run.line_shape)
            if run.line_table is not None:
                eng.set_line_table(*run.line_table)
            eng.set_params(run.chains[r][0])
            eng.mh_config(run.min_boundaries, run.max_boundaries, run.jumping_amplitude,
                          run.gibbs_apriori_variance, seed=SEED + r, refresh_every=1000)
            if r == 0:
                eng.post_begin()
                eng.post_schedule(BURN, EVERY)
                eng.hist_begin(PILOT, SPAN)
            eng.adapt_begin(0.25, ADAPT["adapt_window"], ADAPT["adapt_sweeps"], 2.0, (1e-3, 1e3))
            eng.prior_begin(prior.lam_of(run.smoothness))
        for eng in engines:
            eng.residual(fetch=False)
        chains = [np.full((12, H, W, 3), np.nan) for _ in range(n)]
        dlogs = [np.full((12, H, W), np.nan) for _ in range(n)]
        for r in range(n):
            chains[r][0] = run.chains[r][0]
        lasts = {}
        with _lib.TemperGroup(engines, BETAS, seed=SEED) as group:
            for s in range(1, 12):
                if batched:
                    _lib.mh_sweeps_batch(engines, 1, s, 1, chains, dlogs)
                else:
                    ensemble.sweep_chains(engines, 1, s, 1, chains, dlogs)
                if s % 2 == 0:
                    group.swap(s // 2)
                    lasts[s // 2] = group.last()
            got = group.get()
        out = dict(chains=chains, dlogs=dlogs, scales=[e.adapt_get()[0] for e in engines], got=got, lasts=lasts,
                   moments=[engines[0].post_get(which) for which in (0, 1, 2)],
                   count=engines[0].post_count(), hist=engines[0].hist_get(), hist_count=engines[0].hist_count())
        return out
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("name", ["doublet", "table", "deep"])
def test_run_is_the_schedule_of_the_c_abi(name):
    run = schedule_run(name)
    batched = name != "deep"
    assert run._batched is batched and len(run.chains) == 3 and not run._host_model
    assert (run.line_table is not None) == (name == "table")
    want = replay(run, batched)
    for r in range(3):
        np.testing.assert_array_equal(run.chains[r], want["chains"][r], err_msg="chain %d" % r)
        np.testing.assert_array_equal(run.all_likelihoods[r][1:], want["dlogs"][r][1:], err_msg="dlog %d" % r)
        np.testing.assert_array_equal(run.jump_scales[r], want["scales"][r], err_msg="jump scale %d" % r)
        assert not np.isnan(run.chains[r][:, run.mask == 1]).any()
    assert run.adapted_until == 4 and len(run.posteriors) == 1
    assert run.posterior.count == want["count"] == 4
    for which in (0, 1, 2):
        for a, b in zip(run.posterior.moments(which)[1:], want["moments"][which]):
            np.testing.assert_array_equal(a, b)
    assert run.posterior.histograms.count == want["hist_count"] == 4 - PILOT
    for a, b in zip((run.posterior.histograms.counts, run.posterior.histograms.tails, run.posterior.histograms.range),
                    want["hist"]):
        np.testing.assert_array_equal(a, b)
    rep, got = run.tempering, want["got"]
    assert rep.rounds == got["rounds"] == 5 and rep.last_round == 5 and rep.swap_every == 2
    np.testing.assert_array_equal(rep.betas, BETAS)
    np.testing.assert_array_equal(rep.swap_attempts, got["attempts"])
    np.testing.assert_array_equal(rep.swap_accepts, got["accepts"])
    np.testing.assert_array_equal(rep.labels, got["labels"])
    np.testing.assert_array_equal(rep.energy_count, got["energy_n"])
    np.testing.assert_array_equal(rep.energy_mean, got["energy_mean"])
    np.testing.assert_array_equal(rep.energy_std, np.sqrt(got["energy_m2"] / 4.))
    for key in ("energy", "u", "logu", "decided"):
        np.testing.assert_array_equal(rep.last[key], want["lasts"][5][key])
    np.testing.assert_array_equal(rep.swap_attempts, [2, 3])             # rounds 2, 4 | rounds 1, 3, 5
    # rung 0 took part in an accepted swap within the accumulated span (sweeps 4 .. 10): round 2
    decided = {k: list(last["decided"]) for k, last in want["lasts"].items()}
    print(name, "decided", decided, "labels", rep.labels)
    assert decided[2][0] == 1
    assert not np.array_equal(run.jump_scales[0], run.jump_scales[1])


def test_the_posterior_is_rung_0_before_the_exchange():
    """Rung 0's samples are its chain slots 4, 6, 8, 10, each saved BEFORE the exchange that
    follows its sweep: between slots 4 and 6 rung 0 receives rung 1's state, and the moments are
    those of the slots, not of what the rung held after the exchange."""
    run = schedule_run("doublet")
    inst, cube, var, model, starts = schedule_case("doublet")
    slots = np.asarray(run.chain[BURN::EVERY])
    pm = run.posterior
    assert pm.count == len(slots) == 4
    close(pm.parameters_mean, slots.mean(axis=0), MAP_RTOL, "parameters mean")
    err = np.max(np.abs(pm.parameters_std - slots.std(axis=0, ddof=1)))
    print("parameters std: max|d| = %.3g of the peak %.3g (bar %.1g)" % (err, np.max(np.abs(slots)), MAP_RTOL))
    assert err <= MAP_RTOL * np.max(np.abs(slots))
    cubes = np.stack([run.simulate_convolved(cube.data.shape, s) for s in slots])
    close(pm.convolved_mean, cubes.mean(axis=0), MEAN_RTOL, "convolved mean")
    err, peak = np.max(np.abs(pm.convolved_std - cubes.std(axis=0, ddof=1))), np.max(np.abs(cubes))
    print("convolved std: max|d| = %.3g of the peak %.3g (bar %.1g)" % (err, peak, STD_RTOL))
    assert err <= STD_RTOL * peak
    # the swap shows in the slots: the centres moved by the 5 channels between slots 4 and 6
    live = run.mask == 1
    assert np.median(np.abs(slots[1][live][:, 1] - slots[0][live][:, 1])) > 4.
    assert np.median(np.abs(slots[2][live][:, 1] - slots[1][live][:, 1])) < 1.
    # the histograms: ranges frozen after the pilot's two samples, the other two counted
    ph = run.posterior.histograms
    assert (ph.pilot, ph.span) == (PILOT, SPAN) and ph.count == pm.count - PILOT == 2
    flux_k = HO.flux_factor(SHAPES["doublet"][1])
    lo, hi = ph.range[..., 0], ph.range[..., 1]
    want_bins, want_tails = HO.count(HO.series(slots[PILOT:], flux_k), lo, hi)
    np.testing.assert_array_equal(ph.counts, want_bins)
    np.testing.assert_array_equal(ph.tails, want_tails)
    assert ph.counts.sum() + ph.tails.sum() > 0
    scale = np.maximum(np.abs(lo), np.abs(hi))
    lo68, hi68 = ph.interval(0.68)
    for got, q in ((ph.median, 0.5), (lo68, 0.16), (hi68, 0.84)):
        want = HO.quantile(ph.counts, ph.tails, ph.range, q)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        worst = float((np.abs(got - want)[ok] / np.maximum(scale[ok], 1e-300)).max())
        print("quantile %.2f: worst %.3g of max(|lo|, |hi|) (bar %.1g)" % (q, worst, EXTRACT_RTOL))
        assert ok.any() and worst <= EXTRACT_RTOL


def test_run_with_no_swap_due_and_every_keyword_runs_the_rungs_as_they_are_alone():
    inst, cube, var, _ = run_inputs(32, 16, 16, *SHAPES["doublet"], seed=5)
    model = d3d.GaussianMultipletLineModel(*SHAPES["doublet"])
    kw = dict(model=model, max_iterations=9, min_acceptance_rate=0., smoothness=dict(c=1.), posterior_burn_in=BURN,
              **ADAPT)
    run = d3d.Run(cube, inst, variance=var, seed=SEED, tempering=dict(betas=BETAS, swap_every=20), **kw)
    assert run.tempering.rounds == 0 and len(run.posteriors) == 1 and run.posterior.count == 9 - BURN
    for r, beta in enumerate(BETAS):
        lone = d3d.Run(cube, inst, variance=var / beta, seed=SEED + r, **kw)
        np.testing.assert_array_equal(run.chains[r], lone.chain, err_msg="chain %d" % r)
        np.testing.assert_array_equal(run.jump_scales[r], lone.jump_scale, err_msg="jump scale %d" % r)
        np.testing.assert_array_equal(run.acceptance_maps[r], lone.acceptance_map, err_msg="acceptance %d" % r)
        assert len(np.unique(lone.jump_scale[run.mask == 1])) > 1 and lone.adapted_until == 4
        if r == 0:
            for which in (0, 1, 2):
                for a, b in zip(run.posterior.moments(which)[1:], lone.posterior.moments(which)[1:]):
                    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(run.chains[0][-1], run.chains[1][-1])


def test_prepare_and_initial_search_with_tempering():
    inst, cube = raw_inputs()
    kw = dict(prepare=True, initial_search=True, max_iterations=9, seed=3, min_acceptance_rate=0.)
    run = d3d.Run(cube, inst, tempering=dict(betas=BETAS, swap_every=2), **kw)
    plain = d3d.Run(cube, inst, **kw)
    assert run.search is not None and run.prepared is not None and run.search.detected.any()
    assert run.tempering.rounds == 4 and len(run.chains) == 3
    np.testing.assert_array_equal(run.chain[0], plain.chain[0])
    np.testing.assert_array_equal(run.cube.data, plain.cube.data)
    assert not np.array_equal(run.chains[1][0], run.chains[0][0])       # (the hotter rungs start jittered)
    peak = np.max(np.abs(run.cube.data))
    for r, eng in enumerate(run.engines):
        params, carried = eng.get_params(), eng.download_slot(_lib.SLOT_ERR)
        rebuilt = O.compute_error_in_one_step(run.cube.data, params, run.mask, run.fsf, run.lsf)
        worst = np.max(np.abs(carried - rebuilt))
        print("rung %d: carried - rebuilt residual %.3g of the data peak (bar %.1g)" % (r, worst / peak, RESIDUAL_BAR))
        assert worst <= RESIDUAL_BAR * peak
        assert np.isfinite(run.chains[r][:, run.mask == 1]).all()


def test_a_resumed_tempered_run_continues_bit_for_bit(tmp_path):
    """12 sweeps in one go against 6 + 6 over a checkpoint, with adapt_sweeps (8, window 4: the
    checkpoint falls in the middle of the second window) and swap_every = 2.  refresh_every = 3
    divides the 6 sweeps done: the uninterrupted run rebuilt every rung's residual from its
    parameters at the end of sweep 6, the exchange of round 3 then traded from-scratch residuals,
    and the resumed run rebuilds them from the checkpoint's (traded) parameters -- the same
    numbers, so the chains agree bit for bit and not only to rounding."""
    inst, cube, var, _ = run_inputs(32, 12, 12, *SHAPES["doublet"], seed=6)
    model = d3d.GaussianMultipletLineModel(*SHAPES["doublet"])
    name = str(tmp_path / "ck")
    kw = dict(variance=var, model=model, seed=SEED, min_acceptance_rate=0., refresh_every=3,
              tempering=dict(betas=BETAS, swap_every=2), adapt_sweeps=8, adapt_window=4)
    whole = d3d.Run(cube, inst, max_iterations=13, **kw)
    first = d3d.Run(cube, inst, max_iterations=7, write_every=7, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    assert int(state["iteration"]) == 7 and int(state["n_chains"]) == 3 and int(state["adapt_n_win"][0]) == 2
    assert first.tempering.last_round == 3
    second = d3d.Run(cube, inst, max_iterations=7, initial_parameters=name + "_parameters.npy",
                     resume_state=name + "_state.npz", **kw)
    assert second.sweep_origin == 6
    for r in range(3):
        np.testing.assert_array_equal(first.chains[r], whole.chains[r][:7], err_msg="first, rung %d" % r)
        np.testing.assert_array_equal(second.chains[r][0], np.load(name + "_parameters.npy")[r])
        np.testing.assert_array_equal(second.chains[r][1:], whole.chains[r][7:], err_msg="resumed, rung %d" % r)
        np.testing.assert_array_equal(second.jump_scales[r], whole.jump_scales[r])
    # the round numbering continues: rounds 4, 5, 6 with the uniforms of the uninterrupted run
    rep = second.tempering
    assert rep.rounds == 3 and rep.last_round == 6 == whole.tempering.last_round and whole.tempering.rounds == 6
    for key in ("energy", "u", "logu", "decided"):
        np.testing.assert_array_equal(rep.last[key], whole.tempering.last[key])
    assert rep.last["u"][0] == TO.swap_uniform(SEED, 6, 0)
    np.testing.assert_array_equal(first.tempering.swap_attempts + rep.swap_attempts, whole.tempering.swap_attempts)
    np.testing.assert_array_equal(first.tempering.swap_accepts + rep.swap_accepts, whole.tempering.swap_accepts)
