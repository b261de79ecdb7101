"""
Replica exchange between tempered chains on the device (csrc/d3d_temper.hip, Run(tempering=...)):
the three kernels of a round against numpy and the Philox reference, bit for bit where the
contract says so; the state of every rung after exchanges against a residual rebuilt from scratch
and against the tempering oracle's replay of the same schedule; the Run plumbing (off by default,
rungs as chains, refusals, checkpoints); and the cold rung's energy against untempered replicates.
"""
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import tempering_oracle as TO
from tests.cases import make_case

pytestmark = pytest.mark.gpu

BETAS = (1., 0.5, 0.2, 0.05)
SEED = 77
ROUNDS = 6


@functools.lru_cache(maxsize=None)
def tempered_case(name):
    """The parity case; `c1` with ONE constant variance (the uniform path of k_temper_energy)."""
    case = dict(make_case(name))
    if name == "c1":
        case["var"] = np.full(case["data"].shape, float(np.median(case["var"])))
    return case


def make_engines(case, betas, options=None, seed=SEED, inits=None, refresh_every=0):
    """One engine per rung: variance / beta_r, seed + r, start ``inits[r]`` (default: the case's)."""
    D, H, W = case["D"], case["H"], case["W"]
    uniform = bool(np.all(case["var"] == case["var"].flat[0]))
    engines = []
    for r, b in enumerate(betas):
        eng = _lib.Engine((D, H, W), case["fsf"].shape, options=options)
        engines.append(eng)
        eng.set_taps(case["fsf"], case["lsf"])
        if uniform:
            eng.set_data(case["data"], None, var_scalar=float(case["var"].flat[0] / b), mask=case["mask"])
            assert eng.variance_is_uniform()
        else:
            eng.set_data(case["data"], case["var"] / b, mask=case["mask"])
        eng.set_params(case["init"] if inits is None else inits[r])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, float(case["max_b"][0] ** 2), seed=seed + r,
                      refresh_every=refresh_every)
        eng.residual(fetch=False)
    return engines


def snapshot(engines):
    return [(e.get_params(), e.download_slot(_lib.SLOT_ERR)) for e in engines]


@functools.lru_cache(maxsize=None)
def device_schedule(name, mh_small=1):
    """3 batched sweeps, 6 rounds with every engine's state before and after each, 3 more sweeps."""
    case = tempered_case(name)
    engines = make_engines(case, BETAS, options=None if mh_small == 1 else {"mh_small": mh_small})
    try:
        _lib.mh_sweeps_batch(engines, 3, first_sweep=1)
        rounds = []
        with _lib.TemperGroup(engines, BETAS, seed=SEED) as group:
            start = group.get()
            for k in range(ROUNDS):
                before = snapshot(engines)
                group.swap(k)
                rounds.append(dict(before=before, last=group.last(), after=snapshot(engines), get=group.get()))
            _lib.mh_sweeps_batch(engines, 3, first_sweep=4)
            end = snapshot(engines)
        return dict(start=start, rounds=rounds, end=end)
    finally:
        for e in engines:
            e.close()


@functools.lru_cache(maxsize=None)
def oracle_schedule(name):
    """The same schedule on the tempering oracle (computed once, shared, left unchanged)."""
    case = tempered_case(name)
    lad = TO.Ladder(case, BETAS, SEED)
    for s in (1, 2, 3):
        lad.sweep(s)
    for k in range(ROUNDS):
        lad.swap(k)
    for s in (4, 5, 6):
        lad.sweep(s)
    return lad


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


# ---- 1. exchange mechanics --------------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd_depth", "c1"])
def test_exchange_mechanics(name):
    case = tempered_case(name)
    got = device_schedule(name)
    n = len(BETAS)
    b = np.array(BETAS)
    np.testing.assert_array_equal(got["start"]["labels"], np.arange(n))
    assert got["start"]["rounds"] == 0 and not got["start"]["attempts"].any()
    labels, attempts, accepts = list(range(n)), np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    n_acc = n_rej = 0
    for k, rnd in enumerate(got["rounds"]):
        last = rnd["last"]
        # energies: numpy on the downloaded residuals (another order of the sum: 1/2 chi2 class)
        want_E = np.array([0.5 * np.sum(err ** 2 / (case["var"] / BETAS[r])) / BETAS[r]
                           for r, (_, err) in enumerate(rnd["before"])])
        print(name, "round", k, "E", last["energy"], "rel", np.abs(last["energy"] / want_E - 1.), "u", last["u"],
              "decided", last["decided"])
        np.testing.assert_allclose(last["energy"], want_E, rtol=1e-12, atol=0)
        for i in range(n - 1):
            if i % 2 != k % 2:                      # only pairs of the round's parity were proposed
                assert last["decided"][i] == -1 and np.isnan(last["u"][i]) and np.isnan(last["logu"][i])
                continue
            assert last["u"][i] == TO.swap_uniform(SEED, k, i)                  # bit for bit
            assert ulps(last["logu"][i], np.log(last["u"][i])) <= 4.
            delta = (b[i] - b[i + 1]) * (last["energy"][i] - last["energy"][i + 1])
            assert last["decided"][i] == (1 if last["logu"][i] < delta else 0)   # from the device's own E, logu
            attempts[i] += 1
            if last["decided"][i] == 1:
                accepts[i] += 1
                labels[i], labels[i + 1] = labels[i + 1], labels[i]
                n_acc += 1
            else:
                n_rej += 1
        # accepted pairs hold each other's former state, everything else is untouched: bit for bit
        src = list(range(n))
        for i in range(n - 1):
            if last["decided"][i] == 1:
                src[i], src[i + 1] = i + 1, i
        for r in range(n):
            np.testing.assert_array_equal(rnd["after"][r][0], rnd["before"][src[r]][0], err_msg="params %d" % r)
            np.testing.assert_array_equal(rnd["after"][r][1], rnd["before"][src[r]][1], err_msg="residual %d" % r)
        np.testing.assert_array_equal(rnd["get"]["labels"], labels)
        np.testing.assert_array_equal(rnd["get"]["attempts"], attempts)
        np.testing.assert_array_equal(rnd["get"]["accepts"], accepts)
        assert rnd["get"]["rounds"] == k + 1
        np.testing.assert_array_equal(rnd["get"]["energy_n"], k + 1)
    assert n_acc >= 1 and n_rej >= 1, (n_acc, n_rej)
    # the energy moments: Welford over the rounds, of the state at the rung BEFORE each exchange
    E = np.array([rnd["last"]["energy"] for rnd in got["rounds"]])
    final = got["rounds"][-1]["get"]
    np.testing.assert_allclose(final["energy_mean"], E.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(final["energy_m2"], ((E - E.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-9,
                               atol=1e-18 * np.max(E) ** 2)


# ---- 2. the state stays consistent after an exchange ----------------------------------------------

@pytest.mark.parametrize("name, mh_small", [("odd_depth", 1), ("c1", 1), ("odd_depth", 0)])
def test_state_is_consistent_after_exchanges(name, mh_small):
    """3 more batched sweeps after the rounds: a stale proposal table or an unflushed pending layer
    would show in the carried residual or in the parameters."""
    case = tempered_case(name)
    got = device_schedule(name, mh_small)
    lad = oracle_schedule(name)
    live = case["mask"] == 1
    for k, rnd in enumerate(got["rounds"]):      # the oracle took the device's decisions
        np.testing.assert_array_equal(rnd["last"]["decided"], lad.history[k][2], err_msg="round %d" % k)
    for r, (params, err) in enumerate(got["end"]):
        rebuilt = O.compute_error_in_one_step(case["data"], params, case["mask"], case["fsf"], case["lsf"])
        assert np.max(np.abs(err - rebuilt)) <= 1e-11 * np.max(np.abs(case["data"])), r
        np.testing.assert_allclose(params[live], lad.states[r].params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="rung %d" % r)


# ---- 3. / 4. Run ------------------------------------------------------------------------------

def run_inputs(name="odd_depth"):
    case = make_case(name)
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(case["lsf"]), fsf=ImageFieldSpreadFunction(case["fsf"]))
    cube = d3d.MUSE().build_cube(case["data"])
    return case, inst, cube


def run_kw(case, **more):
    kw = dict(variance=case["var"], mask=case["mask"], seed=31, min_acceptance_rate=0.)
    kw.update(more)
    return kw


def test_run_with_no_swap_due_runs_the_rungs_as_they_are_alone():
    case, inst, cube = run_inputs()
    run = d3d.Run(cube, inst, max_iterations=8, tempering=dict(betas=(1, .3), swap_every=9), **run_kw(case))
    cold = d3d.Run(cube, inst, max_iterations=8, **run_kw(case))
    hot = d3d.Run(cube, inst, max_iterations=8, **run_kw(case, variance=case["var"] / .3, seed=32))
    np.testing.assert_array_equal(run.chain, cold.chain)
    np.testing.assert_array_equal(run.chains[1], hot.chain)
    np.testing.assert_array_equal(run.likelihoods, cold.likelihoods)
    np.testing.assert_array_equal(run.parameters, cold.parameters)           # rung 0 alone
    assert run.rhat is None and len(run.chains) == 2
    rep = run.tempering
    assert rep.rounds == 0 and rep.last_round is None and rep.last is None
    assert not rep.swap_attempts.any() and np.isnan(rep.swap_rates).all() and np.isnan(rep.energy_mean).all()
    np.testing.assert_array_equal(rep.betas, [1., .3])
    np.testing.assert_array_equal(rep.labels, [0, 1])


def test_run_off_by_default_refusals_and_checkpoint_round_trip(tmp_path):
    case, inst, cube = run_inputs()
    plain = d3d.Run(cube, inst, max_iterations=8, **run_kw(case))
    none = d3d.Run(cube, inst, max_iterations=8, tempering=None, **run_kw(case))
    np.testing.assert_array_equal(none.chain, plain.chain)
    np.testing.assert_array_equal(none.likelihoods, plain.likelihoods)
    assert none.tempering is None and plain.tempering is None

    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    temper = dict(betas=(1., 0.5, 0.2), swap_every=2)
    with pytest.raises(ValueError, match="the rungs take the chains' place"):
        d3d.Run(cube, inst, max_iterations=8, chains=2, tempering=temper, **run_kw(case))
    with pytest.raises(NotImplementedError, match="tempering=: the line model Lorentzian"):
        d3d.Run(cube, inst, max_iterations=8, model=Lorentzian, tempering=temper, **run_kw(case))

    # a checkpoint after sweep 7 (write_every = 4: iterations 4 and 8), resumed
    prefix = str(tmp_path / "ck")
    first = d3d.Run(cube, inst, max_iterations=8, write_every=4, checkpoint=prefix, tempering=temper,
                    **run_kw(case))
    assert first.tempering.rounds == 3 and first.tempering.last_round == 3      # after sweeps 2, 4, 6
    np.testing.assert_array_equal(first.tempering.swap_attempts, [1, 2])         # rounds 1, 2, 3: parities 1, 0, 1
    state = np.load(prefix + "_state.npz")
    np.testing.assert_array_equal(state["tempering_betas"], [1., 0.5, 0.2])
    assert int(state["swap_every"]) == 2 and int(state["n_chains"]) == 3 and int(state["iteration"]) == 8
    maps = np.load(prefix + "_parameters.npy")
    assert maps.shape == (3,) + first.chain.shape[1:]
    for other in (dict(betas=(1., 0.5, 0.25), swap_every=2), dict(betas=(1., 0.5, 0.2), swap_every=3), None):
        with pytest.raises(ValueError, match="resume_state was written with"):
            d3d.Run(cube, inst, max_iterations=6, initial_parameters=maps, resume_state=prefix + "_state.npz",
                    tempering=other, **(run_kw(case) if other is not None else run_kw(case, chains=3)))
    again = d3d.Run(cube, inst, max_iterations=6, initial_parameters=maps, resume_state=prefix + "_state.npz",
                    tempering=temper, **run_kw(case))
    # this segment's sweep s is sweep s + 7 of the whole run: exchanges after its sweeps 1, 3, 5 are
    # rounds 4, 5, 6 -- the numbering continues, no uniform of rounds 1 .. 3 is drawn again
    assert again.sweep_origin == 7
    rep = again.tempering
    assert rep.rounds == 3 and rep.last_round == 6
    np.testing.assert_array_equal(rep.swap_attempts, [2, 1])                      # rounds 4, 6 | round 5
    np.testing.assert_array_equal(rep.last["decided"] == -1, [False, True])
    assert rep.last["u"][0] == TO.swap_uniform(31, 6, 0) and np.isnan(rep.last["u"][1])
    assert rep.last["u"][0] not in [TO.swap_uniform(31, k, 0) for k in range(4)]


def test_group_refusals():
    case = tempered_case("odd_depth")
    engines = make_engines(case, (1., 0.5, 0.2))
    other = _lib.Engine((case["D"], case["H"], case["W"] + 1), case["fsf"].shape)
    try:
        for betas in ((0.9, 0.5, 0.2), (1., 0.5, 0.5), (1., 0.5, 0.), (1., 0.5, float("nan")), (1., 0.2, 0.5)):
            with pytest.raises(ValueError, match="betas"):
                _lib.TemperGroup(engines, betas)
        with pytest.raises(ValueError, match="2 to 64 rungs"):
            _lib.TemperGroup(engines[:1], (1.,))
        with pytest.raises(ValueError, match="appears twice"):
            _lib.TemperGroup([engines[0], engines[0]], (1., 0.5))
        with pytest.raises((ValueError, RuntimeError)):                         # no data / another shape
            _lib.TemperGroup([engines[0], other], (1., 0.5))
        engines[2].set_parts([(0, 6, 0, 10), (6, 12, 0, 10)], [0, 1])
        with pytest.raises(NotImplementedError, match="tiled or partitioned"):
            _lib.TemperGroup(engines, (1., 0.5, 0.2))
        with _lib.TemperGroup(engines[:2], (1., 0.5)) as group:
            with pytest.raises(RuntimeError, match="no exchange round yet"):
                group.last()
            engines[1].set_params(case["init"])                                 # (invalidates the residual)
            with pytest.raises(RuntimeError, match="no valid carried residual"):
                group.swap(0)
            assert group.get()["rounds"] == 0
    finally:
        other.close()
        for e in engines:
            e.close()


# ---- 5. the cold rung still samples the posterior ---------------------------------------------------

N_SWEEPS = 16        # the smallest of 16, 32, 64, ... at which the replicates scatter < 5 %


def test_cold_rung_energy_agrees_with_untempered_replicates():
    """`nolsf` started at the truth.  The mean over the second half of the chain of rung 0's energy
    1/2 sum (data - model)^2 / var against 8 untempered runs with other seeds: within 4 of their
    replicate standard deviations of their mean (a sign error in the rule drives rung 0 to the hot
    rungs' energies, tens of sigma away)."""
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
    run = d3d.Run(cube, inst, tempering=dict(betas=(1., 0.85, 0.7), swap_every=1), **kw)
    got = energy(run)
    print("N = %d: untempered replicates mean %.3f sd %.3f (%.2f %% of the mean); rung 0 tempered %.3f = %+.2f sd; "
          "swap rates %s, rung energies %s" % (N_SWEEPS, mean, sd, 100. * sd / mean, got, (got - mean) / sd,
                                               run.tempering.swap_rates, run.tempering.energy_mean))
    assert sd < 0.05 * mean
    assert run.tempering.swap_accepts.sum() > 0                  # (else the run shows nothing: change the seed)
    assert abs(got - mean) <= 4. * sd
    assert np.all(np.diff(run.tempering.energy_mean) > 0.)       # and the hotter the rung, the higher its energy
