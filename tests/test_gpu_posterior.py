"""
GPU tests of the posterior moments kept on the device (d3d_post_*, k_post_accum,
Run(posterior_burn_in=...)):

  * against the ORACLE: the chain is streamed out (keep_one_in = 1), the oracle builds the clean
    and the convolved cube of every scheduled chain slot on the host, and the device's means and
    standard deviations are compared with numpy's over those stacks;
  * identities: one sample is build_clean / forward bit for bit; the chain does not notice the
    accumulation; chains=R; split calls; refusals; Jensen's inequality for chi2.

Tolerances (derived, DESIGN.md sections 5 and 8b): means 1e-12 of the cube's peak -- a mean of
samples that each meet the project's cube tolerance meets it; standard deviations 2e-12 of the
cube's peak -- the sample standard deviation is the norm of a projection of the sample vector
over sqrt(n - 1), so per-sample errors <= delta move it by at most delta sqrt(n / (n - 1)), and
Welford's recurrence adds O(n 2^-52) of the value; parameter and flux moments 1e-12 of the map's
peak (they are the chain's own numbers).
"""
import ctypes
import os

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior
from oracle import deconv3d_oracle as O
from tests.cases import make_case
from tests.test_gpu_multiplet import QUAD, SHAPES, multiplet, run_inputs

pytestmark = pytest.mark.gpu

MEAN_RTOL = 1e-12
STD_RTOL = 2e-12
MAP_RTOL = 1e-12
LINES = {"single": ([0.], [1.]), "doublet": SHAPES["doublet"], "quad": QUAD}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bounded_case(D, H, W, fsf, lsf, seed):
    data, var, mask, truth, init, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=seed)
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, init=init,
                min_b=min_b, max_b=max_b)


def oracle_case(name):
    """The cases of the oracle comparison: (case, line, every)."""
    if name == "fixture":            # the reference's 24 x 30 x 21 fixture with its own 15 x 15 FSF
        g = np.load(os.path.join(GOLDEN, "ref_mat_fixture.npz"))
        data, fsf = g["data"], np.ascontiguousarray(g["fsf"])
        D, H, W = data.shape
        assert (D, H, W) == (21, 30, 24) and fsf.shape == (15, 15)     # 24 x 30 spaxels, 21 channels
        rng = np.random.default_rng(11)
        min_b, max_b = O.model_min_boundaries(), O.model_max_boundaries(data, fsf)
        init = min_b + (max_b - min_b) * rng.random((H, W, 3))
        init[..., 2] = np.maximum(init[..., 2], 0.3)
        mask = np.ones((H, W))
        mask[3, 4] = mask[29, 20] = 0
        case = dict(D=D, H=H, W=W, fsf=fsf, lsf=None, data=data, var=g["var"], mask=mask, init=init,
                    min_b=min_b, max_b=max_b)
        return case, "single", 1
    if name in ("c1", "c1_every3", "c1_doublet", "c1_quad"):       # BASELINE config 1: 32 x 16 x 16
        return make_case("c1"), {"c1": "single", "c1_every3": "single", "c1_doublet": "doublet",
                                 "c1_quad": "quad"}[name], 3 if name in ("c1_every3", "c1_quad") else 1
    if name == "cube64":             # 64^3, Moffat 11 x 11 (k_mh_small)
        return bounded_case(64, 64, 64, O.moffat_cropped(11, 3.0, 2.5), O.gaussian_lsf_vector(64, 0.9088), 5), \
            "single", 1
    if name == "odd_depth":          # 21 channels: the pad channel of the device layout stays 0
        return make_case("odd_depth"), "doublet", 1
    if name == "d30":                # not 32 / 64 / 128: the LSF is applied in k_lines, TMP0 is not the clean cube
        return make_case("d30"), "single", 3
    if name == "deep":               # > 1024 channels: the z-blocked / deep kernel forms
        return bounded_case(1100, 6, 7, O.gaussian_fsf_image(1.0), O.muse_like_lsf(1100), 9), "doublet", 1
    if name == "nan_masked":         # NaN voxels: their spaxels are masked by the device
        case = make_case("c1")
        case["data"] = case["data"].copy()
        case["data"][3, 2, 5] = case["data"][17, 9, 9] = case["data"][31, 15, 0] = np.nan
        return case, "single", 1
    if name == "uniform":            # one constant variance: the uniform-variance sweep kernels
        case = make_case("c1")
        case["var"] = np.full(case["var"].shape, float(np.median(case["var"])))
        return case, "doublet", 3
    raise KeyError(name)


ORACLE_CASES = ["fixture", "c1", "c1_every3", "c1_doublet", "c1_quad", "cube64", "odd_depth", "d30", "deep",
                "nan_masked", "uniform"]


def engine_for(case, line="single", options=None, seed=4321, refresh_every=0, parts=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    eng.set_line_shape(*LINES[line])
    if parts is not None:
        eng.set_parts(*parts)
    eng.set_params(case["init"])
    ra = float(case["max_b"][0] ** 2)
    eng.mh_config(case["min_b"], case["max_b"], 0.1, ra, seed=seed, refresh_every=refresh_every)
    return eng


def flux_of(params, line):
    return params[..., 0] * params[..., 2] * (np.sqrt(2. * np.pi) * float(np.sum(LINES[line][1])))


def close(got, want, rtol, what):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(got - want)))
    print("%s: max|d| = %.3g = %.3g of the peak %.3g (bar %.1g)" % (what, err, err / scale, scale, rtol))
    assert err <= rtol * scale, "%s: max|d| = %g vs %g * %g" % (what, err, rtol, scale)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_moments_match_numpy_over_the_oracle_cubes_of_the_chain(name, monkeypatch):
    case, line, every = oracle_case(name)
    monkeypatch.setattr(O, "gaussian_line", multiplet(*LINES[line]))
    dims = (case["D"], case["H"], case["W"])
    big = name in ("cube64", "deep")
    first, n_sweeps = (2, 5) if big else (3, 12 if every == 1 else 15)
    mask = np.array(case["mask"], dtype=np.float64)
    mask[np.isnan(case["data"]).any(axis=0)] = 0
    with engine_for(case, line) as eng:
        eng.post_begin()
        eng.post_schedule(first, every)
        chain = np.full((n_sweeps + 1,) + dims[1:] + (3,), np.nan)
        eng.mh_sweeps(n_sweeps, 1, 1, chain)
        slots = list(range(first, n_sweeps + 1, every))
        assert eng.post_count() == len(slots) >= 3
        got = [eng.post_get(which) for which in (0, 1, 2)]
    n = len(slots)
    clean = np.stack([O.simulate_clean(dims, chain[s], mask) for s in slots])
    conv = np.stack([O.simulate_convolved(dims, chain[s], mask, case["fsf"], case["lsf"]) for s in slots])
    maps = np.stack([np.concatenate((chain[s], flux_of(chain[s], line)[..., None]), axis=-1) for s in slots])
    for label, stack, (mean, m2), rt_mean, rt_std in (("clean", clean, got[1], MEAN_RTOL, STD_RTOL),
                                                       ("convolved", conv, got[2], MEAN_RTOL, STD_RTOL)):
        assert not np.isnan(mean).any() and not np.isnan(m2).any() and (m2 >= 0.).all()
        peak = np.max(np.abs(stack))
        err = np.max(np.abs(mean - stack.mean(axis=0)))
        print("%s %s mean: max|d| = %.3g (%.3g of the peak)" % (name, label, err, err / peak))
        assert err <= rt_mean * peak, "%s mean: %g vs peak %g" % (label, err, peak)
        err = np.max(np.abs(posterior.std_from_m2(n, m2) - stack.std(axis=0, ddof=1)))
        print("%s %s std: max|d| = %.3g (%.3g of the peak)" % (name, label, err, err / peak))
        assert err <= rt_std * peak, "%s std: %g vs peak %g" % (label, err, peak)
    dead = mask != 1
    assert (got[1][0][:, dead] == 0.).all() and (got[1][1][:, dead] == 0.).all()     # masked spaxels: 0
    mean, m2 = got[0]
    for k, label in enumerate(("a", "c", "w", "F")):
        close(mean[..., k], maps.mean(axis=0)[..., k], MAP_RTOL, "%s %s mean" % (name, label))
        peak = np.max(np.abs(maps[..., k]))
        err = np.max(np.abs(posterior.std_from_m2(n, m2[..., k]) - maps.std(axis=0, ddof=1)[..., k]))
        print("%s %s std: max|d| = %.3g (%.3g of the peak)" % (name, label, err, err / peak))
        assert err <= MAP_RTOL * peak, "%s std: %g vs peak %g" % (label, err, peak)


@pytest.mark.parametrize("name,line", [("c1", "single"), ("d30", "doublet"), ("odd_depth", "quad"), ("deep", "single")])
def test_one_sample_is_the_forward_model_bit_for_bit(name, line):
    case = oracle_case(name)[0]
    with engine_for(case, line) as eng:
        eng.post_begin()
        assert eng.post_count() == 0
        eng.post_accumulate()
        assert eng.post_count() == 1
        clean_mean, clean_m2 = eng.post_get(1)
        conv_mean, conv_m2 = eng.post_get(2)
        map_mean, map_m2 = eng.post_get(0)
        np.testing.assert_array_equal(clean_mean, eng.build_clean())
        np.testing.assert_array_equal(conv_mean, eng.forward())
        np.testing.assert_array_equal(map_mean[..., :3], eng.get_params())
        assert (clean_m2 == 0.).all() and (conv_m2 == 0.).all() and (map_m2 == 0.).all()
        pm = posterior.PosteriorMoments.from_engine(eng)
        assert pm.count == 1 and np.isnan(pm.clean_std).all() and np.isnan(pm.flux_std).all()
        np.testing.assert_array_equal(pm.convolved_mean, conv_mean)


def chain_state(eng, n_sweeps, first=1, calls=None):
    """Run the sweeps; everything the chain carries afterwards."""
    acc = 0
    for n in (calls or [n_sweeps]):
        acc += eng.mh_sweeps(n, first, 1)
        first += n
    return eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(), acc


def big_case():
    """A shape whose colour launches fill the chip (two pending layers)."""
    fsf = O.moffat_cropped(11, 3.0, 2.5)
    lsf = O.gaussian_lsf_vector(64, 0.9088)
    rng = np.random.default_rng(77)
    D, H, W = 64, 256, 256              # 24 x 24 window positions per colour: more than half the chip's slots
    truth = O.synthetic_truth(D, H, W, rng)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        eng.set_params(truth)
        clean = eng.forward()
    sigma = 0.05 * 10.0 * np.max(fsf)
    data = clean + rng.normal(0., sigma, size=clean.shape)
    var = (sigma * (0.5 + rng.random(clean.shape))) ** 2
    min_b, max_b = O.model_min_boundaries(), O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=np.ones((H, W)), init=init,
                min_b=min_b, max_b=max_b)


def unnoticed_case(name):
    """(case, engine keywords, sweeps)"""
    if name == "chip_filling":
        return big_case(), {}, 4
    if name == "small_64":
        return oracle_case("cube64")[0], {}, 5
    if name == "partitioned":
        case = make_case("moffat")      # 64 x 20 x 18, 11 x 11: two parts, two phases
        rects = np.array([[0, 20, 0, 9], [0, 20, 9, 18]], dtype=np.int32)
        return case, dict(parts=(rects, np.array([0, 1], dtype=np.int32))), 5
    if name == "z_blocked":
        case = make_case("tile_deep")   # 600 channels
        return case, {}, 3
    if name == "uniform":
        return oracle_case("uniform")[0], dict(line="doublet"), 6
    if name == "refresh":
        return make_case("c1"), dict(refresh_every=4), 10
    raise KeyError(name)


@pytest.mark.parametrize("name", ["chip_filling", "small_64", "partitioned", "z_blocked", "uniform", "refresh"])
def test_the_chain_does_not_notice_the_accumulation(name):
    case, kw, n_sweeps = unnoticed_case(name)
    with engine_for(case, **kw) as eng:
        if name == "chip_filling":
            assert eng.mh_layers() == 2
        if name == "z_blocked":
            assert case["D"] > 512
        plain = chain_state(eng, n_sweeps)
    with engine_for(case, **kw) as eng:
        eng.post_begin()
        eng.post_schedule(2, 1)
        watched = chain_state(eng, n_sweeps)
        assert eng.post_count() == n_sweeps - 1
    for a, b, what in zip(plain, watched, ("parameters", "carried residual", "log ratios", "accepted")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert plain[3] > 0


def test_batched_chains_do_not_notice_and_accumulate_their_own():
    case = make_case("c1")
    R, n_sweeps, first = 3, 9, 4

    def run(schedule):
        engines = [engine_for(case, "doublet", seed=100 + r, refresh_every=5) for r in range(R)]
        try:
            if schedule:
                for r, eng in enumerate(engines):
                    if r != 1:                      # chain 1 has no schedule: it accumulates nothing
                        eng.post_begin()
                        eng.post_schedule(first, 2)
            chains = [np.full((n_sweeps + 1, case["H"], case["W"], 3), np.nan) for _ in range(R)]
            acc = _lib.mh_sweeps_batch(engines, n_sweeps, 1, 1, chains)
            state = [(e.get_params(), e.download_slot(_lib.SLOT_ERR), e.get_dlog()) for e in engines]
            moments = [(e.post_count(), e.post_get(0), e.post_get(1), e.post_get(2)) if schedule and r != 1 else None
                       for r, e in enumerate(engines)]
            return acc, state, chains, moments
        finally:
            for eng in engines:
                eng.close()

    acc0, state0, chains0, _ = run(False)
    acc1, state1, chains1, moments = run(True)
    assert acc0 == acc1
    for r in range(R):
        np.testing.assert_array_equal(chains0[r], chains1[r])
        for a, b in zip(state0[r], state1[r]):
            np.testing.assert_array_equal(a, b)
    # each chain's moments are those of its own engine run alone
    for r in (0, 2):
        with engine_for(case, "doublet", seed=100 + r, refresh_every=5) as eng:
            eng.post_begin()
            eng.post_schedule(first, 2)
            eng.mh_sweeps(n_sweeps, 1, 1)
            assert eng.post_count() == moments[r][0] == len(range(first, n_sweeps + 1, 2))
            for which in (0, 1, 2):
                for a, b in zip(eng.post_get(which), moments[r][1 + which]):
                    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("calls", [[1, 7, 2], [1] * 10, [3, 3, 4]])
def test_split_calls_give_the_same_moments_bit_for_bit(calls):
    case = make_case("moffat")

    def run(split):
        with engine_for(case, refresh_every=6) as eng:
            eng.post_begin()
            eng.post_schedule(3, 2)
            chain_state(eng, 10, calls=split)
            return eng.post_count(), [eng.post_get(which) for which in (0, 1, 2)]

    n0, whole = run([10])
    n1, parts = run(calls)
    assert n0 == n1 == 4
    for a, b in zip(whole, parts):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def run_kw(var, **more):
    kw = dict(variance=var, max_iterations=12, seed=31, min_acceptance_rate=0.)
    kw.update(more)
    return kw


@pytest.mark.parametrize("sweeps_per_call", [1, 64])
def test_run_accumulates_the_chain_slots(sweeps_per_call):
    inst, cube, var, _ = run_inputs(32, 16, 16, *SHAPES["doublet"], seed=5)
    model = d3d.GaussianMultipletLineModel(*SHAPES["doublet"])
    plain = d3d.Run(cube, inst, model=model, **run_kw(var, sweeps_per_call=sweeps_per_call))
    assert plain.posterior is None and plain.posteriors is None
    run = d3d.Run(cube, inst, model=model, posterior_burn_in=4, posterior_every=3,
                  **run_kw(var, sweeps_per_call=sweeps_per_call))
    np.testing.assert_array_equal(plain.chain, run.chain)         # the run does not notice either
    np.testing.assert_array_equal(plain.convolved_cube.data, run.convolved_cube.data)
    slots = run.chain[4::3]
    pm = run.posterior
    assert pm.count == len(slots) == 3 and run.posteriors == [pm]
    close(pm.parameters_mean, slots.mean(axis=0), MAP_RTOL, "parameters mean")
    err = np.max(np.abs(pm.parameters_std - slots.std(axis=0, ddof=1)))
    assert err <= MAP_RTOL * np.max(np.abs(slots)), "parameters std: %g" % err
    cubes = np.stack([run.simulate_convolved(cube.data.shape, s) for s in slots])
    close(pm.convolved_mean, cubes.mean(axis=0), MEAN_RTOL, "convolved mean")
    for arr in (pm.clean_mean, pm.clean_std, pm.convolved_mean, pm.convolved_std, pm.flux_mean, pm.flux_std,
                pm.parameters_std):
        assert not np.isnan(arr).any()
    out = pm.convolved_cube()
    assert out.z is cube.z and out.meta is cube.meta and out.data.shape == cube.data.shape


@pytest.mark.parametrize("batched", [True, False])
def test_run_chains_are_the_single_runs_and_pool(batched):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    B, R = 5, 3
    many = d3d.Run.__new__(d3d.Run)
    many._batched = batched                 # both transports of _sweep_chains
    many.__init__(cube, inst, chains=R, posterior_burn_in=B, **run_kw(var))
    assert many._batched is batched and len(many.posteriors) == R
    stacks = {1: [], 2: []}
    for r in range(R):
        one = d3d.Run(cube, inst, posterior_burn_in=B, **run_kw(var, seed=31 + r))
        np.testing.assert_array_equal(one.chain, many.chains[r])
        assert one.posterior.count == many.posteriors[r].count == 12 - B
        for which in (0, 1, 2):
            for a, b in zip(one.posterior.moments(which)[1:], many.posteriors[r].moments(which)[1:]):
                np.testing.assert_array_equal(a, b)
        for s in many.chains[r][B:]:
            stacks[1].append(many.simulate_clean(cube.data.shape, s))
            stacks[2].append(many.simulate_convolved(cube.data.shape, s))
    pm = many.posterior
    assert pm.count == R * (12 - B)
    slots = np.concatenate([ch[B:] for ch in many.chains])
    close(pm.parameters_mean, slots.mean(axis=0), MAP_RTOL, "pooled parameters mean")
    close(pm.clean_mean, np.mean(stacks[1], axis=0), MEAN_RTOL, "pooled clean mean")
    close(pm.convolved_mean, np.mean(stacks[2], axis=0), MEAN_RTOL, "pooled convolved mean")
    peak = np.max(np.abs(stacks[2]))
    err = np.max(np.abs(pm.convolved_std - np.std(stacks[2], axis=0, ddof=1)))
    assert err <= STD_RTOL * peak, (err, peak)


def test_run_that_stops_before_the_burn_in_has_no_sample(caplog):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    with caplog.at_level("WARNING", logger="deconv3d"):
        run = d3d.Run(cube, inst, posterior_burn_in=40, **run_kw(var))
    assert run.posterior.count == 0
    assert np.isnan(run.posterior.clean_mean).all() and np.isnan(run.posterior.flux_std).all()
    assert len([r for r in caplog.records if "posterior_burn_in" in r.getMessage()]) == 1


def test_refusals_by_status_code_and_exception():
    case = make_case("c1")
    lib = _lib.load()
    dims = (case["D"], case["H"], case["W"])

    def last():
        return lib.d3d_last_error().decode()

    with _lib.Engine(dims, case["fsf"].shape) as eng:
        ctx = eng._ctx
        n = ctypes.c_int64(-1)
        assert lib.d3d_post_count(ctx, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.d3d_post_schedule(ctx, 1, 1) == _lib.ERR_STATE          # not begun
        assert lib.d3d_post_accumulate(ctx) == _lib.ERR_STATE
        assert lib.d3d_post_get(ctx, 1, None, None) == _lib.ERR_STATE
        for what in (-1, 4):
            assert lib.d3d_post_begin(ctx, what) == _lib.ERR_INVALID and "what" in last()
        with pytest.raises(ValueError):
            eng.post_begin(7)
        assert lib.d3d_post_begin(ctx, _lib.POST_CLEAN) == 0
        assert lib.d3d_post_accumulate(ctx) == _lib.ERR_STATE and "parameters" in last()
        with pytest.raises(RuntimeError):
            eng.post_accumulate()
        eng.set_params(case["init"])
        eng.post_accumulate()                                               # clean only: no taps needed
        assert eng.post_count() == 1
        assert lib.d3d_post_get(ctx, 2, None, None) == _lib.ERR_STATE and "convolved" in last()
        with pytest.raises(RuntimeError):
            eng.post_get(2)
        for which in (-1, 3):
            assert lib.d3d_post_get(ctx, which, None, None) == _lib.ERR_INVALID
        assert lib.d3d_post_schedule(ctx, 1, 0) == _lib.ERR_INVALID and "every" in last()
        assert lib.d3d_post_schedule(ctx, -1, 1) == _lib.ERR_INVALID
        with pytest.raises(ValueError):
            eng.post_schedule(3, 0)
        eng.post_begin(_lib.POST_CONVOLVED)                                 # begun again: afresh
        assert eng.post_count() == 0
        assert lib.d3d_post_accumulate(ctx) == _lib.ERR_STATE and "taps" in last()
        eng.post_end()
        assert lib.d3d_post_accumulate(ctx) == _lib.ERR_STATE
        eng.post_end()                                                      # twice is fine
    with _lib.Engine(dims, case["fsf"].shape) as eng:                       # a tile
        eng.set_tile(0, 0, case["W"], 0, case["H"], 0, case["W"])
        assert lib.d3d_post_begin(eng._ctx, 3) == _lib.ERR_UNSUPPORTED and "tile" in last()
        with pytest.raises(NotImplementedError):
            eng.post_begin()
    assert lib.d3d_post_begin(None, 3) == _lib.ERR_INVALID


def test_a_new_model_resets_the_moments():
    case = make_case("c1")
    with engine_for(case) as eng:
        eng.post_begin()
        eng.post_schedule(1, 1)
        eng.mh_sweeps(3, 1, 1)
        assert eng.post_count() == 3
        eng.set_line_shape(*LINES["doublet"])
        assert eng.post_count() == 0
        eng.post_accumulate()
        np.testing.assert_array_equal(eng.post_get(1)[0], eng.build_clean())   # nothing of the old model left
        assert (eng.post_get(2)[1] == 0.).all()
        eng.set_taps(case["fsf"], case["lsf"])
        assert eng.post_count() == 0
        eng.post_accumulate()
        eng.set_data(case["data"], case["var"], mask=case["mask"])
        assert eng.post_count() == 0
        eng.mh_sweeps(2, 4, 1)                                                  # the schedule survives a reset
        assert eng.post_count() == 2


def test_phase_driven_callers_accumulate_themselves():
    case = make_case("moffat")
    rects = np.array([[0, 20, 0, 9], [0, 20, 9, 18]], dtype=np.int32)
    phases = np.array([0, 1], dtype=np.int32)
    with engine_for(case, parts=(rects, phases)) as eng:
        eng.post_begin()
        eng.post_schedule(1, 1)
        eng.mh_sweeps(4, 1, 1)
        want = [eng.post_get(which) for which in (0, 1, 2)]
    with engine_for(case, parts=(rects, phases)) as eng:
        eng.post_begin()
        for s in range(1, 5):
            for ph in (0, 1):
                eng.mh_phase(ph, s)
            eng.post_accumulate()
        assert eng.post_count() == 4
        for which in (0, 1, 2):
            for a, b in zip(want[which], eng.post_get(which)):
                np.testing.assert_array_equal(a, b)


def test_the_mean_cube_fits_where_the_mean_map_does_not():
    """Jensen: chi2 is convex in the model cube, so chi2(E[cube]) <= E[chi2(cube)].  The 14 x 14 [OII]
    case under the 11 x 11 Moffat FSF of tests/test_gpu_multiplet.py::test_oii_science_check's
    docstring, where single spaxels are not identified: the mean CUBE fits, the cube of the mean
    MAP does not.  Only the two inequalities are asserted; DESIGN.md section 8b has the figures."""
    blank = d3d.MUSE().build_cube(np.zeros((64, 14, 14)))
    oii = d3d.GaussianMultipletLineModel.from_rest_wavelengths(blank, [0.372603, 0.372882], [1.0, 1.4], 0.7)
    inst, cube, var, truth = run_inputs(64, 14, 14, oii.offsets, oii.ratios, seed=8, noise=0.02)
    start = truth.copy()
    start[..., 0] *= 0.8
    start[..., 1] += 0.3
    start[..., 2] *= 1.15
    B = 480                               # the last 20 % of 600: what run.parameters averages
    run = d3d.Run(cube, inst, model=oii, variance=var, max_iterations=600, seed=21, min_acceptance_rate=0.,
                  initial_parameters=start, posterior_burn_in=B)

    def half_chi2(sim):
        return 0.5 * float(np.sum((cube.data - sim) ** 2 / var))

    assert run.posterior.count == 600 - B
    of_mean_cube = half_chi2(run.posterior.convolved_mean)
    of_samples = float(np.mean([half_chi2(run.simulate_convolved(cube.data.shape, s)) for s in run.chain[B:]]))
    of_mean_map = half_chi2(run.convolved_cube.data)
    print("half chi2 over %d voxels: mean cube %.1f, mean over the %d samples %.1f, cube of the mean map %.1f"
          % (cube.data.size, of_mean_cube, run.posterior.count, of_samples, of_mean_map))
    assert of_mean_cube <= of_samples * (1. + 1e-10)
    assert of_mean_cube < of_mean_map
