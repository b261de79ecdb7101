"""
GPU tests of the region posteriors kept on the device (d3d_region_*, d3d_region.hip,
Run(regions=...)) against tests/region_oracle.py, the numpy restatement of their contract.

  * (F, C, S) are + * / sqrt in a fixed order: compared BIT FOR BIT.
  * Spectra go through exp: within MEAN_RTOL = 1e-12 of the spectrum's peak, test_gpu_posterior's
    bar and derivation (at most 700 terms here, each within a few ulp of exp); bit for bit with a
    TabulatedLineModel, whose curve is the same IEEE operations on both sides.  The second moment
    is compared as test_gpu_posterior compares it: the standard deviation from M2 within
    STD_RTOL = 2e-12 of the peak (per-sample errors <= delta move it by at most
    delta sqrt(n / (n - 1)), Welford adds O(n 2^-52) of the value).
"""
import ctypes

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior, regions
from oracle import deconv3d_oracle as O
from tests import region_oracle as RO
from tests import tabulated_oracle as TO
from tests.cases import make_case
from tests.test_gpu_multiplet import run_inputs
from tests.test_gpu_posterior import LINES, MEAN_RTOL, STD_RTOL, chain_state, engine_for, run_kw

pytestmark = pytest.mark.gpu

SAMPLES = 5
SQRT_2PI = np.sqrt(2. * np.pi)


def flux_k_of(line):
    s = 0.
    for r in LINES[line][1]:
        s += r
    return SQRT_2PI * s


def live_mask(case):
    mask = np.array(case["mask"], dtype=np.float64)
    mask[np.isnan(case["data"]).any(axis=0)] = 0
    return mask


def random_params(case, rng, n=SAMPLES):
    """n maps of in-bounds parameters (the widths away from 0, as the cases' starts)."""
    p = case["min_b"] + (case["max_b"] - case["min_b"]) * rng.random((n, case["H"], case["W"], 3))
    p[..., 2] = np.maximum(p[..., 2], 0.3)
    return p


def layouts(case):
    """name -> (labels, K): the label layouts of the scalar test at this case's field."""
    H, W = case["H"], case["W"]
    mask = live_mask(case)
    y, x = np.mgrid[0:H, 0:W]
    out = {"singletons": (np.arange(1, H * W + 1).reshape(H, W), H * W),
           "whole": (np.ones((H, W), dtype=int), 1),
           "checkerboard": ((y + x) % 2 + 1, 2)}
    bordered = regions.blocks((H, W), 4).astype(int)
    bordered[[0, -1], :] = 0
    bordered[:, [0, -1]] = 0
    out["blocks_with_border"] = (bordered, int(max(bordered.max(), 1)))      # (tiny: one region, no member)
    dead = np.where(mask == 1, 1, 2)
    out["all_masked"] = (dead, 2)                                           # region 2: masked members only, or none
    live = np.flatnonzero(mask.reshape(-1) == 1)
    if live.size >= 129:        # exactly one full chunk, and one full chunk plus one member, scattered
        pick = np.random.default_rng(64).permutation(live)[:129]
        hand = np.zeros(H * W, dtype=int)
        hand[pick[:64]] = 1
        hand[pick[64:]] = 2
        out["64_and_65"] = (hand.reshape(H, W), 2)
    return out


def accumulate(eng, maps):
    for p in maps:
        eng.set_params(p)
        eng.post_accumulate()


# ---- 1. scalars bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["c1", "odd_depth", "tiny", "moffat"])
def test_scalars_are_the_oracles_bit_for_bit(name):
    case = make_case(name)
    mask = live_mask(case)
    maps = random_params(case, np.random.default_rng(7))
    fk = flux_k_of("single")
    seen = set()
    with engine_for(case) as eng:
        eng.post_begin(0)
        for layout, (labels, K) in layouts(case).items():
            eng.region_begin(labels, K, capacity=SAMPLES, spectra=False)
            assert eng.region_count() == (0, 0)
            accumulate(eng, maps)
            assert eng.region_count() == (SAMPLES, SAMPLES)
            series, mean, m2, sizes = eng.region_get()
            assert mean is None and m2 is None and series.shape == (SAMPLES, K, 3)
            want_members = RO.members(labels, mask, K)
            np.testing.assert_array_equal(sizes, [len(m) for m in want_members], err_msg=layout)
            np.testing.assert_array_equal(series, RO.series(maps, labels, mask, K, fk), err_msg=layout)
            seen.update(int(s) for s in sizes)
            if layout == "singletons":      # F is the map's own a w flux_k of that sample
                F = ((maps[..., 0] * maps[..., 2]) * fk).reshape(SAMPLES, -1)
                np.testing.assert_array_equal(series[..., 0], np.where(mask.reshape(-1) == 1, F, 0.))
            if layout == "all_masked":
                assert sizes[1] == 0 and (series[:, 1, 0] == 0.).all() and np.isnan(series[:, 1, 1:]).all()
            if layout == "64_and_65":
                assert sizes.tolist() == [64, 65]
    if name == "moffat":
        assert 357 in seen          # five full chunks and a short one
    if name == "tiny":
        assert 0 in seen


def test_singleton_flux_is_the_moments_map_after_one_sample():
    case = make_case("c1")
    mask = live_mask(case)
    labels = np.arange(1, 257).reshape(16, 16)
    with engine_for(case) as eng:
        eng.post_begin(0)
        eng.region_begin(labels, 256, capacity=1, spectra=False)
        eng.set_params(case["init"])
        eng.post_accumulate()
        F_map = eng.post_get(0)[0][..., 3]
        series = eng.region_get()[0]
    np.testing.assert_array_equal(series[0, :, 0].reshape(16, 16)[mask == 1], F_map[mask == 1])
    # one member: C = (F c) / F, c to the rounding of a product and a quotient
    np.testing.assert_allclose(series[0, :, 1].reshape(16, 16)[mask == 1], case["init"][..., 1][mask == 1], rtol=2.3e-16)
    # S = sqrt(F (w^2 + (c - C)^2) / F), w to the rounding of a product, a quotient and a root
    np.testing.assert_allclose(series[0, :, 2].reshape(16, 16)[mask == 1], case["init"][..., 2][mask == 1], rtol=4e-16)


# ---- 2. spectra ---------------------------------------------------------------------------------

def spectra_layouts(case):
    all_of = layouts(case)
    return {k: all_of[k] for k in ("whole", "blocks_with_border", "all_masked")}


def check_spectra(eng, maps, labels, mask, K, D, unit_line, what, exact=False):
    """Five samples into the spectra of a context whose regions are begun; returns (mean, m2)."""
    accumulate(eng, maps)
    n = len(maps)
    _, mean, m2, _ = eng.region_get()
    assert mean.shape == m2.shape == (K, D) and eng.region_count()[0] == n
    samples = np.stack([RO.spectra(p, labels, mask, K, D, unit_line) for p in maps])
    want_mean, want_m2 = RO.welford(samples)
    if exact:
        np.testing.assert_array_equal(mean, want_mean, err_msg=what)
        np.testing.assert_array_equal(m2, want_m2, err_msg=what)
        return mean, m2
    peak = max(float(np.max(np.abs(samples))), 1e-300)
    err = float(np.max(np.abs(mean - want_mean)))
    print("%s spectrum mean: max|d| = %.3g = %.3g of the peak %.3g" % (what, err, err / peak, peak))
    assert err <= MEAN_RTOL * peak, "%s mean: %g vs peak %g" % (what, err, peak)
    err = float(np.max(np.abs(posterior.std_from_m2(n, m2) - posterior.std_from_m2(n, want_m2))))
    print("%s spectrum std: max|d| = %.3g = %.3g of the peak" % (what, err, err / peak))
    assert err <= STD_RTOL * peak, "%s std: %g vs peak %g" % (what, err, peak)
    err = float(np.max(np.abs(posterior.std_from_m2(n, m2) - samples.std(axis=0, ddof=1))))
    assert err <= STD_RTOL * peak, "%s std against numpy's: %g vs peak %g" % (what, err, peak)
    return mean, m2


def region_sums(cube, labels, K):
    """(K, D): a (D, H, W) cube summed over every region (masked spaxels hold 0 in a clean cube)."""
    return np.stack([cube[:, labels == k + 1].sum(axis=1) for k in range(K)])


def within(got, want, what):
    """MEAN_RTOL of the spectra's peak."""
    peak = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(got - want)))
    print("%s: max|d| = %.3g = %.3g of the peak %.3g" % (what, err, err / peak, peak))
    assert err <= MEAN_RTOL * peak, "%s: %g vs peak %g" % (what, err, peak)


@pytest.mark.parametrize("name", ["c1", "odd_depth", "tiny", "moffat"])
def test_spectra_match_the_oracle_and_the_clean_cube(name):
    case = make_case(name)
    mask = live_mask(case)
    D = case["D"]
    maps = random_params(case, np.random.default_rng(8))
    with engine_for(case) as eng:
        eng.post_begin(_lib.POST_CLEAN)
        for layout, (labels, K) in spectra_layouts(case).items():
            eng.region_begin(labels, K, capacity=0, spectra=True)          # no series: the spectra alone
            # one sample: K = 1 is the spatial sum of d3d_build_clean's cube
            eng.set_params(maps[0])
            eng.post_accumulate()
            assert eng.region_count() == (1, 0) and eng.region_get()[0].shape == (0, K, 3)
            one, one_m2 = eng.region_get()[1:3]
            assert (one_m2 == 0.).all()
            within(one, region_sums(eng.build_clean(), labels, K), "%s %s against build_clean" % (name, layout))
            eng.region_begin(labels, K, capacity=0, spectra=True)          # afresh
            mean, _ = check_spectra(eng, maps, labels, mask, K, D, RO.gaussian_unit_line(), "%s %s" % (name, layout))
            within(mean, region_sums(eng.post_get(1)[0], labels, K), "%s %s against clean_mean" % (name, layout))
            if layout == "all_masked":
                assert (mean[1] == 0.).all()


def test_spectra_of_a_deep_cube_take_ten_channel_steps():
    """tile_deep, D = 600: ten 64-channel steps, the last partial; fed parameters only, no chain."""
    case = make_case("tile_deep")
    mask = live_mask(case)
    D = case["D"]
    assert D == 600
    maps = random_params(case, np.random.default_rng(9))
    with engine_for(case) as eng:
        eng.post_begin(0)
        for layout in ("whole", "blocks_with_border"):
            labels, K = layouts(case)[layout]
            eng.region_begin(labels, K, capacity=SAMPLES)
            check_spectra(eng, maps, labels, mask, K, D, RO.gaussian_unit_line(), "tile_deep %s" % layout)
            np.testing.assert_array_equal(eng.region_get()[0], RO.series(maps, labels, mask, K, flux_k_of("single")))
        eng.region_begin(labels, K, capacity=0)
        eng.set_params(maps[0])
        eng.post_accumulate()
        within(eng.region_get()[1], region_sums(eng.build_clean(), labels, K), "tile_deep against build_clean")


@pytest.mark.parametrize("key,doublet", [("S", False), ("C", True)])
def test_spectra_with_a_table_are_bit_for_bit(key, doublet):
    from tests.test_gpu_tabulated import DOUBLET, model_of, set_model
    case = make_case("odd_depth")
    mask = live_mask(case)
    model = model_of(key, doublet)
    tab, sup = TO.PROFILES[key]()
    line = TO.line(tab, sup, *(DOUBLET if doublet else ([0.], [1.])))
    maps = random_params(case, np.random.default_rng(10), 3)
    labels, K = layouts(case)["checkerboard"]
    fk = model.table_integral * float(np.sum(model.ratios))
    with engine_for(case) as eng:
        set_model(eng, model)
        eng.post_begin(0)
        eng.region_begin(labels, K, capacity=3)
        check_spectra(eng, maps, labels, mask, K, case["D"], lambda z, c, w: line(z, 1., c, w), key, exact=True)
        series = eng.region_get()[0]
    want = RO.series(maps, labels, mask, K, fk)
    np.testing.assert_array_equal(series, want)


# ---- 3. multiplet -------------------------------------------------------------------------------

@pytest.mark.parametrize("line", ["doublet", "quad"])
def test_a_multiplet_takes_its_flux_factor_and_its_shape(line):
    case = make_case("c1")
    mask = live_mask(case)
    maps = random_params(case, np.random.default_rng(11))
    labels, K = layouts(case)["blocks_with_border"]
    with engine_for(case, line) as eng:
        eng.post_begin(0)
        eng.region_begin(labels, K, capacity=SAMPLES)
        check_spectra(eng, maps, labels, mask, K, case["D"], RO.gaussian_unit_line(*LINES[line]), line)
        series = eng.region_get()[0]
    np.testing.assert_array_equal(series, RO.series(maps, labels, mask, K, flux_k_of(line)))
    single = RO.series(maps, labels, mask, K, flux_k_of("single"))
    assert not np.array_equal(series[..., 0], single[..., 0])


# ---- 3b. regions of more than 64 chunks: the folds' second trips -----------------------------------

def wide_field():
    """96 x 96 x 7 (odd depth, 3 x 3 taps) with a label map and a mask that give, in row-major order:
    region 1 of exactly 4096 unmasked members (64 full chunks: region_chunk_sums' loop ends on its
    boundary, k_region_spectra_fold's unroll by 32 has no remainder); region 2 of 4161 unmasked members
    with every seventh spaxel of its stretch masked (66 chunks, the last of one member: a second trip of
    two partials and 62 padded lanes, a remainder of two); region 3 of one spaxel; region 4 whose
    members are all masked."""
    D, H, W = 7, 96, 96
    fsf = np.outer([0.25, 0.5, 0.25], [0.2, 0.6, 0.2])
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, _, _, init, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=96)
    i = np.arange(H * W)
    labels, mask = np.zeros(H * W, dtype=int), np.ones(H * W)
    labels[:4096] = 1
    mask[(i >= 4096) & (i % 7 == 3)] = 0
    last = 4096 + int(np.flatnonzero(np.cumsum(mask[4096:]) == 4161)[0])
    labels[4096:last + 1] = 2
    labels[last + 1] = 3
    mask[last + 1] = 1
    labels[last + 2:last + 12] = 4
    mask[last + 2:last + 12] = 0
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    case = dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=mask.reshape(H, W), init=init,
                min_b=min_b, max_b=max_b)
    return case, labels.reshape(H, W)


@pytest.mark.parametrize("line", ["single", "doublet"])
def test_regions_of_64_and_66_chunks_fold_past_the_first_trip(line):
    """Parameters set directly, three samples through d3d_post_accumulate: the sizes, the scalars bit
    for bit, the spectra and their Welford moments at the spectra tests' bars."""
    case, labels = wide_field()
    mask = live_mask(case)
    assert np.array_equal(mask, case["mask"])
    K = 4
    maps = random_params(case, np.random.default_rng(12), 3)
    with engine_for(case, line) as eng:
        eng.post_begin(0)
        eng.region_begin(labels, K, capacity=3, spectra=True)
        mean, _ = check_spectra(eng, maps, labels, mask, K, case["D"], RO.gaussian_unit_line(*LINES[line]),
                                "wide %s" % line)
        series, _, _, sizes = eng.region_get()
    assert sizes.tolist() == [4096, 4161, 1, 0]
    assert (labels == 4).sum() == 10 and ((labels == 2) & (mask == 0)).sum() > 600
    np.testing.assert_array_equal(series, RO.series(maps, labels, mask, K, flux_k_of(line)))
    assert (series[:, 3, 0] == 0.).all() and np.isnan(series[:, 3, 1:]).all()
    assert (mean[3] == 0.).all() and (mean[:2].max(axis=1) > 0.).all()


# ---- 4. chain paths -----------------------------------------------------------------------------

BLOCKS =regions.blocks((16, 16), 4)


def watched(case, calls, capacity=10, seed=4321, line="single"):
    with engine_for(case, line, seed=seed, refresh_every=5) as eng:
        eng.post_begin()
        eng.post_schedule(1, 1)
        eng.region_begin(BLOCKS, 16, capacity=capacity)
        state = chain_state(eng, sum(calls), calls=calls)
        return state, eng.region_count(), eng.region_get(), [eng.post_get(w) for w in (0, 1, 2)]


def same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_split_calls_and_the_capacity_and_the_unwatched_chain():
    case = make_case("c1")
    whole_state, whole_n, whole, whole_post = watched(case, [10])
    split_state, split_n, split, _ = watched(case, [1, 9])
    assert whole_n == split_n == (10, 10)
    same(whole, split)                                       # series, spectra, sizes: bit-identical
    same(whole_state, split_state)
    with engine_for(case, seed=4321, refresh_every=5) as eng:       # without regions: the same chain, the same moments
        eng.post_begin()
        eng.post_schedule(1, 1)
        same(chain_state(eng, 10), whole_state)
        for w in (0, 1, 2):
            same(eng.post_get(w), whole_post[w])
    # the series is the oracle's of the moments' samples? (the chain itself is not streamed here:
    # test_run_series_is_the_oracle_of_the_chain checks that); past the capacity the series alone stops
    short_state, short_n, short, short_post = watched(case, [10], capacity=4)
    assert short_n == (10, 4) and short[0].shape == (4, 16, 3)
    np.testing.assert_array_equal(short[0], whole[0][:4])
    same(short[1:], whole[1:])
    same(short_state, whole_state)
    for w in (0, 1, 2):
        same(short_post[w], whole_post[w])


def test_batched_chains_keep_their_own_regions():
    case = make_case("c1")
    R, n_sweeps = 3, 6
    engines = [engine_for(case, "doublet", seed=100 + r, refresh_every=5) for r in range(R)]
    try:
        for eng in engines:
            eng.post_begin(_lib.POST_CLEAN)
            eng.post_schedule(2, 2)
            eng.region_begin(BLOCKS, 16, capacity=3)
        _lib.mh_sweeps_batch(engines, n_sweeps, 1, 1)
        got = [(e.region_count(), e.region_get()) for e in engines]
    finally:
        for eng in engines:
            eng.close()
    for r in range(R):
        with engine_for(case, "doublet", seed=100 + r, refresh_every=5) as eng:
            eng.post_begin(_lib.POST_CLEAN)
            eng.post_schedule(2, 2)
            eng.region_begin(BLOCKS, 16, capacity=3)
            eng.mh_sweeps(n_sweeps, 1, 1)
            assert eng.region_count() == got[r][0] == (3, 3)
            same(eng.region_get(), got[r][1])
    assert not np.array_equal(got[0][1][0], got[1][1][0])


# ---- 5. Run -------------------------------------------------------------------------------------

ODD_IDS = np.where(BLOCKS % 3 == 0, 0, BLOCKS * 10)          # 0 = no region; the ids are 10, 20, 40, ...


def test_run_series_is_the_oracle_of_the_chain(tmp_path):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    B, every = 4, 3
    plain = d3d.Run(cube, inst, posterior_burn_in=B, posterior_every=every, **run_kw(var))
    assert plain.posterior.regions is None
    run = d3d.Run(cube, inst, posterior_burn_in=B, posterior_every=every, regions=ODD_IDS, **run_kw(var))
    np.testing.assert_array_equal(plain.chain, run.chain)            # bit for bit what it was
    same(plain.posterior.moments(1)[1:], run.posterior.moments(1)[1:])
    rp = run.posterior.regions
    ids = np.unique(ODD_IDS[ODD_IDS > 0])
    compact = np.searchsorted(ids, ODD_IDS) * (ODD_IDS > 0) + (ODD_IDS > 0)
    slots = run.chain[B::every]
    assert rp.count == len(slots) == 3 and rp.ids.tolist() == ids.tolist()
    np.testing.assert_array_equal(rp.sizes, [np.sum((ODD_IDS == i) & (run.mask == 1)) for i in ids])
    np.testing.assert_array_equal(rp.series, RO.series(slots, compact, run.mask, len(ids), SQRT_2PI))
    clean = np.mean([run.simulate_clean(cube.data.shape, s) for s in slots], axis=0)
    within(rp.spectrum_mean, region_sums(clean, compact, len(ids)), "spectra against the chain's clean cubes")
    assert rp.spectrum_std.shape == (len(ids), 32) and not np.isnan(rp.spectrum_std).any()
    assert rp.flux_covariance().shape == (len(ids),) * 2 and rp.quantiles([0.5]).shape == (len(ids), 3, 1)
    run.posterior.save(str(tmp_path / "out"))
    saved = np.load(str(tmp_path / "out_posterior_regions.npz"))
    np.testing.assert_array_equal(saved["flux"], rp.flux)
    np.testing.assert_array_equal(saved["ids"], ids)
    bare = d3d.Run(cube, inst, posterior_burn_in=B, regions=dict(labels=ODD_IDS, spectra=False), **run_kw(var))
    assert bare.posterior.regions.spectrum_mean is None and bare.posterior.regions.count == 12 - B


@pytest.mark.parametrize("batched", [True, False])
def test_run_chains_keep_their_own_and_pool(batched):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    B = 5
    many = d3d.Run.__new__(d3d.Run)
    many._batched = batched
    many.__init__(cube, inst, chains=2, posterior_burn_in=B, regions=BLOCKS, **run_kw(var))
    ones = [d3d.Run(cube, inst, posterior_burn_in=B, regions=BLOCKS, **run_kw(var, seed=31 + r)) for r in range(2)]
    for r in range(2):
        np.testing.assert_array_equal(many.posteriors[r].regions.series, ones[r].posterior.regions.series)
        same(many.posteriors[r].regions.spectrum_moments(), ones[r].posterior.regions.spectrum_moments())
    pooled = many.posterior.regions
    assert pooled.count == 2 * (12 - B)
    np.testing.assert_array_equal(pooled.series, np.concatenate([o.posterior.regions.series for o in ones]))
    n, mean, m2 = posterior.pool([o.posterior.regions.spectrum_moments() for o in ones])
    np.testing.assert_array_equal(pooled.spectrum_mean, mean)
    np.testing.assert_array_equal(pooled.spectrum_std, posterior.std_from_m2(n, m2))


def test_run_tempering_follows_rung_0_only():
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    run = d3d.Run(cube, inst, posterior_burn_in=5, regions=BLOCKS, tempering=dict(betas=(1., 0.5), swap_every=2),
                  **run_kw(var))
    assert len(run.posteriors) == 1 and run.posterior.regions.count == 12 - 5
    assert run.engines[1].region_count() == (0, 0)
    np.testing.assert_array_equal(run.posterior.regions.series,
                                  RO.series(run.chain[5:], BLOCKS, run.mask, 16, SQRT_2PI))


def test_refusals_by_status_code_and_exception():
    case = make_case("c1")
    lib = _lib.load()
    dims = (case["D"], case["H"], case["W"])
    lab = np.ascontiguousarray(BLOCKS, dtype=np.int32)
    ptr = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def last():
        return lib.d3d_last_error().decode()

    with _lib.Engine(dims, case["fsf"].shape) as eng:
        ctx = eng._ctx
        n, stored = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.d3d_region_count(ctx, ctypes.byref(n), ctypes.byref(stored)) == 0 and n.value == stored.value == 0
        assert lib.d3d_region_begin(ctx, ptr, 16, 4, 1) == _lib.ERR_STATE and "d3d_post_begin" in last()
        assert lib.d3d_region_get(ctx, None, None, None, None) == _lib.ERR_STATE
        with pytest.raises(RuntimeError):
            eng.region_begin(BLOCKS, capacity=4)
        eng.post_begin(0)
        assert lib.d3d_region_begin(ctx, ptr, 15, 4, 1) == _lib.ERR_INVALID and "labels" in last()   # a label beyond K
        assert lib.d3d_region_begin(ctx, ptr, 0, 4, 1) == _lib.ERR_INVALID and "K" in last()
        assert lib.d3d_region_begin(ctx, ptr, 16, -1, 1) == _lib.ERR_INVALID and "capacity" in last()
        assert lib.d3d_region_begin(ctx, ptr, 16, 4, 2) == _lib.ERR_INVALID and "what" in last()
        assert lib.d3d_region_begin(ctx, None, 16, 4, 1) == _lib.ERR_INVALID
        neg = lab.copy()
        neg[3, 3] = -1
        assert lib.d3d_region_begin(ctx, neg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 16, 4, 1) == _lib.ERR_INVALID
        with pytest.raises(ValueError):
            eng.region_begin(BLOCKS.astype(float), capacity=4)
        with pytest.raises(ValueError):
            eng.region_begin(BLOCKS[:, :8], capacity=4)
        assert lib.d3d_region_count(ctx, ctypes.byref(n), None) == 0 and n.value == 0      # nothing was begun
        eng.region_begin(BLOCKS, capacity=4, spectra=False)
        assert lib.d3d_region_get(ctx, None, None, None, None) == 0
        mean = np.empty((16, dims[0]))
        assert lib.d3d_region_get(ctx, None, _lib._dp(mean), None, None) == _lib.ERR_STATE and "spectra" in last()
        eng.region_end()
        assert lib.d3d_region_get(ctx, None, None, None, None) == _lib.ERR_STATE
        eng.region_end()                                                    # twice is fine
        eng.region_begin(BLOCKS, capacity=4)
        eng.post_end()                                                      # the moments' end frees them
        assert eng.region_count() == (0, 0)
        assert lib.d3d_region_get(ctx, None, None, None, None) == _lib.ERR_STATE
    with _lib.Engine(dims, case["fsf"].shape) as eng:                       # a tile
        eng.set_tile(0, 0, case["W"], 0, case["H"], 0, case["W"])
        assert lib.d3d_region_begin(eng._ctx, ptr, 16, 4, 1) == _lib.ERR_UNSUPPORTED and "tile" in last()
        with pytest.raises(NotImplementedError):
            eng.region_begin(BLOCKS, capacity=4)
    assert lib.d3d_region_begin(None, ptr, 16, 4, 1) == _lib.ERR_INVALID


def test_run_refuses_a_host_evaluated_model():
    class Boxy(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            return parameters[0] * (np.abs(x - parameters[1]) <= parameters[2])

    inst, cube, var, _ = run_inputs(16, 9, 9, [0.], [1.], seed=6)
    with pytest.raises(NotImplementedError, match="regions=.*evaluated on the host"):
        d3d.Run(cube, inst, model=Boxy, posterior_burn_in=2, regions=regions.blocks((9, 9), 3), **run_kw(var))


def test_whatever_resets_the_moments_resets_the_regions():
    case = make_case("c1")
    mask = live_mask(case)
    with engine_for(case) as eng:
        eng.post_begin(0)
        eng.post_schedule(1, 1)
        eng.region_begin(BLOCKS, 16, capacity=8)
        eng.mh_sweeps(3, 1, 1)
        assert eng.region_count() == (3, 3)
        eng.set_line_shape(*LINES["doublet"])
        assert eng.region_count() == (0, 0) and eng.region_get()[0].shape == (0, 16, 3)
        eng.post_accumulate()
        series, mean, m2, _ = eng.region_get()
        np.testing.assert_array_equal(series, RO.series(eng.get_params()[None], BLOCKS, mask, 16, flux_k_of("doublet")))
        assert (m2 == 0.).all() and mean.any()                # nothing of the old model left
        # another mask lays the members out again
        other = np.ones_like(mask)
        other[4:8, 4:8] = 0
        eng.set_data(case["data"], case["var"], mask=other)
        assert eng.region_count() == (0, 0)
        eng.post_accumulate()
        series, _, _, sizes = eng.region_get()
        assert sizes[5] == 0 and sizes.sum() == 256 - 16
        np.testing.assert_array_equal(series, RO.series(eng.get_params()[None], BLOCKS, other, 16, flux_k_of("doublet")))


# ---- 6. science ---------------------------------------------------------------------------------

def test_a_blocks_flux_is_better_determined_than_its_spaxels():
    """c1 under its 9 x 9 FSF, 4 x 4 blocks, started at the truth, 400 sweeps of which the last 300
    are sampled: neighbours trade flux, so the variance of a block's summed flux is smaller than the
    sum of its spaxels' flux variances (what independent spaxels would give).  On the CPU oracle's
    chain of the same case and seed the ratio var(F_block) / sum var(F_i) of the four interior
    blocks is 0.25, 0.52, 0.30, 0.31 (all sixteen: 0.07 to 0.52); asserted with half the room the
    worst leaves, 1 - (1 - 0.515) / 2."""
    case = make_case("c1")
    mask = live_mask(case)
    with engine_for(case, seed=99, refresh_every=0) as eng:
        eng.set_params(case["truth"])
        eng.post_begin(0)
        eng.post_schedule(101, 1)
        eng.region_begin(BLOCKS, 16, capacity=300, spectra=False)
        eng.mh_sweeps(400, 1, 1)
        assert eng.region_count() == (300, 300)
        flux = eng.region_get()[0][..., 0]
        spaxel_var = eng.post_get(0)[1][..., 3] / 299. * (mask == 1)
    ratio = flux.var(axis=0, ddof=1) / np.array([spaxel_var[BLOCKS == k].sum() for k in range(1, 17)])
    print("var(F_block) / sum var(F_i):\n%s" % np.round(ratio.reshape(4, 4), 3))
    interior = ratio.reshape(4, 4)[1:3, 1:3]
    assert (interior < 1. - (1. - 0.515) / 2.).all(), interior
