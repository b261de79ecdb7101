"""
GPU tests of the posterior histograms kept on the device (d3d_hist_*: k_hist_freeze, k_hist_accum,
k_hist_quantiles; Run(posterior_histograms=...)) against the numpy restatement of their contract
(tests/histogram_oracle.py):

  * counters as INTEGERS: samples fed directly (on lo, on hi, beyond both, two modes) and the
    samples of a chain streamed out with keep_one_in = 1, binned by the restatement into the
    device's ranges;
  * ranges against mean +- span sd of the pilot.  Bar: the moments meet MAP_RTOL = 1e-12 of the
    map's peak for the mean and for the standard deviation (tests/test_gpu_posterior.py), so
    mean -+ span sd meets (1 + span) 1e-12; 2e-12 (STD_RTOL) leaves room for the restatement's own
    Welford roundings;
  * quantile, mode and outside maps against the restatement on the downloaded counters.  Bar:
    1e-13 of max(|lo|, |hi|) -- about eight roundings of numbers no larger than that, and equality
    is what is expected;
  * device quantiles against the chain's own inverted-CDF sample quantiles.  Bar: one bin width of
    that spaxel (both lie in the same bin); checks whose q n falls in a tail are left out;
  * identities (the chain does not notice; split calls; batched chains), life cycle, refusals, Run.
"""
import ctypes

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior
from tests import histogram_oracle as HO
from tests.cases import make_case
from tests.test_gpu_multiplet import run_inputs
from tests.test_gpu_posterior import LINES, chain_state, engine_for

pytestmark = pytest.mark.gpu

RANGE_RTOL = 2e-12          # times (1 + span), of the quantity's peak
EXTRACT_RTOL = 1e-13        # of max(|lo|, |hi|)
QS = (0.01, 0.16, 0.25, 0.5, 0.75, 0.84, 0.99, 0.999)
FIRST, PILOT, N_HIST, SPAN = 3, 24, 37, 6.0


def flux_k(line):
    return HO.flux_factor(LINES[line][1])


def live_mask(case):
    mask = np.array(case["mask"], dtype=np.float64)
    mask[np.isnan(case["data"]).any(axis=0)] = 0
    return mask


def check_ranges(rng, samples, pilot, span, case, line, what):
    """The device's ranges against the restatement's from the pilot's samples (n, H, W, 4)."""
    L, U = HO.bounds(case["min_b"], case["max_b"], flux_k(line))
    mask = live_mask(case)
    lo, hi = HO.freeze(*HO.welford(samples[:pilot]), pilot, span, L, U, mask)
    dead = mask != 1
    assert np.isnan(rng[dead]).all() and not np.isnan(rng[~dead]).any()
    worst = 0.
    for k, label in enumerate(("a", "c", "w", "F")):
        peak = float(np.max(np.abs(samples[:pilot, ..., k])))
        bar = (1. + span) * RANGE_RTOL * peak
        err = max(float(np.nanmax(np.abs(rng[..., k, 0] - lo[..., k]))), float(np.nanmax(np.abs(rng[..., k, 1] - hi[..., k]))))
        print("%s range of %s: max|d| = %.3g (bar %.3g, peak %.3g)" % (what, label, err, bar, peak))
        assert err <= bar, "%s range of %s: %g vs %g" % (what, label, err, bar)
        worst = max(worst, err / max(peak, 1e-300))
    assert (rng[~dead][..., 1] > rng[~dead][..., 0]).all()
    return worst


def check_extraction(eng, bins, tails, rng, what):
    """Quantile, mode and outside maps of the device against the restatement on the same counters."""
    quant, mode, outside = eng.hist_quantiles(QS)
    scale = np.maximum(np.abs(rng[..., 0]), np.abs(rng[..., 1]))
    worst = 0.
    for j, q in enumerate(QS):
        want = HO.quantile(bins, tails, rng, q)
        np.testing.assert_array_equal(np.isnan(quant[..., j]), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            rel = np.abs(quant[..., j] - want)[ok] / np.maximum(scale[ok], 1e-300)
            worst = max(worst, float(rel.max()))
    want = HO.mode(bins, tails, rng)
    np.testing.assert_array_equal(np.isnan(mode), np.isnan(want))
    ok = ~np.isnan(want)
    worst_mode = float((np.abs(mode - want)[ok] / np.maximum(scale[ok], 1e-300)).max()) if ok.any() else 0.
    want = HO.outside(bins, tails, rng)
    np.testing.assert_array_equal(np.isnan(outside), np.isnan(want))
    ok = ~np.isnan(want)
    worst_out = float(np.abs(outside - want)[ok].max()) if ok.any() else 0.
    print("%s: worst quantile %.3g, mode %.3g of max(|lo|,|hi|), outside %.3g (bar %.1g)"
          % (what, worst, worst_mode, worst_out, EXTRACT_RTOL))
    assert worst <= EXTRACT_RTOL and worst_mode <= EXTRACT_RTOL and worst_out <= EXTRACT_RTOL, what
    return quant, mode, outside


# ---- 1. samples fed directly ----------------------------------------------------------------

@pytest.mark.parametrize("name,line", [("tiny", "single"), ("d30", "doublet")])      # 1 x 3 and 9 x 11 spaxels
def test_fed_samples_land_in_the_restatements_counters(name, line):
    case = make_case(name)
    H, W = case["H"], case["W"]
    pilot, span = 8, 2.0
    rng_ = np.random.default_rng(3)
    base = case["truth"].copy()
    spread = np.array([0.3, 0.05, 0.1])
    fed = [base + spread * rng_.normal(size=(H, W, 3)) for _ in range(pilot)]
    with engine_for(case, line) as eng:
        eng.post_begin(0)
        eng.hist_begin(pilot, span)
        assert eng.hist_count() == 0
        for p in fed[:-1]:
            eng.set_params(p)
            eng.post_accumulate()
        assert np.isnan(eng.hist_get()[2]).all()                 # not frozen before sample number `pilot`
        eng.set_params(fed[-1])
        eng.post_accumulate()
        assert eng.hist_count() == 0 and eng.post_count() == pilot
        bins, tails, rng = eng.hist_get()
        assert bins.sum() == 0 and tails.sum() == 0
        check_ranges(rng, HO.series(np.stack(fed), flux_k(line)), pilot, span, case, line, name)
        lo = np.where(np.isnan(rng[..., :3, 0]), base, rng[..., :3, 0])      # masked spaxels: any finite value
        hi = np.where(np.isnan(rng[..., :3, 1]), base, rng[..., :3, 1])
        ext = hi - lo
        later = [lo.copy(), hi.copy(), lo - 0.1 * ext, hi + 0.3 * ext, np.nextafter(hi, -np.inf),
                 np.nextafter(lo, -np.inf)]
        later += [lo + (0.2 + 0.01 * j) * ext for j in range(5)]                   # two separated modes
        later += [lo + (0.8 + 0.005 * j) * ext for j in range(3)]
        later += [lo + ext * rng_.random((H, W, 3)) for _ in range(4)]
        for p in later:
            eng.set_params(p)
            eng.post_accumulate()
        assert eng.hist_count() == len(later) and eng.post_count() == pilot + len(later)
        bins, tails, rng2 = eng.hist_get()
        np.testing.assert_array_equal(rng2, rng)                  # frozen once
        want_bins, want_tails = HO.count(HO.series(np.stack(later), flux_k(line)), rng[..., 0], rng[..., 1])
        np.testing.assert_array_equal(bins, want_bins)
        np.testing.assert_array_equal(tails, want_tails)
        live = live_mask(case) == 1
        total = bins.sum(axis=-1, dtype=np.int64) + tails.sum(axis=-1, dtype=np.int64)
        assert (total[live] == len(later)).all() and (total[~live] == 0).all()
        acw = bins[live][:, :3]
        assert (acw[..., 0] >= 1).all()                           # a sample on lo is in bin 0 ...
        assert (tails[live][:, :3, 0] == 2).all()                 # ... the two beneath it below
        assert (tails[live][:, :3, 1] >= 1).all()                 # (a sample on hi: above, or bin 63 when
        assert ((tails[live][:, :3, 1] + acw[..., 63]) >= 3).all()  # (hi - lo) * (64 / (hi - lo)) rounds below 64)
        assert (acw[..., 12:16].sum(axis=-1) >= 5).all() and (acw[..., 51:54].sum(axis=-1) >= 3).all()
        assert (acw[..., 20:45].sum(axis=-1) <= 4).all()          # the gap between the modes: the uniform draws only
        check_extraction(eng, bins, tails, rng, name)


# ---- 2. - 4. a chain ------------------------------------------------------------------------

CHAINS = {"d30": ("d30", "single", 1, "init"), "c1": ("c1", "doublet", 3, "init"),
          "odd_depth": ("odd_depth", "doublet", 1, "init"),
          # started at the truth (the quantile comparison: a chain that has arrived)
          "d30_truth": ("d30", "single", 1, "truth"), "c1_truth": ("c1", "single", 1, "truth")}
_runs = {}


def chain_run(key):
    """The chain of CHAINS[key] with histograms on, once a session: everything downloaded."""
    if key not in _runs:
        name, line, every, start = CHAINS[key]
        case = dict(make_case(name))
        case["init"] = case[start]
        n_sweeps = FIRST + (PILOT + N_HIST - 1) * every
        with engine_for(case, line) as eng:
            eng.post_begin()
            eng.post_schedule(FIRST, every)
            eng.hist_begin(PILOT, SPAN)
            chain = np.full((n_sweeps + 1, case["H"], case["W"], 3), np.nan)
            eng.mh_sweeps(n_sweeps, 1, 1, chain)
            slots = list(range(FIRST, n_sweeps + 1, every))
            assert eng.post_count() == len(slots) == PILOT + N_HIST and eng.hist_count() == N_HIST
            bins, tails, rng = eng.hist_get()
            extracted = check_extraction(eng, bins, tails, rng, key)
        _runs[key] = dict(case=case, line=line, samples=HO.series(chain[slots], flux_k(line)), bins=bins,
                          tails=tails, rng=rng, extracted=extracted)
    return _runs[key]


@pytest.mark.parametrize("key", ["d30", "c1", "odd_depth"])
def test_chain_samples_land_in_the_restatements_counters(key):
    r = chain_run(key)
    check_ranges(r["rng"], r["samples"], PILOT, SPAN, r["case"], r["line"], key)
    want_bins, want_tails = HO.count(r["samples"][PILOT:], r["rng"][..., 0], r["rng"][..., 1])
    np.testing.assert_array_equal(r["bins"], want_bins)
    np.testing.assert_array_equal(r["tails"], want_tails)
    dead = live_mask(r["case"]) != 1
    assert dead.sum() == 3
    assert (r["bins"][dead] == 0).all() and (r["tails"][dead] == 0).all() and np.isnan(r["rng"][dead]).all()
    total = r["bins"].sum(axis=-1, dtype=np.int64) + r["tails"].sum(axis=-1, dtype=np.int64)
    assert (total[~dead] == N_HIST).all()
    quant, mode, outside = r["extracted"]
    assert np.isnan(quant[dead]).all() and np.isnan(mode[dead]).all() and np.isnan(outside[dead]).all()
    assert not np.isnan(quant[~dead]).any() and not np.isnan(outside[~dead]).any()


@pytest.mark.parametrize("key", ["d30_truth", "c1_truth"])
def test_device_quantiles_lie_within_a_bin_of_the_chains_sample_quantiles(key):
    """Left out (q n in a tail) and worst difference in bins are printed; at most 10 % may be left out."""
    r = chain_run(key)
    live = live_mask(r["case"]) == 1
    later = r["samples"][PILOT:]
    quant = r["extracted"][0]
    below, above = r["tails"][..., 0].astype(np.int64), r["tails"][..., 1].astype(np.int64)
    width = (r["rng"][..., 1] - r["rng"][..., 0]) / 64.
    checks = left_out = 0
    worst = 0.
    for q in (0.16, 0.5, 0.84):
        t = q * N_HIST
        assert t != np.floor(t)
        want = np.quantile(later, q, axis=0, method="inverted_cdf")
        inside = live[..., None] & (t > below) & (t <= N_HIST - above)
        checks += int(live.sum()) * 4
        left_out += int((live[..., None] & ~inside).sum())
        diff = np.abs(quant[..., QS.index(q)] - want)[inside] / width[inside]
        worst = max(worst, float(diff.max()))
    print("%s: %d of %d checks left out (q n in a tail); worst difference %.3f of a bin" % (key, left_out, checks, worst))
    assert worst <= 1.0
    assert left_out <= 0.1 * checks


# ---- 5. identities --------------------------------------------------------------------------

def hist_state(eng):
    return (eng.hist_count(),) + eng.hist_get() + eng.post_get(0)


def same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def test_the_chain_does_not_notice_the_histograms():
    case = make_case("c1")
    n_sweeps = 30
    with engine_for(case, refresh_every=7) as eng:
        plain = chain_state(eng, n_sweeps)
    with engine_for(case, refresh_every=7) as eng:
        eng.post_begin()
        eng.post_schedule(2, 1)
        moments_only = chain_state(eng, n_sweeps)
        map_moments = eng.post_get(0)
    with engine_for(case, refresh_every=7) as eng:
        eng.post_begin()
        eng.post_schedule(2, 1)
        eng.hist_begin(5, 4.0)
        watched = chain_state(eng, n_sweeps)
        assert eng.hist_count() == n_sweeps - 1 - 5
        assert eng.hist_get()[0].sum() > 0
        for a, b in zip(map_moments, eng.post_get(0)):            # nor do the moments
            np.testing.assert_array_equal(a, b)
    for other in (moments_only, watched):
        for a, b, what in zip(plain, other, ("parameters", "carried residual", "log ratios", "accepted")):
            np.testing.assert_array_equal(a, b, err_msg=what)
    assert plain[3] > 0


@pytest.mark.parametrize("calls", [[13, 27], [4, 36], [1] * 40])
def test_split_calls_give_the_same_histograms(calls):
    case = make_case("d30")

    def run(split):
        with engine_for(case, "doublet", refresh_every=6) as eng:
            eng.post_begin(0)
            eng.post_schedule(3, 2)
            eng.hist_begin(6, 5.0)
            chain_state(eng, 40, calls=split)
            return hist_state(eng)

    whole = run([40])
    assert whole[0] == len(range(3, 41, 2)) - 6
    same(whole, run(calls))


def test_batched_chains_keep_the_histograms_of_their_single_runs():
    case = make_case("c1")
    R, n_sweeps = 2, 36

    def begin(eng):
        eng.post_begin(_lib.POST_CONVOLVED)
        eng.post_schedule(4, 1)
        eng.hist_begin(9, 6.0)

    engines = [engine_for(case, "doublet", seed=700 + r, refresh_every=5) for r in range(R)]
    try:
        for eng in engines:
            begin(eng)
        _lib.mh_sweeps_batch(engines, n_sweeps, 1, 1)
        batched = [hist_state(eng) + eng.hist_quantiles(QS) for eng in engines]
    finally:
        for eng in engines:
            eng.close()
    assert not np.array_equal(batched[0][1], batched[1][1])
    for r in range(R):
        with engine_for(case, "doublet", seed=700 + r, refresh_every=5) as eng:
            begin(eng)
            eng.mh_sweeps(n_sweeps, 1, 1)
            assert eng.hist_count() == n_sweeps - 3 - 9
            same(batched[r], hist_state(eng) + eng.hist_quantiles(QS))


# ---- 6. life cycle --------------------------------------------------------------------------

def test_life_cycle():
    case = make_case("d30")
    with engine_for(case) as eng:
        eng.post_begin(0)
        eng.post_schedule(1, 1)
        eng.hist_begin(4, 6.0)
        eng.mh_sweeps(3, 1, 1)
        # before the pilot has passed: nothing counted, nothing frozen, every output NaN
        assert eng.post_count() == 3 and eng.hist_count() == 0
        bins, tails, rng = eng.hist_get()
        assert bins.shape == (9, 11, 4, 64) and tails.shape == (9, 11, 4, 2) and rng.shape == (9, 11, 4, 2)
        assert bins.dtype == np.uint32 and bins.sum() == 0 and tails.sum() == 0 and np.isnan(rng).all()
        for out in eng.hist_quantiles([0.5, 0.9]):
            assert np.isnan(out).all()
        assert eng.hist_quantiles([0.5, 0.9])[0].shape == (9, 11, 4, 2)
        eng.mh_sweeps(1, 4, 1)                                   # sample number `pilot`: frozen, not counted
        assert eng.hist_count() == 0 and not np.isnan(eng.hist_get()[2]).all() and eng.hist_get()[0].sum() == 0
        assert np.isnan(eng.hist_quantiles([0.5])[0]).all()
        eng.mh_sweeps(6, 5, 1)
        assert eng.hist_count() == 6
        live = live_mask(case) == 1
        bins, tails, rng = eng.hist_get()
        assert ((bins.sum(axis=-1, dtype=np.int64) + tails.sum(axis=-1, dtype=np.int64))[live] == 6).all()
        ph = posterior.PosteriorHistograms.from_engine(eng)
        assert ph.count == 6 and not np.isnan(ph.median[live]).any() and np.isnan(ph.median[~live]).all()
        # set_data: counts zero, ranges unfrozen -- and the next pilot freezes new ones
        eng.set_data(case["data"], case["var"], mask=case["mask"])
        assert eng.post_count() == 0 and eng.hist_count() == 0
        bins2, tails2, rng2 = eng.hist_get()
        assert bins2.sum() == 0 and tails2.sum() == 0 and np.isnan(rng2).all()
        eng.residual(fetch=False)
        eng.mh_sweeps(9, 11, 1)
        assert eng.post_count() == 9 and eng.hist_count() == 5
        rng3 = eng.hist_get()[2]
        assert not np.isnan(rng3[live]).any() and not np.array_equal(rng3[live], rng[live])
        # hist_end frees the counters, the moments go on; post_end frees both
        eng.hist_end()
        assert eng.hist_count() == 0 and eng.post_count() == 9
        with pytest.raises(RuntimeError):
            eng.hist_get()
        eng.mh_sweeps(1, 20, 1)
        assert eng.post_count() == 10
        eng.hist_begin(2, 1.0)                                    # begun again: the moments start afresh
        assert eng.post_count() == 0
        eng.post_end()
        assert eng.hist_count() == 0
        with pytest.raises(RuntimeError):
            eng.hist_get()
        with pytest.raises(RuntimeError):
            eng.hist_quantiles([0.5])
        eng.hist_end()                                            # twice is fine
        eng.mh_sweeps(2, 21, 1)                                   # and the chain goes on


# ---- 7. refusals ----------------------------------------------------------------------------

def test_refusals_by_status_code_and_exception():
    case = make_case("c1")
    lib = _lib.load()
    dims = (case["D"], case["H"], case["W"])

    def last():
        return lib.d3d_last_error().decode()

    with _lib.Engine(dims, case["fsf"].shape) as eng:
        ctx = eng._ctx
        n = ctypes.c_int64(-1)
        assert lib.d3d_hist_count(ctx, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.d3d_hist_begin(ctx, 10, 6.0) == _lib.ERR_STATE and "d3d_post_begin" in last()
        with pytest.raises(RuntimeError):
            eng.hist_begin()
        eng.post_begin(0)
        assert lib.d3d_hist_begin(ctx, 10, 6.0) == _lib.ERR_STATE and "d3d_mh_config" in last()
        with pytest.raises(RuntimeError):
            eng.hist_begin()
        assert lib.d3d_hist_get(ctx, None, None, None) == _lib.ERR_STATE
        q = (ctypes.c_double * 2)(0.5, 0.9)
        assert lib.d3d_hist_quantiles(ctx, 2, q, None, None, None) == _lib.ERR_STATE
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 1.0)
        for pilot in (1, 0, -5):
            assert lib.d3d_hist_begin(ctx, pilot, 6.0) == _lib.ERR_INVALID and "pilot" in last()
            with pytest.raises(ValueError):
                eng.hist_begin(pilot, 6.0)
        for span in (0., -1., float("inf"), float("nan")):
            assert lib.d3d_hist_begin(ctx, 10, span) == _lib.ERR_INVALID and "span" in last()
            with pytest.raises(ValueError):
                eng.hist_begin(10, span)
        assert eng.hist_count() == 0
        eng.hist_begin(2, 6.0)
        assert lib.d3d_hist_get(ctx, None, None, None) == 0
        assert lib.d3d_hist_quantiles(ctx, 2, q, None, None, None) == 0
        for n_q in (0, -1, 9):
            assert lib.d3d_hist_quantiles(ctx, n_q, q, None, None, None) == _lib.ERR_INVALID and "n_q" in last()
        with pytest.raises(ValueError):
            eng.hist_quantiles([])
        with pytest.raises(ValueError):
            eng.hist_quantiles(np.linspace(0.1, 0.9, 9))
        for bad in (0., 1., -0.5, 1.5, float("nan")):
            with pytest.raises(ValueError):
                eng.hist_quantiles([0.5, bad])
        assert lib.d3d_hist_quantiles(ctx, 2, None, None, None, None) == _lib.ERR_INVALID
        assert eng.hist_quantiles(np.linspace(0.1, 0.9, 8))[0].shape == (16, 16, 4, 8)
    assert lib.d3d_hist_begin(None, 10, 6.0) == _lib.ERR_INVALID
    assert lib.d3d_hist_end(None) == _lib.ERR_INVALID


# ---- 8. Run ---------------------------------------------------------------------------------

def run_kw(var, **more):
    kw = dict(variance=var, max_iterations=70, seed=31, min_acceptance_rate=0.)
    kw.update(more)
    return kw


def test_run_keeps_histograms_beside_the_moments(tmp_path):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    with pytest.raises(ValueError, match="posterior_burn_in"):
        d3d.Run(cube, inst, posterior_histograms=True, **run_kw(var))
    mask = np.ones((16, 16))
    mask[2, 3] = mask[11, 7] = 0
    B, pilot = 8, 24
    plain = d3d.Run(cube, inst, mask=mask, posterior_burn_in=B, **run_kw(var))
    assert plain.posterior.histograms is None
    run = d3d.Run(cube, inst, mask=mask, posterior_burn_in=B, posterior_histograms=dict(pilot=pilot),
                  **run_kw(var))
    np.testing.assert_array_equal(plain.chain, run.chain)
    for a, b in zip(plain.posterior.moments(0)[1:], run.posterior.moments(0)[1:]):
        np.testing.assert_array_equal(a, b)
    ph = run.posterior.histograms
    assert isinstance(ph, d3d.PosteriorHistograms) and (ph.pilot, ph.span) == (pilot, 6.0)
    assert run.posterior.count == 70 - B and ph.count == run.posterior.count - pilot
    live = mask == 1
    med, (lo68, hi68) = ph.median, ph.interval(0.68)
    lo, hi = ph.range[..., 0], ph.range[..., 1]
    for arr in (med, lo68, hi68, ph.outside, lo, hi):
        assert arr.shape == (16, 16, 4) and np.isnan(arr[~live]).all() and not np.isnan(arr[live]).any()
    # (this short chain is still drifting after its pilot: a series may have every sample in a tail, and then no mode)
    np.testing.assert_array_equal(np.isnan(ph.mode), ph.counts.sum(axis=-1) == 0)
    assert np.isnan(ph.mode[~live]).all() and not np.isnan(ph.mode[live]).all()
    inside = ~np.isnan(ph.mode)
    assert (ph.mode[inside] > lo[inside]).all() and (ph.mode[inside] < hi[inside]).all()
    assert (lo[live] <= med[live]).all() and (med[live] <= hi[live]).all()
    L, U = HO.bounds(run.min_boundaries, run.max_boundaries, HO.flux_factor([1.]))
    assert (med[live] >= L).all() and (med[live] <= U).all()
    assert (lo68[live] <= med[live]).all() and (med[live] <= hi68[live]).all()
    assert (ph.outside[live] >= 0.).all() and (ph.outside[live] <= 1.).all()
    assert (ph.counts[~live] == 0).all()
    # the counters are those of the chain's own samples in the device's ranges
    want_bins, want_tails = HO.count(HO.series(run.chain[B + pilot:], HO.flux_factor([1.])), lo, hi)
    np.testing.assert_array_equal(ph.counts, want_bins)
    np.testing.assert_array_equal(ph.tails, want_tails)
    ph.save(str(tmp_path / "run"))
    assert int(np.load(str(tmp_path / "run") + "_posterior_histograms.npz")["count"]) == ph.count


def test_run_chains_keep_their_own_and_a_short_run_is_warned(caplog):
    inst, cube, var, _ = run_inputs(32, 16, 16, [0.], [1.], seed=6)
    with caplog.at_level("INFO", logger="deconv3d"):
        many = d3d.Run(cube, inst, chains=2, posterior_burn_in=5, posterior_histograms=dict(pilot=10, span=5.),
                       **run_kw(var, max_iterations=40))
    assert many.posterior.histograms is None
    assert len([r for r in caplog.records if "posterior_histograms" in r.getMessage() and "pooled" in r.getMessage()]) == 1
    for r in range(2):
        one = d3d.Run(cube, inst, posterior_burn_in=5, posterior_histograms=dict(pilot=10, span=5.),
                      **run_kw(var, max_iterations=40, seed=31 + r))
        a, b = many.posteriors[r].histograms, one.posterior.histograms
        assert a.count == b.count == 40 - 5 - 10
        np.testing.assert_array_equal(a.counts, b.counts)
        np.testing.assert_array_equal(a.range, b.range)
        np.testing.assert_array_equal(a.median, b.median)
    caplog.clear()
    with caplog.at_level("WARNING", logger="deconv3d"):
        short = d3d.Run(cube, inst, posterior_burn_in=5, posterior_histograms=True, **run_kw(var, max_iterations=12))
    assert len([r for r in caplog.records if "posterior_histograms" in r.getMessage()]) == 1
    assert short.posterior.histograms.count == 0 and np.isnan(short.posterior.histograms.median).all()
