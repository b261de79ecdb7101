"""
The end of a sweep with everything armed (csrc/d3d_sweep.hip: end_sweep; DESIGN.md, "The order at the
end of a sweep"), through the C ABI, against tests/composed_oracle.py.

Two feature sets, because the noise scales refuse the robust weights and the predictive accuracy:

  R  prior, adaptation, robust weights, moments of both cubes, histograms, regions with spectra,
     predictive accuracy, a refresh every third sweep, the streamed chain and log ratios;
  N  the same with the noise scales (groups of four channels, a spaxel map with holes) in the place of
     the robust weights, and no predictive accuracy.

1. STEPWISE.  Before sweep s everything the context carries is downloaded -- accumulators included --
   and the oracle is made from it; then one sweep on both.  Every comparison is one step from the
   device's own state, at the bar of the feature's own test file: parameters and log ratios 1e-9, the
   residual 1e-11 of its peak, accepted counts equal, Q_g and N_g bit for bit, tau, weights and the
   rewritten 1/variance rtol 1e-12, region scalars bit for bit, histogram counters equal, the moments,
   spectra, ranges, jump scales and predictive accumulators at test_gpu_posterior's, test_gpu_regions',
   test_gpu_histograms', test_gpu_adapt's and test_gpu_predictive's.

   Before every step the carried residual gets a known offset of 1e-3 of its peak (uploaded; the oracle
   is made from the same cube).  A carried and a from-scratch residual otherwise differ by the rounding
   of a few sweeps, which no bar above resolves; with the offset, a draw taken before the refresh or a
   predictive sample taken after it is wrong by 1e-3, not by 1e-15.

   The quantities compared bit for bit take the device's own downloaded arrays where the oracle's are
   equal only to rounding: the samples the parameters after the step (the end of a sweep does not change
   them), the draw the residual after the step.  The predictive sample reads the residual BEFORE the
   refresh, which a refresh sweep leaves nowhere to download: there the oracle's own carried residual
   stands in (one sweep from the device's, equal to 1e-11 of its peak), at the same bar.

2. ONE CALL of N sweeps is N calls of one, with everything downloaded between them, bit for bit.
3. BATCHED: two contexts in d3d_mh_sweeps_batch are the two single contexts bit for bit.

(The oracle is made afresh from the device's state at every step, so no oracle run is shared between
tests: the host's share is the updates of the sweeps themselves, at most 14 277 in a test: three sweeps of
4759 spaxels.)
"""
import numpy as np
import pytest

from deconv3d_amd import _lib, posterior, regions
from oracle import deconv3d_oracle as O
from tests import composed_oracle as CO
from tests import noise_oracle as NO
from tests.test_gpu_histograms import RANGE_RTOL
from tests.test_gpu_mh_dispatch import LAM, problem as dispatch_problem
from tests.test_gpu_posterior import MAP_RTOL, MEAN_RTOL, STD_RTOL

pytestmark = pytest.mark.gpu

OFFSET = 1e-3               # of the carried residual's peak
PRED_RTOL = 1e-10           # tests/test_gpu_predictive.py, the Student-t marginal: rtol, and atol of the largest |q|


# ---- the problems ------------------------------------------------------------------------------------

def small_case():
    """NaN voxels, a whole NaN spectrum, zero variances, an odd depth, 5 x 5 taps."""
    return dict(NO.shape_case((21, 30, 24)), ra=35.0, block=5,
                spec=dict(window=2, last=4, every=2, sweeps=6))


def fill_case():
    """tests/test_gpu_mh_dispatch.py's chip-filling problem: k_mh_ws in two chained strips."""
    p = dispatch_problem("fill", 16, False)
    D, H, W = p["dims"]
    return dict(D=D, H=H, W=W, fsf=p["fsf"], lsf=p["lsf"], data=p["data"], var=p["var"], mask=p["mask"],
                init=p["init"], min_b=p["mn"], max_b=p["mx"], ra=p["ra"], block=23,
                spec=dict(window=1, last=2, every=1, sweeps=3))


def batch_case(geom):
    p = dispatch_problem(geom, 16, False)
    D, H, W = p["dims"]
    return dict(D=D, H=H, W=W, fsf=p["fsf"], lsf=p["lsf"], data=p["data"], var=p["var"], mask=p["mask"],
                init=p["init"], min_b=p["mn"], max_b=p["mx"], ra=p["ra"], block=H // 3,
                spec=dict(window=2, last=4, every=2, sweeps=6))


def zb_case():
    """514 channels on the 5 x 6 field of tests/test_gpu_adapt.py:
    test_fixed_scale_map_on_every_default_kernel_family: the z-blocked kernels, k_mh_zdecide decides."""
    D, H, W = 514, 5, 6
    fsf = O.gaussian_fsf_image(1.6)
    lsf = O.muse_like_lsf(D)
    rng = np.random.default_rng(D)
    truth = np.dstack((1 + 5 * rng.random((H, W)), D * (0.3 + 0.4 * rng.random((H, W))), 1.0 + 2 * rng.random((H, W))))
    mask = np.ones((H, W))
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    sigma = 0.05 * clean.max()
    data = clean + rng.normal(0, sigma, clean.shape)
    var = np.full(clean.shape, sigma ** 2)
    min_b = O.model_min_boundaries()
    max_b = O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.5)
    return dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, init=init, min_b=min_b, max_b=max_b,
                ra=float(max_b[0] ** 2), block=3, spec=dict(window=2, last=4, every=2, sweeps=6))


CASES = {"small": small_case, "fill": fill_case, "zb": zb_case, "b48": lambda: batch_case("b48"),
         "few": lambda: batch_case("few")}
# what the dispatcher must have launched (mh_path_fields), where the problem was chosen for it
PATHS = {"fill": dict(family="ws", NS=256, U=2, M=2, K=2, NTV=False, UV=False, prior=True, multi=False),
         "zb": dict(family="zb"), "b48": dict(family="batch ws"), "few": dict(family="batch small")}


def features(case, which):
    """Set R or N on a case, with the case's schedule (spec)."""
    D, H, W = case["D"], case["H"], case["W"]
    spec = case["spec"]
    labels = regions.blocks((H, W), case["block"]).astype(int)
    ft = dict(lam=LAM, adapt=dict(target=0.25, window=spec["window"], last=spec["last"], gain=2.0, range=(1e-3, 1e3)),
              post=dict(first=1, every=1, cubes=True), hist=dict(pilot=2, span=4.0),
              regions=dict(labels=labels, K=int(labels.max()), spectra=True), refresh_every=3)
    if which == "R":
        ft.update(robust=dict(nu=4, every=spec["every"], start=1, accumulate_from=2), pred=True)
    else:
        ft.update(noise=dict(group=np.arange(D) // 4, every=spec["every"], start=1, shape=1., rate=1.,
                             spaxels=NO.holes(H, W)))
    return CO.features_of(**ft)


def armed_engine(case, ft, seed=77):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape)
    try:
        eng.set_taps(case["fsf"], case["lsf"])
        eng.set_data(case["data"], case["var"], mask=case["mask"])
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, case["ra"], seed=seed, refresh_every=ft["refresh_every"])
        eng.prior_begin(ft["lam"])
        a = ft["adapt"]
        eng.adapt_begin(a["target"], a["window"], a["last"], a["gain"], a["range"])
        if ft["robust"]:
            eng.robust_begin(**ft["robust"])
        else:
            n = ft["noise"]
            eng.noise_begin(n["group"], int(n["group"].max()) + 1, n["spaxels"], shape=n["shape"], rate=n["rate"],
                            every=n["every"], start=n["start"], capacity=8)
        eng.post_begin()
        eng.hist_begin(ft["hist"]["pilot"], ft["hist"]["span"])
        r = ft["regions"]
        eng.region_begin(r["labels"], r["K"], capacity=8, spectra=True)
        if ft["pred"]:
            eng.pred_begin()
        eng.post_schedule(ft["post"]["first"], ft["post"]["every"])
    except Exception:
        eng.close()
        raise
    return eng


def download(eng, ft):
    """Everything the context carries between two sweeps, as composed_oracle's state; and what is only
    compared (`rows`, `weights`, `noise`)."""
    scale, acc, n_win, k = eng.adapt_get()
    bins, tails, rng = eng.hist_get()
    series, spec_mean, spec_m2, sizes = eng.region_get()
    out = dict(params=eng.get_params(), err=eng.download_slot(_lib.SLOT_ERR), ivar=eng.download_slot(_lib.SLOT_IVAR),
               scale=scale, acc=acc.astype(np.int64), n_win=n_win, k=k,
               post=dict(n=eng.post_count(), map=eng.post_get(0), clean=eng.post_get(1), conv=eng.post_get(2)),
               hist=dict(bins=bins, tails=tails, range=rng), regions=dict(spec=(spec_mean, spec_m2)),
               rows=series, sizes=sizes, dlog=eng.get_dlog())
    assert eng.region_count() == (out["post"]["n"], out["post"]["n"]) and eng.hist_count() == max(out["post"]["n"] - 2, 0)
    if ft["pred"]:
        out["pred"] = eng.pred_get()
        assert eng.pred_count() == out["post"]["n"]
    if ft["robust"]:
        weights, mean, count = eng.robust_get()
        out["robust"] = dict(mean=mean, count=count)
        out["weights"] = weights
    else:
        scales, sweeps, voxels, sums, tau = eng.noise_get()
        group = ft["noise"]["group"]
        out["noise"] = dict(scale=scales, sweeps=sweeps, voxels=voxels, sums=sums, tau=tau)
        out["tau_g"] = np.array([tau[group == g][0] for g in range(int(group.max()) + 1)])
    return out


def flat(state):
    """name -> array, of everything in a downloaded state (for bit-for-bit comparisons)."""
    out = {}
    for k, v in state.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                if isinstance(vv, tuple):
                    for j, a in enumerate(vv):
                        out["%s.%s.%d" % (k, kk, j)] = np.asarray(a)
                else:
                    out["%s.%s" % (k, kk)] = np.asarray(vv)
        elif isinstance(v, tuple):
            for j, a in enumerate(v):
                out["%s.%d" % (k, j)] = np.asarray(a)
        else:
            out[k] = np.asarray(v)
    return out


def same_bits(a, b, what):
    fa, fb = flat(a), flat(b)
    assert sorted(fa) == sorted(fb)
    for k in sorted(fa):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg="%s: %s" % (what, k))


def check_path(eng, name):
    """After a call that swept: the family the problem was made for (the read clears the record)."""
    want = PATHS.get(name)
    if want is None:
        return
    got = _lib.mh_path_fields(eng.get_option("mh_path"))
    print(name, got)
    for k, v in want.items():
        assert got[k] == v, "%s: mh_path %s is %r, not %r" % (name, k, got[k], v)
    if name == "fill":
        assert eng.get_option("mh_strips_on") == 2 and eng.get_option("mh_strip_order_on") == 2


# ---- 1. stepwise against the oracle ---------------------------------------------------------------

def within_peak(got, want, rtol, what):
    peak = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(got - want)))
    print("%s: max|d| = %.3g = %.3g of the peak %.3g (bar %.1g)" % (what, err, err / peak, peak, rtol))
    assert err <= rtol * peak, "%s: max|d| = %g vs %g * %g" % (what, err, rtol, peak)


def moments_close(n, got, want, rt_mean, rt_std, what):
    """(mean, M2) as tests/test_gpu_posterior.py compares them: of the peak of the quantity."""
    peak = max(float(np.max(np.abs(want[0]))), 1e-300)
    err = float(np.max(np.abs(got[0] - want[0])))
    print("%s mean: max|d| = %.3g (%.3g of the peak)" % (what, err, err / peak))
    assert err <= rt_mean * peak, "%s mean: %g vs peak %g" % (what, err, peak)
    if n >= 2:
        err = float(np.max(np.abs(posterior.std_from_m2(n, got[1]) - posterior.std_from_m2(n, want[1]))))
        print("%s std: max|d| = %.3g (%.3g of the peak)" % (what, err, err / peak))
        assert err <= rt_std * peak, "%s std: %g vs peak %g" % (what, err, peak)
    else:
        assert (got[1] == 0.).all()


def compare_step(s, pb, ft, co, before, after, chain, dlog, accepted, want_err, tag):
    """The context after its step (`after`; before it: `before`) against the oracle after the same step."""
    live = pb["mask"] == 1
    counted = pb["i0"] != 0.
    refresh, draw, sampled = co.refresh_due(s), co.rescale_due(s), co.post_due(s)
    # the chain: streamed and carried
    np.testing.assert_array_equal(chain[s], after["params"])
    np.testing.assert_array_equal(dlog[s][live], after["dlog"][live])
    np.testing.assert_allclose(chain[s][live], co.chain[s][live], rtol=1e-9, atol=1e-9, err_msg="%s params" % tag)
    np.testing.assert_array_equal(chain[s][~live], before["params"][~live])
    np.testing.assert_allclose(dlog[s][live], co.dlog[s][live], rtol=1e-9, atol=1e-9 * np.abs(co.dlog[s][live]).max(),
                               err_msg="%s dlog" % tag)
    assert accepted == int(co.counts.sum()) and 0 < accepted < int(live.sum())
    rel = np.max(np.abs(after["err"] - want_err)) / np.max(np.abs(want_err))
    print("%s residual (%s): %.3g of its peak" % (tag, "refreshed" if refresh else "carried", rel))
    assert rel <= 1e-11, "%s residual" % tag
    # adaptation
    np.testing.assert_allclose(after["scale"], co.scale, rtol=1e-13, atol=0., err_msg="%s jump scales" % tag)
    np.testing.assert_array_equal(after["acc"], co.acc, err_msg="%s accepted per spaxel" % tag)
    assert (after["n_win"], after["k"]) == (co.n_win, co.k)
    # the rescaling
    if not draw:
        np.testing.assert_array_equal(after["ivar"], before["ivar"])
    else:
        np.testing.assert_allclose(after["ivar"], co.ivar, rtol=1e-12, atol=0., err_msg="%s 1/variance" % tag)
        assert np.all(after["ivar"][~counted] == 0.)
        assert not np.array_equal(after["ivar"], before["ivar"])
    if ft["robust"]:
        assert after["robust"]["count"] == co.robust.count
        np.testing.assert_allclose(after["robust"]["mean"], co.robust.weight_mean(), rtol=1e-12, atol=0.)
        if draw:
            np.testing.assert_allclose(after["weights"][counted], co.robust.weights[counted], rtol=1e-12, atol=0.)
            assert np.isnan(after["weights"][~counted]).all()
    else:
        got, n = after["noise"], ft["noise"]
        assert list(got["sweeps"]) == list(before["noise"]["sweeps"]) + ([s] if draw else [])
        if draw:
            want = NO.draw_scales(pb["seed"], s, after["err"], pb["i0"], n["group"], n["spaxels"], n["shape"], n["rate"],
                                  len(before["tau_g"]), before["tau_g"])
            np.testing.assert_array_equal(got["voxels"], want["voxels"], err_msg="%s N_g" % tag)
            np.testing.assert_array_equal(got["sums"], want["sums"], err_msg="%s Q_g" % tag)
            assert (want["voxels"] >= 2).all() and want["margin"].min() > 1e-9
            np.testing.assert_allclose(got["tau"], want["tau"], rtol=1e-12, atol=0., err_msg="%s tau" % tag)
            np.testing.assert_allclose(got["scale"][-1], want["scale"], rtol=1e-12, atol=0.)
            np.testing.assert_array_equal(want["tau_g"], co.noise.tau_g)
        else:
            np.testing.assert_array_equal(got["tau"], before["noise"]["tau"])
    # the sample
    n = after["post"]["n"]
    assert n == co.post["n"] == before["post"]["n"] + int(sampled)
    moments_close(n, after["post"]["map"], co.post["map"], MAP_RTOL, MAP_RTOL, "%s map" % tag)
    moments_close(n, after["post"]["clean"], co.post["clean"], MEAN_RTOL, STD_RTOL, "%s clean" % tag)
    moments_close(n, after["post"]["conv"], co.post["conv"], MEAN_RTOL, STD_RTOL, "%s convolved" % tag)
    np.testing.assert_array_equal(after["rows"][:-1], before["rows"])
    np.testing.assert_array_equal(after["rows"][-1], co.rows[-1], err_msg="%s region scalars" % tag)
    np.testing.assert_array_equal(after["sizes"], [len(m) for m in CO.RG.members(ft["regions"]["labels"], pb["mask"],
                                                                                 ft["regions"]["K"])])
    moments_close(n, after["regions"]["spec"], co.spec, MEAN_RTOL, STD_RTOL, "%s spectra" % tag)
    # the histograms: frozen by sample number `pilot`, counted from the next one on
    pilot, span = ft["hist"]["pilot"], ft["hist"]["span"]
    rng, want = after["hist"]["range"], co.hist["range"]
    if n < pilot:
        assert np.isnan(rng).all()
    elif n == pilot:
        assert np.isnan(rng[~live]).all() and not np.isnan(rng[live]).any()
        for k, label in enumerate("acwF"):
            bar = (1. + span) * RANGE_RTOL * float(np.max(np.abs(co.post["map"][0][..., k])))
            err = float(np.nanmax(np.abs(rng[..., k, :] - want[..., k, :])))
            print("%s range of %s: max|d| = %.3g (bar %.3g)" % (tag, label, err, bar))
            assert err <= bar, "%s range of %s" % (tag, label)
    else:
        np.testing.assert_array_equal(rng, before["hist"]["range"])
    np.testing.assert_array_equal(after["hist"]["bins"], co.hist["bins"], err_msg="%s bins" % tag)
    np.testing.assert_array_equal(after["hist"]["tails"], co.hist["tails"], err_msg="%s tails" % tag)
    total = after["hist"]["bins"].sum(axis=-1, dtype=np.int64) + after["hist"]["tails"].sum(axis=-1, dtype=np.int64)
    assert (total[live] == max(n - pilot, 0)).all() and (total[~live] == 0).all()
    # the predictive accumulators: set R's density is the Student-t marginal, whose log1p is a libm call on
    # either side -- the bar of tests/test_gpu_predictive.py: test_student_t_uses_the_base_variance_and_the_marginal
    if ft["pred"]:
        M, S, mean, m2 = after["pred"]
        top = float(np.max(np.abs(co.pred.M)))
        for what, got, want, scale in (("M", M, co.pred.M, top), ("mean", mean, co.pred.mean, top),
                                       ("S", S, co.pred.S, 1.), ("M2", m2, co.pred.m2, top * top)):
            print("%s pred %s (%s residual): max deviation / scale %.3g" % (
                tag, what, "the oracle's carried" if refresh else "the device's", np.max(np.abs(got - want)) / max(scale, 1e-300)))
            np.testing.assert_allclose(got, want, rtol=PRED_RTOL, atol=PRED_RTOL * scale, err_msg="%s pred %s" % (tag, what))
        assert (M[~counted] == 0.).all() and (S[~counted] == 0.).all()


@pytest.mark.parametrize("name,which", [("small", "R"), ("small", "N"), ("fill", "R"), ("zb", "N")])
def test_stepwise_against_the_oracle(name, which):
    """Sweeps 1 .. 6 (`fill`: 1 .. 3 with a draw and a window every sweep): adapt steps, a refresh on a
    draw sweep (3) and on a sweep without a draw (6; `fill`: the draw sweep 3 alone), the histograms'
    freeze after sweep 2 and binned samples from sweep 3 on."""
    case = CASES[name]()
    pb = CO.problem_of(case, 0.1, case["ra"], 77)
    ft = features(case, which)
    H, W = case["H"], case["W"]
    n_sweeps = case["spec"]["sweeps"]
    rng = np.random.default_rng(5)
    seen = set()
    with armed_engine(case, ft) as eng:
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), pb["i0"])
        eng.residual(fetch=False)
        chain = np.full((n_sweeps + 1, H, W, 3), np.nan)
        dlog = np.full((n_sweeps + 1, H, W), np.nan)
        for s in range(1, n_sweeps + 1):
            tag = "%s %s sweep %d" % (name, which, s)
            before = download(eng, ft)
            before["err"] = before["err"] + OFFSET * np.max(np.abs(before["err"])) * rng.uniform(-1., 1., before["err"].shape)
            eng.upload_slot(_lib.SLOT_ERR, before["err"])
            co = CO.Composed(pb, ft, before)
            accepted = eng.mh_sweeps(1, s, 1, chain, dlog)
            check_path(eng, name)
            after = download(eng, ft)
            co.updates(s)
            want_err = co.st.err.copy()
            if co.refresh_due(s):
                want_err = pb["data0"] - O.forward_full(pb["dims"], co.st.params, pb["mask"], pb["fsf"], pb["lsf"])
            k_before = co.k
            co.end_of_sweep(s, device=dict(params=after["params"], err=after["err"]))
            compare_step(s, pb, ft, co, before, after, chain, dlog, accepted, want_err, tag)
            seen.update(w for w, on in (("adapt", co.k > k_before), ("window without a step", co.k == k_before and co.n_win == 0),
                                        ("refresh with a draw", co.refresh_due(s) and co.rescale_due(s)),
                                        ("refresh without a draw", co.refresh_due(s) and not co.rescale_due(s)),
                                        ("freeze", after["post"]["n"] == 2), ("binned", after["post"]["n"] > 2)) if on)
    want = {"adapt", "refresh with a draw", "freeze", "binned"} | ({"refresh without a draw"} if n_sweeps >= 6 else set())
    assert want <= seen, sorted(want - seen)


# ---- 2. one call against many ------------------------------------------------------------------------

def run_calls(case, ft, calls, between, name=None, seed=77):
    """The sweeps in `calls` calls; `between`: everything is downloaded after every call but the last."""
    H, W = case["H"], case["W"]
    total = sum(calls)
    with armed_engine(case, ft, seed) as eng:
        chain = np.full((total + 1, H, W, 3), np.nan)
        dlog = np.full((total + 1, H, W), np.nan)
        accepted, first = 0, 1
        for j, n in enumerate(calls):
            accepted += eng.mh_sweeps(n, first, 1, chain, dlog)
            first += n
            if j == 0:
                check_path(eng, name)
            if between and j + 1 < len(calls):
                download(eng, ft)
        out = download(eng, ft)
    out.update(chain=chain, dlog_chain=dlog, accepted=np.int64(accepted))
    return out


@pytest.mark.parametrize("name,which", [("small", "R"), ("small", "N"), ("fill", "R"), ("zb", "N")])
def test_one_call_is_many_calls_bit_for_bit(name, which):
    case = CASES[name]()
    ft = features(case, which)
    n = case["spec"]["sweeps"]
    whole = run_calls(case, ft, [n], False, name)
    split = run_calls(case, ft, [1] * n, True, name)
    same_bits(whole, split, "%s %s" % (name, which))
    assert whole["post"]["n"] == n and not np.isnan(whole["chain"][1:]).any()
    if name == "fill":          # (two sweeps of the chained strips back to back in the one call)
        quiet = run_calls(case, ft, [1] * n, False, name)
        same_bits(whole, quiet, "fill R, nothing downloaded between the calls")


# ---- 3. batched chains ----------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ["b48", "few"])
@pytest.mark.parametrize("which", ["R", "N"])
def test_batched_chains_are_the_single_contexts_bit_for_bit(geom, which):
    case = CASES[geom]()
    ft = features(case, which)
    n = case["spec"]["sweeps"]
    H, W = case["H"], case["W"]
    seeds = (77, 78)
    engs = [armed_engine(case, ft, seed) for seed in seeds]
    try:
        chains = [np.full((n + 1, H, W, 3), np.nan) for _ in seeds]
        dlogs = [np.full((n + 1, H, W), np.nan) for _ in seeds]
        accepted = _lib.mh_sweeps_batch(engs, n, 1, 1, chains, dlogs)
        check_path(engs[0], geom)
        both = [download(e, ft) for e in engs]
    finally:
        for e in engs:
            e.close()
    for r, seed in enumerate(seeds):
        both[r].update(chain=chains[r], dlog_chain=dlogs[r], accepted=np.int64(accepted[r]))
        same_bits(both[r], run_calls(case, ft, [n], False, seed=seed), "%s %s chain %d" % (geom, which, r))
    assert not np.array_equal(both[0]["params"], both[1]["params"])
