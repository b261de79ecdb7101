"""
CPU tests (no GPU) of the pointwise predictive accuracy (Run(predictive=...),
deconv3d_amd/predictive.py, tests/predictive_oracle.py): the keyword is validated and a run without
posterior_burn_in or with a host-evaluated model refused before any device work; the streaming
maximum and sum never overflow and equal a direct logsumexp; the pooling of chains equals the run
over the concatenated samples; the host's extraction, fold and comparison are the oracle's; the C
entry points are declared, bound, built and cite the reference lines they extend.
"""
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, predictive
from tests import predictive_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_pred_begin", "d3d_pred_count", "d3d_pred_get", "d3d_pred_maps", "d3d_pred_cubes", "d3d_pred_end")
POOL_FACTOR = 4.          # the "small multiple" of the streaming run's own deviation


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- keyword ------------------------------------------------------------------------------------

def test_keyword_becomes_a_dict():
    assert predictive.check_keyword(None, None) is None
    assert predictive.check_keyword(False, None) is None
    assert predictive.check_keyword(True, 5) == dict()
    assert predictive.check_keyword(dict(), 5) == dict()


@pytest.mark.parametrize("value", [1, 0, "yes", 2.5, (True,), dict(every=2), dict(nu=4)])
def test_run_refuses_bad_keywords_before_any_device_work(value):
    with pytest.raises(ValueError, match="predictive="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, posterior_burn_in=5, predictive=value)


@pytest.mark.parametrize("value", [True, dict()])
def test_run_needs_posterior_burn_in(value):
    with pytest.raises(ValueError, match="predictive= needs posterior_burn_in="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, predictive=value)


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="predictive=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, posterior_burn_in=5,
                predictive=True)


# ---- the streaming update -----------------------------------------------------------------------

def logsumexp(qs):
    qs = np.asarray(qs, dtype=np.longdouble)
    m = qs.max(axis=0)
    return m + np.log(np.exp(qs - m).sum(axis=0))


@pytest.mark.parametrize("order", ["rising", "falling", "alternating"])
def test_jumps_beyond_the_range_of_exp_neither_overflow_nor_lose_the_sum(order):
    """q moves by more than 745 = -log(smallest double) between consecutive samples: exp(q - M)
    of a naive running sum overflows on the way up and vanishes on the way down."""
    steps = np.array([0., -800., -1650., -2500.5, -2500.25, -4000., -4000.])
    qs = {"rising": steps[::-1], "falling": steps,
          "alternating": np.array([-4000., 0., -1650., -0.5, -800., -2500., -0.25])}[order]
    assert np.max(np.abs(np.diff(qs))[:3]) > 745. and np.abs(np.diff(qs)).max() > 745.
    qs = np.stack([qs, qs - 3.0e5, qs * 1e-3], axis=1)       # (three voxels: far below 0, and gentle)
    acc = PO.Accum((3,))
    for q in qs:
        acc.add(q)
        assert np.isfinite(acc.M).all() and np.isfinite(acc.S).all()
        assert np.all(acc.S >= 1.) and np.all(acc.S <= acc.n)
    np.testing.assert_array_equal(acc.M, qs.max(axis=0))
    got = acc.M + np.log(acc.S)
    want = logsumexp(qs)
    print(order, "M + log S", got, "direct", want)
    np.testing.assert_allclose(got, np.asarray(want, dtype=np.float64), rtol=1e-15, atol=0.)


def test_first_sample_and_uncounted_voxels():
    counted = np.array([True, False, True])
    err, i0 = np.array([1., 7., 200.]), np.array([4., 0., 0.25])
    q = PO.q_of(err, i0)
    np.testing.assert_array_equal(q, [-2., 0., -5000.])
    acc = PO.Accum((3,)).add(np.array([-2., -5., -5000.]), counted)
    np.testing.assert_array_equal(acc.M, [-2., 0., -5000.])
    np.testing.assert_array_equal(acc.S, [1., 0., 1.])
    np.testing.assert_array_equal(acc.mean, [-2., 0., -5000.])
    np.testing.assert_array_equal(acc.m2, [0., 0., 0.])
    lppd, p = PO.extract(1, acc.M, acc.S, acc.m2, i0)
    np.testing.assert_array_equal(lppd, PO.log_density(err, i0))      # one sample: its density
    assert np.isnan(p).all() and np.isnan(lppd[1])


# ---- both densities -------------------------------------------------------------------------------

@pytest.mark.parametrize("nu", [0, 1, 4, 30])
def test_densities_are_scipys(nu):
    from scipy import stats
    rng = np.random.default_rng(3)
    r, i0 = rng.normal(0., 3., 200), rng.uniform(0.1, 5., 200)
    dist = stats.norm() if nu == 0 else stats.t(nu)
    want = dist.logpdf(r * np.sqrt(i0)) + 0.5 * np.log(i0)          # y = r sqrt(i0) is standard
    np.testing.assert_allclose(PO.log_density(r, i0, nu), want, rtol=1e-12, atol=1e-12)
    assert predictive.log_norm(nu) == PO.log_norm(nu)


# ---- pooling ----------------------------------------------------------------------------------------

def dev(a, ref):
    """Largest deviation from the extended-precision value, in units of the array's scale."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("blocks", [(30, 30, 30), (1, 57, 2, 40), (25, 0, 25)])
def test_pooled_accumulators_equal_the_concatenated_run(blocks):
    """R blocks merged against one run over all their samples: M bit for bit; S, mean and M2 within
    POOL_FACTOR times the deviation of the single streaming run from the extended-precision values
    (both judged against those), never below one ulp of the scale."""
    rng = np.random.default_rng(11)
    shape = (6, 5, 4)
    base = rng.normal(-40., 30., shape)
    qs = [-np.abs(base + rng.normal(0., 5., shape) * (1. + 10. * (rng.random(shape) < 0.1)))
          for _ in range(sum(blocks))]
    whole = PO.accumulate(qs)
    at, parts = 0, []
    for n in blocks:
        parts.append(PO.accumulate(qs[at:at + n]).parts() if n else (0,) + (np.zeros(shape),) * 4)
        at += n
    n, M, S, mean, m2 = PO.merge(parts)
    assert n == whole.n == sum(blocks)
    np.testing.assert_array_equal(M, whole.M)
    exact = PO.direct(qs)
    np.testing.assert_array_equal(M, np.asarray(exact[0], dtype=np.float64))
    eps = np.finfo(np.float64).eps
    for name, got, one, ref in (("S", S, whole.S, exact[1]), ("mean", mean, whole.mean, exact[2]),
                                ("M2", m2, whole.m2, exact[3])):
        own, pooled = dev(one, ref), dev(got, ref)
        print(blocks, name, "streaming %.3g pooled %.3g (eps %.3g)" % (own, pooled, eps))
        assert pooled <= POOL_FACTOR * max(own, eps), name
    # the product's merge is the oracle's, bit for bit
    for a, b in zip(predictive.merge(parts), (n, M, S, mean, m2)):
        np.testing.assert_array_equal(a, b)


# ---- extraction, fold, comparison -------------------------------------------------------------------

def hand_made(seed, D=5, H=3, W=4, n=9, shift=0.):
    rng = np.random.default_rng(seed)
    i0 = rng.uniform(0.5, 2., (D, H, W))
    i0[1, 0, 0] = i0[4, 2, 3] = 0.
    qs = [-(rng.normal(shift, 1., (D, H, W)) ** 2) for _ in range(n)]
    acc = PO.accumulate(qs, i0 != 0.)
    return acc, i0


def test_host_extraction_and_fold_are_the_oracles():
    acc, i0 = hand_made(5)
    for nu in (0, 4):
        want = PO.extract(acc.n, acc.M, acc.S, acc.m2, i0, nu)
        pa = predictive.PredictiveAccuracy.from_accumulators(acc.n, acc.M, acc.S, acc.mean, acc.m2, i0, nu)
        np.testing.assert_array_equal(pa.lppd_cube, want[0])
        np.testing.assert_array_equal(pa.p_waic_cube, want[1])
        maps = PO.fold_maps(*want)
        np.testing.assert_array_equal(pa.lppd_map, maps[..., 0])
        np.testing.assert_array_equal(pa.p_waic_map, maps[..., 1])
        np.testing.assert_array_equal(pa.voxels, (i0 != 0.).sum(0))
        np.testing.assert_array_equal(pa.elpd_map, maps[..., 0] - maps[..., 1])
        lppd, p, elpd, se = PO.scalars(maps)
        assert (pa.lppd, pa.p_waic, pa.elpd, pa.waic) == (lppd, p, lppd - p, -2. * (lppd - p))
        live = i0 != 0.
        pointwise = (want[0] - want[1])[live]
        np.testing.assert_allclose(elpd, pointwise.sum(), rtol=1e-13)
        np.testing.assert_allclose(pa.se, np.sqrt(pointwise.size * pointwise.var(ddof=1)), rtol=1e-10)
        assert pa.nu == nu and pa.count == acc.n
        assert np.isnan(pa.lppd_cube[~live]).all() and np.isfinite(pa.lppd_cube[live]).all()


def test_fold_is_a_sum_in_the_devices_order():
    """70 channel pairs: lanes 0 .. 5 take two pairs each; the plain sum agrees to rounding, the fold
    itself is pinned on powers of two, where every order is exact."""
    rng = np.random.default_rng(2)
    lppd = rng.normal(-3., 1., (139, 2, 2))
    lppd[7, 0, 1] = np.nan
    p = np.where(np.isnan(lppd), np.nan, rng.uniform(0., 1., lppd.shape))
    maps = PO.fold_maps(lppd, p)
    np.testing.assert_allclose(maps[..., 0], np.nansum(lppd, 0), rtol=1e-13)
    np.testing.assert_allclose(maps[..., 3], np.nansum((lppd - p) ** 2, 0), rtol=1e-13)
    np.testing.assert_array_equal(maps[..., 2], [[139, 138], [139, 139]])
    exact = np.where(np.isnan(lppd), np.nan, 2. ** rng.integers(-3, 4, lppd.shape))
    np.testing.assert_array_equal(PO.fold_maps(exact, exact * 0.)[..., 0], np.nansum(exact, 0))
    np.testing.assert_array_equal(predictive.fold_maps(lppd, p), maps)


def test_compare_on_hand_made_cubes(tmp_path):
    shape = (2, 1, 3)
    lppd_a = np.array([[[-1., -2., np.nan]], [[-3., -1., -2.]]])
    p_a = np.where(np.isnan(lppd_a), np.nan, 0.5)
    lppd_b = lppd_a - np.array([[[1., 0., 0.]], [[2., 1., 3.]]])
    p_b = np.where(np.isnan(lppd_b), np.nan, 0.25)

    def report(lppd, p):
        return predictive.PredictiveAccuracy(7, lambda: PO.fold_maps(lppd, p), lambda a=True, b=True: (lppd, p))

    a, b = report(lppd_a, p_a), report(lppd_b, p_b)
    d = np.array([1., 0., 2., 1., 3.]) - 0.25
    delta, se = a.compare(b)
    assert delta == d.sum() == 5.75
    np.testing.assert_allclose(se, np.sqrt(5 * d.var(ddof=1)), rtol=1e-15)
    back = b.compare(a)
    assert back[0] == -delta and back[1] == se
    assert a.compare(a) == (0., 0.)
    assert (delta, se) == PO.compare(lppd_a, p_a, lppd_b, p_b)
    np.testing.assert_allclose(a.elpd - b.elpd, delta, rtol=1e-15)
    # another shape, another set of counted voxels
    with pytest.raises(ValueError, match="different shapes"):
        a.compare(report(lppd_a[:1], p_a[:1]))
    other = lppd_b.copy()
    other[0, 0, 2], other[1, 0, 0] = -1., np.nan
    with pytest.raises(ValueError, match="count different voxels"):
        a.compare(report(other, np.where(np.isnan(other), np.nan, 0.25)))
    assert shape == a.lppd_cube.shape
    a.save(str(tmp_path / "r"))
    saved = np.load(str(tmp_path / "r_posterior_predictive.npz"))
    assert int(saved["count"]) == 7 and float(saved["elpd"]) == a.elpd
    np.testing.assert_array_equal(saved["lppd_cube"], lppd_a)
    np.testing.assert_array_equal(saved["voxels"], [[2, 2, 1]])


def test_pooled_report_merges_lazily_and_extracts_on_the_host():
    (acc_a, i0), (acc_b, _) = hand_made(5), hand_made(6, n=4, shift=1.)
    calls = []

    def part(acc):
        def raw():
            calls.append(acc.n)
            return acc.M, acc.S, acc.mean, acc.m2
        return predictive.PredictiveAccuracy(acc.n, None, None, raw, nu=4)

    both = predictive.pooled([part(acc_a), part(acc_b)], i0)
    assert both.count == 13 and both.nu == 4 and calls == []          # nothing fetched yet
    n, M, S, mean, m2 = PO.merge([acc_a.parts(), acc_b.parts()])
    want = PO.extract(n, M, S, m2, i0, 4)
    np.testing.assert_array_equal(both.lppd_cube, want[0])
    np.testing.assert_array_equal(both.p_waic_cube, want[1])
    np.testing.assert_array_equal(both.lppd_map, PO.fold_maps(*want)[..., 0])
    assert sorted(calls) == [4, 9]                                      # once each
    np.testing.assert_array_equal(predictive.base_ivar(np.array([1., np.nan, 2.]), np.array([4., 1., 0.])),
                                  PO.base_ivar(np.array([1., np.nan, 2.]), np.array([4., 1., 0.])))


def test_posterior_moments_carry_and_save_it(tmp_path):
    from deconv3d_amd import posterior
    pm = posterior.PosteriorMoments(0, lambda which: (np.zeros((1, 1, 4)), np.zeros((1, 1, 4)))
                                    if which == 0 else (np.zeros((2, 1, 1)), np.zeros((2, 1, 1))))
    assert pm.predictive is None
    assert d3d.PredictiveAccuracy is predictive.PredictiveAccuracy


# ---- the C ABI ---------------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_built_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("pointwise predictive accuracy: lppd and WAIC per voxel"):]
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.PRED_PROTOTYPES
        decl = section.index("int %s(" % name)
        comment = section[section.rindex("/*", 0, decl):decl]
        assert "lib/run.py:407-426" in comment, name
    for name in ("pred_begin", "pred_count", "pred_get", "pred_maps", "pred_cubes", "pred_end"):
        assert callable(getattr(_lib.Engine, name))
    make = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\bd3d_pred\.hip\b", make, flags=re.M)
    import __graft_entry__ as entry
    assert "d3d_pred.hip" in entry.SOURCES                                     # d3d_source_hash covers it
    src = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "d3d_pred.hip")).read()
    assert "fp contract(off)" in src
    for kernel in ("k_pred_accum", "k_pred_maps", "k_pred_view"):
        assert kernel in src
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)                                           # the default library exports them
    for name in ENTRIES:
        assert hasattr(lib, name), name
