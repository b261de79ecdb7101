"""
CPU tests (no GPU) of the region posteriors' host side (deconv3d_amd/regions.py: the label builders,
check_regions, RegionPosterior, pooled; Run(regions=...)) and of the numpy restatement of their
contract the GPU tests compare the device with (tests/region_oracle.py).
"""
import math

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior, regions
from tests import region_oracle as RO


# ---- the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 128, 357, 1000])
def test_oracle_sums_agree_with_fsum(n):
    """The fixed order is a sum of n terms like any other: within n 2^-52 of sum |terms| of the
    exactly rounded sum (the a-priori bound of any summation order is (n - 1) u sum |terms| to first
    order, u = 2^-53)."""
    rng = np.random.default_rng(n)
    for scale in (1.0, 1e-8):
        terms = rng.normal(size=n) * np.exp(scale * rng.normal(size=n))
        got = RO.chunked_sum(terms)
        want = math.fsum(terms)
        bound = n * 2.0 ** -52 * math.fsum(np.abs(terms))
        print("n = %d: |d| = %.3g (bound %.3g)" % (n, abs(got - want), bound))
        assert abs(got - want) <= bound


def test_oracle_sum_of_66_chunks_agrees_with_fsum():
    """4161 terms: 65 full chunks and one of a single term, the largest region of
    tests/test_gpu_regions.py's wide field -- within n eps sum |terms| of the exactly rounded sum."""
    n = 4161
    rng = np.random.default_rng(n)
    for scale in (1.0, 1e-8):
        terms = rng.normal(size=n) * np.exp(scale * rng.normal(size=n))
        got = RO.chunked_sum(terms)
        want = math.fsum(terms)
        bound = n * np.finfo(np.float64).eps * math.fsum(np.abs(terms))
        print("n = %d: |d| = %.3g (bound %.3g)" % (n, abs(got - want), bound))
        assert abs(got - want) <= bound
    # (and the chunking is what it says: 66 partials, the last a single term)
    parts = [RO.fold_by_halves(terms[m:m + RO.CHUNK]) for m in range(0, n, RO.CHUNK)]
    assert len(parts) == 66 and parts[-1] == terms[-1]


def test_oracle_fold_by_halves_is_the_xor_butterfly():
    """v[:32] + v[32:], ... is what lane 0 of the xor-butterfly v[l] += v[l ^ d], d = 32 .. 1, holds."""
    rng = np.random.default_rng(3)
    for n in (1, 17, 64):
        terms = rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, size=n)
        v = np.zeros(64)
        v[:n] = terms
        d = 32
        while d:
            v = v + v[np.arange(64) ^ d]
            d //= 2
        assert (v == v[0]).all() and v[0] == RO.fold_by_halves(terms)


def test_oracle_scalars_of_a_hand_made_map():
    params = np.zeros((2, 3, 3))
    params[..., 0] = [[1., 2., 0.], [4., 1., 3.]]
    params[..., 1] = [[10., 12., 99.], [10., 10., 5.]]
    params[..., 2] = [[1., 0.5, 7.], [0.25, 2., 1.]]
    labels = np.array([[1, 1, 2], [1, 0, 3]])
    mask = np.array([[1, 1, 1], [1, 1, 0]])
    got = RO.scalars(params, labels, mask, 4, 2.0)
    # region 1: F_i = 2, 2, 2 at c = 10, 12, 10
    assert got[0, 0] == 6.0 and got[0, 1] == 32.0 / 3.0
    d = np.array([10., 12., 10.]) - 32.0 / 3.0
    want = np.sqrt(np.sum(2.0 * (np.array([1., 0.5, 0.25]) ** 2 + d ** 2)) / 6.0)
    assert abs(got[0, 2] - want) <= 4 * np.finfo(float).eps * want
    assert got[1, 0] == 0.0 and np.isnan(got[1, 1:]).all()          # no flux
    assert got[2, 0] == 0.0 and np.isnan(got[2, 1:]).all()          # every member masked
    assert got[3, 0] == 0.0 and np.isnan(got[3, 1:]).all()          # no member
    assert [len(m) for m in RO.members(labels, mask, 4)] == [3, 1, 0, 0]


def test_oracle_welford_and_spectra():
    rng = np.random.default_rng(5)
    stack = rng.normal(size=(7, 3, 4))
    mean, m2 = RO.welford(stack)
    np.testing.assert_allclose(mean, stack.mean(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(m2, stack.var(axis=0) * 7, rtol=1e-13)
    params = np.dstack((1 + rng.random((9, 9)), 3 + 4 * rng.random((9, 9)), 0.5 + rng.random((9, 9))))
    labels = np.ones((9, 9), dtype=int)
    mask = np.ones((9, 9))
    mask[4, 4] = 0
    line = RO.gaussian_unit_line()
    got = RO.spectra(params, labels, mask, 1, 10, line)
    z = np.arange(10.)
    want = sum(p[0] * np.exp(-(z - p[1]) ** 2 / (2 * p[2] ** 2))
               for p, m in zip(params.reshape(-1, 3), mask.reshape(-1)) if m)
    np.testing.assert_allclose(got[0], want, rtol=1e-13)


# ---- the builders -------------------------------------------------------------------------------

def test_blocks():
    lab = regions.blocks((5, 7), 3)
    assert lab.dtype == np.int32 and lab.shape == (5, 7)
    np.testing.assert_array_equal(lab[0], [1, 1, 1, 2, 2, 2, 3])
    np.testing.assert_array_equal(lab[:, 0], [1, 1, 1, 4, 4])
    assert lab.max() == 6 and lab.min() == 1
    np.testing.assert_array_equal(regions.blocks((4, 4), 1).reshape(-1), np.arange(1, 17))
    assert (regions.blocks((4, 4), 9) == 1).all()
    with pytest.raises(ValueError):
        regions.blocks((4, 4), 0)


def test_annuli():
    lab = regions.annuli((21, 21), (10, 10), [0., 2., 5., 9.])
    assert lab.dtype == np.int32 and lab[10, 10] == 1 and lab[10, 11] == 1 and lab[10, 12] == 2
    assert lab[10, 15] == 3 and lab[10, 19] == 0 and lab[0, 0] == 0
    y, x = np.mgrid[0:21, 0:21]
    r = np.hypot(y - 10, x - 10)
    np.testing.assert_array_equal(lab == 2, (r >= 2) & (r < 5))
    np.testing.assert_array_equal(lab, lab[::-1, ::-1])            # circles are symmetric
    # inclined: the minor axis is foreshortened by cos i, the major axis (along y at pa = 0) is not
    inc = regions.annuli((21, 21), (10, 10), [0., 3.5], pa=0., inclination=60.)
    assert inc[13, 10] == 1 and inc[10, 13] == 0 and inc[10, 11] == 1 and inc[10, 12] == 0
    turned = regions.annuli((21, 21), (10, 10), [0., 3.5], pa=90., inclination=60.)
    np.testing.assert_array_equal(turned, inc.T)
    hole = regions.annuli((21, 21), (10, 10), [3., 6.])
    assert hole[10, 10] == 0 and hole[10, 14] == 1
    for bad in ([1.], [2., 1.], [-1., 2.], [0., np.inf]):
        with pytest.raises(ValueError):
            regions.annuli((21, 21), (10, 10), bad)
    with pytest.raises(ValueError):
        regions.annuli((21, 21), (10, 10), [0., 2.], inclination=90.)


# ---- the keyword --------------------------------------------------------------------------------

def test_keyword_is_normalised():
    assert regions.check_regions(None, (3, 4), None) is None
    lab = np.array([[0, 7, 7, 3], [0, 0, 3, 900], [7, 0, 0, 0]])
    got = regions.check_regions(lab, (3, 4), 5)
    np.testing.assert_array_equal(got["ids"], [3, 7, 900])
    np.testing.assert_array_equal(got["labels"], [[0, 2, 2, 1], [0, 0, 1, 3], [2, 0, 0, 0]])
    assert got["labels"].dtype == np.int32 and got["spectra"] is True
    got = regions.check_regions(dict(labels=lab.astype(np.uint8), spectra=False), (3, 4), 5)
    assert got["spectra"] is False and got["labels"].max() == 3
    assert regions.check_regions(lab, None, 5)["labels"].shape == (3, 4)     # shape checked later


GOOD = np.ones((9, 9), dtype=np.int32)
BAD_KEYWORDS = [dict(regions=GOOD),                                                   # no posterior_burn_in
                dict(posterior_burn_in=2, regions=np.ones((9, 8), dtype=np.int32)),   # wrong shape
                dict(posterior_burn_in=2, regions=np.ones((9, 9, 1), dtype=np.int32)),
                dict(posterior_burn_in=2, regions=np.ones((9, 9))),                   # not integers
                dict(posterior_burn_in=2, regions=np.ones((9, 9), dtype=bool)),
                dict(posterior_burn_in=2, regions=GOOD - 2),                          # negatives
                dict(posterior_burn_in=2, regions=GOOD * 0),                          # all zeros
                dict(posterior_burn_in=2, regions=dict(spectra=True)),                # no labels
                dict(posterior_burn_in=2, regions=dict(labels=GOOD, spectra="yes")),
                dict(posterior_burn_in=2, regions=dict(labels=GOOD, chunks=32))]


@pytest.mark.parametrize("kw", BAD_KEYWORDS)
def test_run_refuses_a_bad_keyword_before_any_device_work(kw, monkeypatch):
    with pytest.raises(ValueError, match="regions="):
        regions.check_regions(kw["regions"], (9, 9), kw.get("posterior_burn_in"))

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "Engine", no_device)
    cube = d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)))
    with pytest.raises(ValueError, match="regions="):
        d3d.Run(cube, d3d.MUSE(), max_iterations=4, **kw)


def test_binding_declares_the_entry_points():
    for name in ("d3d_region_begin", "d3d_region_count", "d3d_region_get", "d3d_region_end"):
        assert name in _lib.SYMBOLS and name in _lib.REGION_PROTOTYPES
    assert d3d.RegionPosterior is regions.RegionPosterior
    for name in ("region_begin", "region_count", "region_get", "region_end"):
        assert callable(getattr(_lib.Engine, name))


# ---- RegionPosterior with fake fetchers ---------------------------------------------------------

def fake(series, spec=None, sizes=None, ids=None, count=None):
    """A RegionPosterior over a given series (n, K, 3) and spectra samples (n, K, D); counts the fetches."""
    calls = []
    K = series.shape[1]

    def get():
        calls.append(1)
        mean = m2 = None
        if spec is not None:
            mean, m2 = RO.welford(spec) if len(spec) else (np.zeros(spec.shape[1:]),) * 2
        return series, mean, m2, np.arange(K) + 2 if sizes is None else sizes
    n = len(series) if count is None else count
    return regions.RegionPosterior(n, get, ids), calls


def test_region_posterior_summaries_and_lazy_download():
    rng = np.random.default_rng(8)
    series = rng.normal(size=(50, 3, 3)) + [10., 5., 2.]
    spec = rng.normal(size=(50, 3, 6))
    rp, calls = fake(series, spec, ids=[4, 9, 11])
    assert rp.count == 50 and not calls
    np.testing.assert_array_equal(rp.ids, [4, 9, 11])
    assert not calls
    np.testing.assert_array_equal(rp.flux, series[..., 0])
    np.testing.assert_array_equal(rp.centre, series[..., 1])
    np.testing.assert_array_equal(rp.width, series[..., 2])
    np.testing.assert_array_equal(rp.sizes, [2, 3, 4])
    np.testing.assert_array_equal(rp.flux_mean, series[..., 0].mean(axis=0))
    np.testing.assert_array_equal(rp.width_std, series[..., 2].std(axis=0, ddof=1))
    q = rp.quantiles([0.16, 0.5, 0.84])
    assert q.shape == (3, 3, 3)
    np.testing.assert_array_equal(q[1, 2], np.quantile(series[:, 1, 2], [0.16, 0.5, 0.84]))
    np.testing.assert_allclose(rp.flux_covariance(), np.cov(series[..., 0].T), rtol=1e-12)
    np.testing.assert_allclose(rp.spectrum_mean, spec.mean(axis=0), atol=1e-14)
    np.testing.assert_allclose(rp.spectrum_std, spec.std(axis=0, ddof=1), rtol=1e-12)
    assert len(calls) == 1                                          # one download for everything
    with pytest.raises(ValueError):
        rp.quantiles([1.5])
    assert fake(series)[0].ids.tolist() == [1, 2, 3]               # no ids: 1..K


def test_anticorrelated_neighbours_show_in_the_covariance():
    rng = np.random.default_rng(9)
    trade = rng.normal(size=400)
    flux = np.stack([10. + trade, 10. - trade + 0.1 * rng.normal(size=400)], axis=1)
    series = np.dstack([flux, np.ones_like(flux), np.ones_like(flux)])
    cov = fake(series)[0].flux_covariance()
    assert cov[0, 1] < 0 and cov[0, 1] == cov[1, 0]
    assert cov[0, 0] + cov[1, 1] + 2 * cov[0, 1] < 0.05 * (cov[0, 0] + cov[1, 1])   # the sum is well determined


def test_no_sample_is_nan_and_no_spectra_is_none():
    rp, _ = fake(np.empty((0, 2, 3)), np.empty((0, 2, 5)))
    assert rp.count == 0 and rp.flux.shape == (0, 2)
    for arr in (rp.flux_mean, rp.flux_std, rp.centre_mean, rp.width_std, rp.quantiles([0.5]), rp.flux_covariance(),
                rp.spectrum_mean, rp.spectrum_std):
        assert np.isnan(arr).all()
    assert rp.quantiles([0.1, 0.9]).shape == (2, 3, 2) and rp.spectrum_mean.shape == (2, 5)
    one, _ = fake(np.ones((1, 2, 3)), np.ones((1, 2, 5)))
    assert (one.flux_mean == 1.).all() and np.isnan(one.flux_std).all() and np.isnan(one.spectrum_std).all()
    assert np.isnan(one.flux_covariance()).all()
    bare, _ = fake(np.ones((4, 2, 3)))
    assert bare.spectrum_mean is None and bare.spectrum_std is None
    with pytest.raises(ValueError):
        bare.spectrum_moments()


def test_a_full_series_keeps_counting_the_spectra():
    rng = np.random.default_rng(10)
    spec = rng.normal(size=(9, 2, 4))
    rp, _ = fake(np.ones((5, 2, 3)), spec, count=9)               # capacity 5, nine samples taken
    assert rp.count == 9 and rp.flux.shape == (5, 2)
    np.testing.assert_allclose(rp.spectrum_std, spec.std(axis=0, ddof=1), rtol=1e-12)


def test_pooling_concatenates_the_series_and_pools_the_spectra():
    rng = np.random.default_rng(11)
    sers = [rng.normal(size=(n, 2, 3)) for n in (6, 0, 9)]
    specs = [rng.normal(size=(n, 2, 5)) + r for r, n in enumerate((6, 0, 9))]
    parts = [fake(s, sp, ids=[5, 8])[0] for s, sp in zip(sers, specs)]
    both = regions.pooled(parts)
    assert both.count == 15
    np.testing.assert_array_equal(both.ids, [5, 8])
    np.testing.assert_array_equal(both.series, np.concatenate(sers))
    every = np.concatenate(specs)
    np.testing.assert_allclose(both.spectrum_mean, every.mean(axis=0), atol=1e-14)
    np.testing.assert_allclose(both.spectrum_std, every.std(axis=0, ddof=1), rtol=1e-12)
    np.testing.assert_array_equal(both.flux_mean, np.concatenate(sers)[..., 0].mean(axis=0))
    bare = regions.pooled([fake(s)[0] for s in sers])
    assert bare.spectrum_mean is None and bare.flux.shape == (15, 2)


def test_save_writes_the_npz(tmp_path):
    rng = np.random.default_rng(12)
    series, spec = rng.normal(size=(4, 2, 3)), rng.normal(size=(4, 2, 5))
    rp, _ = fake(series, spec, ids=[3, 30])
    rp.save(str(tmp_path / "out"))
    got = np.load(str(tmp_path / "out_posterior_regions.npz"))
    assert int(got["count"]) == 4 and got["ids"].tolist() == [3, 30] and got["sizes"].tolist() == [2, 3]
    np.testing.assert_array_equal(got["flux"], series[..., 0])
    np.testing.assert_array_equal(got["spectrum_std"], rp.spectrum_std)
    # PosteriorMoments.save writes its regions too
    pm = posterior.PosteriorMoments(4, lambda which: (np.zeros((2, 2, 4) if which == 0 else (3, 2, 2)),) * 2)
    pm.regions = fake(series)[0]
    pm.save(str(tmp_path / "run"))
    got = np.load(str(tmp_path / "run_posterior_regions.npz"))
    assert "spectrum_mean" not in got.files and got["width"].shape == (4, 2)
