"""
CPU tests (no GPU) of the posterior histograms' host side (deconv3d_amd/posterior.py:
check_histograms, PosteriorHistograms; Run(posterior_histograms=...)) and of the numpy restatement
of their contract the GPU tests compare the device with (tests/histogram_oracle.py).
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior
from tests import histogram_oracle as HO


def test_keyword_is_normalised():
    assert posterior.check_histograms(None, None) is None
    assert posterior.check_histograms(None, 5) is None
    assert posterior.check_histograms(False, 5) is None
    assert posterior.check_histograms(True, 5) == dict(pilot=200, span=6.0)
    assert posterior.check_histograms({}, 5) == dict(pilot=200, span=6.0)
    assert posterior.check_histograms(dict(pilot=np.int64(24)), 5) == dict(pilot=24, span=6.0)
    got = posterior.check_histograms(dict(span=3, pilot=2), 1)
    assert got == dict(pilot=2, span=3.0) and isinstance(got["span"], float) and isinstance(got["pilot"], int)


BAD_KEYWORDS = [dict(posterior_histograms=True),                                    # no posterior_burn_in
                dict(posterior_histograms=dict(pilot=24)),
                dict(posterior_burn_in=3, posterior_histograms=dict(pilot=1)),
                dict(posterior_burn_in=3, posterior_histograms=dict(pilot=2.5)),
                dict(posterior_burn_in=3, posterior_histograms=dict(pilot=True)),
                dict(posterior_burn_in=3, posterior_histograms=dict(span=0.)),
                dict(posterior_burn_in=3, posterior_histograms=dict(span=-1.)),
                dict(posterior_burn_in=3, posterior_histograms=dict(span=float("inf"))),
                dict(posterior_burn_in=3, posterior_histograms=dict(span=float("nan"))),
                dict(posterior_burn_in=3, posterior_histograms=dict(span="6")),
                dict(posterior_burn_in=3, posterior_histograms=dict(bins=128)),
                dict(posterior_burn_in=3, posterior_histograms=200),
                dict(posterior_burn_in=3, posterior_histograms="yes")]


@pytest.mark.parametrize("kw", BAD_KEYWORDS)
def test_run_refuses_a_bad_keyword_before_any_device_work(kw):
    with pytest.raises(ValueError, match="posterior_histograms"):
        posterior.check_histograms(kw["posterior_histograms"], kw.get("posterior_burn_in"))
    cube = d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)))
    with pytest.raises(ValueError, match="posterior_histograms"):
        d3d.Run(cube, d3d.MUSE(), max_iterations=4, **kw)


def test_binding_declares_the_entry_points():
    for name in ("d3d_hist_begin", "d3d_hist_count", "d3d_hist_get", "d3d_hist_quantiles", "d3d_hist_end"):
        assert name in _lib.SYMBOLS and name in _lib.HIST_PROTOTYPES
    assert d3d.PosteriorHistograms is posterior.PosteriorHistograms
    for name in ("hist_begin", "hist_count", "hist_get", "hist_quantiles", "hist_end"):
        assert callable(getattr(_lib.Engine, name))


def synthetic(name, n, rng):
    """(n, 2, 3, 4) series: four differently shaped marginals, the same law in every spaxel."""
    shape = (n, 2, 3)
    if name == "normal":
        cols = [rng.normal(5., 1., shape), rng.normal(-3., 0.1, shape), rng.normal(0., 7., shape),
                rng.normal(1e3, 2., shape)]
    elif name == "heavy":           # Student t with 3 degrees of freedom: samples far beyond 6 sd of a pilot
        cols = [rng.standard_t(3, shape), 10. + rng.standard_t(3, shape), rng.standard_t(3, shape) * 0.01,
                rng.standard_t(3, shape) - 4.]
    elif name == "bimodal":         # two separated modes, both visited by the pilot
        pick = rng.random(shape) < 0.3
        cols = [np.where(pick, rng.normal(2., 0.2, shape), rng.normal(6., 0.3, shape)) + k for k in range(4)]
    elif name == "bounded":         # piles up against the lower bound, as a width at min_w does
        cols = [np.abs(rng.normal(0., 1., shape)) + k for k in range(4)]
    else:
        raise KeyError(name)
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("name", ["normal", "heavy", "bimodal", "bounded"])
@pytest.mark.parametrize("pilot,n,span", [(24, 37, 6.0), (200, 1013, 6.0), (50, 333, 2.0)])
def test_restated_quantile_lies_within_a_bin_of_the_sample_quantile(name, pilot, n, span):
    """Both values lie in the same bin whenever q n falls inside the range (the histogram's cumulative
    count first reaches q n in the bin of the sample of rank ceil(q n)), so they differ by less than
    its width; q n is never an integer here."""
    rng = np.random.default_rng(100 + n)
    x = synthetic(name, pilot + n, rng)
    L, U = np.full(4, -1e9), np.full(4, 1e9)
    if name == "bounded":
        L = np.arange(4.)
    lo, hi = HO.freeze(*HO.welford(x[:pilot]), pilot, span, L, U)
    assert (hi > lo).all() and (lo >= L).all()
    bins, tails = HO.count(x[pilot:], lo, hi)
    total = bins.sum(axis=-1, dtype=np.int64) + tails.sum(axis=-1, dtype=np.int64)
    assert (total == n).all()
    rng2 = np.stack((lo, hi), axis=-1)
    width = (hi - lo) / 64.
    checked = 0
    for q in (0.16, 0.5, 0.84, 0.025, 0.975):
        assert q * n != np.floor(q * n)
        got = HO.quantile(bins, tails, rng2, q)
        want = np.quantile(x[pilot:], q, axis=0, method="inverted_cdf")
        inside = (q * n > tails[..., 0]) & (q * n <= n - tails[..., 1].astype(np.int64))
        assert (got[~inside & (q * n <= tails[..., 0])] == lo[~inside & (q * n <= tails[..., 0])]).all()
        assert (np.abs(got - want)[inside] <= width[inside]).all(), (name, q)
        assert (got[inside] >= lo[inside]).all() and (got[inside] <= hi[inside]).all()
        checked += int(inside.sum())
    # (a range of 2 sd leaves the 2.5 % quantiles in its tails; the central three stay inside)
    assert checked >= 0.8 * (5 if span == 6.0 else 3) * lo.size
    if name == "heavy" and span == 6.0 and n > 1000:
        assert tails.sum() > 0            # the case does exercise the tails


def test_restatement_edges():
    lo, hi = np.array([0., 0., 5., np.nan]), np.array([64., 64., 5., np.nan])
    # exactly lo -> bin 0; exactly hi -> above; just below lo -> below; a bin edge -> the upper bin
    x = np.array([[0., -1e-300, 5., 1.], [64., np.nextafter(64., 0.), 5., 1.], [1., 63., 5., 1.], [1., 63.5, 4., 1.]])
    bins, tails = HO.count(x, lo, hi)
    assert bins[0, 0] == 1 and bins[0, 1] == 2 and tails[0].tolist() == [0, 1]
    assert bins[1, 63] == 3 and tails[1].tolist() == [1, 0]
    assert bins[2].sum() == 0 and tails[2].sum() == 0 and bins[3].sum() == 0 and tails[3].sum() == 0
    rng = np.stack((lo, hi), axis=-1)
    assert np.isnan(HO.quantile(bins, tails, rng, 0.5)[2:]).all()
    assert np.isnan(HO.mode(bins, tails, rng)[2:]).all() and np.isnan(HO.outside(bins, tails, rng)[2:]).all()
    assert HO.mode(bins, tails, rng)[0] == 1.5 and HO.mode(bins, tails, rng)[1] == 63.5
    assert HO.outside(bins, tails, rng)[0] == 0.25
    assert HO.quantile(bins, tails, rng, 0.9)[0] == 64. and HO.quantile(bins, tails, rng, 0.2)[1] == 0.
    # ties: the lowest of the fullest bins
    b = np.zeros((1, 64), dtype=np.uint32)
    b[0, [7, 40]] = 3
    assert HO.mode(b, np.zeros((1, 2), dtype=np.uint32), np.array([[0., 64.]]))[0] == 7.5
    # a pilot that did not move takes the whole of the bounds; coinciding bounds stay empty
    mean, m2 = np.array([3., 3., 3.]), np.array([0., 4., 0.])
    flo, fhi = HO.freeze(mean, m2, 5, 6., np.array([1., 2.5, 3.]), np.array([9., 3.5, 3.]))
    assert flo.tolist() == [1., 2.5, 3.] and fhi.tolist() == [9., 3.5, 3.]
    masked = HO.freeze(np.ones((2, 2, 4)), np.ones((2, 2, 4)), 3, 1., np.zeros(4), np.full(4, 9.), np.array([[1, 0], [1, 1]]))
    assert np.isnan(masked[0][0, 1]).all() and np.isnan(masked[1][0, 1]).all() and not np.isnan(masked[0][1]).any()


def test_histograms_object_is_lazy_and_saves(tmp_path):
    rng = np.random.default_rng(9)
    x = synthetic("bimodal", 24 + 500, rng)
    L, U = np.full(4, -1e9), np.full(4, 1e9)
    lo, hi = HO.freeze(*HO.welford(x[:24]), 24, 6., L, U)
    bins, tails = HO.count(x[24:], lo, hi)
    r = np.stack((lo, hi), axis=-1)
    calls = dict(get=0, q=0)

    def get():
        calls["get"] += 1
        return bins, tails, r

    def quantiles(qs):
        calls["q"] += 1
        assert 1 <= len(qs) <= 8
        return (np.stack([HO.quantile(bins, tails, r, q) for q in qs], axis=-1), HO.mode(bins, tails, r),
                HO.outside(bins, tails, r))

    ph = posterior.PosteriorHistograms(500, get, quantiles, pilot=24, span=6.)
    assert calls == dict(get=0, q=0) and ph.count == 500
    med = ph.median
    assert med.shape == (2, 3, 4) and ph.mode.shape == (2, 3, 4) and calls["q"] == 1
    lo68, hi68 = ph.interval(0.68)
    assert (lo68 <= med).all() and (med <= hi68).all() and calls["q"] == 2
    ph.interval(0.68)
    assert calls["q"] == 2 and calls["get"] == 0
    assert ph.quantiles(np.linspace(0.05, 0.95, 11)).shape == (2, 3, 4, 11) and calls["q"] == 4
    assert (np.diff(ph.quantiles(np.linspace(0.05, 0.95, 11)), axis=-1) >= 0).all()
    assert ph.counts is bins and ph.tails is tails and ph.range is r and calls["get"] == 1
    # both modes were seen by the pilot: the fuller one (70 %, near 6 + k) is the mode
    assert (np.abs(ph.mode - (6. + np.arange(4))) < 0.5).all()
    for bad in (0., 1., -0.1, 1.5):
        with pytest.raises(ValueError):
            ph.quantiles([0.5, bad])
        with pytest.raises(ValueError):
            ph.interval(bad)
    with pytest.raises(ValueError):
        ph.quantiles([])
    ph.save(str(tmp_path / "run"))
    z = np.load(str(tmp_path / "run") + "_posterior_histograms.npz")
    assert int(z["count"]) == 500 and int(z["pilot"]) == 24 and float(z["span"]) == 6.
    np.testing.assert_array_equal(z["counts"], bins)
    np.testing.assert_array_equal(z["median"], med)
    np.testing.assert_array_equal(z["hi68"], hi68)
    pm = posterior.PosteriorMoments(0, lambda which: None)
    assert pm.histograms is None
