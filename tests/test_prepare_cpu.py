"""
CPU tests (no GPU) of the cube preparation (deconv3d_amd/prepare.py, Run(prepare=),
line_search(prepare=)): shapes, types and ranges are refused before any device work; the numpy
restatement of the contract (tests/prepare_oracle.py) on hand-made spectra; on the planted raw
cube the preparation brings the matched filter back and the rejection pass improves the
continuum; the C entry points are declared, bound, and cite the reference lines they replace.
"""
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, prepare, search
from tests import line_search_oracle as LS
from tests import prepare_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- refusals before device work ------------------------------------------------------

@pytest.mark.parametrize("kw, match", [
    (dict(continuum_window=50), "continuum_window="),
    (dict(continuum_window=1), "continuum_window="),
    (dict(continuum_window=259), "continuum_window="),
    (dict(continuum_window=5.5), "continuum_window="),
    (dict(continuum_window="wide"), "continuum_window="),
    (dict(reject=0.), "reject="),
    (dict(reject=-3.), "reject="),
    (dict(reject=NAN), "reject="),
    (dict(reject="three"), "reject="),
    (dict(rescale=1), "rescale="),
    (dict(rescale=True), "needs the variance="),
    (dict(noise_mask=np.ones((9, 8))), "noise_mask MUST have"),
    (dict(noise_mask=np.zeros((9, 9))), "selects no spaxel"),
])
def test_bad_settings_are_refused_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        d3d.prepare_cube(small_cube(), **kw)
    with pytest.raises(ValueError, match=match):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, prepare=kw)
    with pytest.raises(ValueError, match=match):
        d3d.line_search(small_cube(), d3d.MUSE(), prepare=kw)


def test_bad_cubes_variances_and_keys_are_refused_before_any_device_work():
    with pytest.raises(ValueError, match="three axes"):
        d3d.prepare_cube(np.ones((8, 9)))
    with pytest.raises(TypeError, match="real numbers"):
        d3d.prepare_cube(np.ones((8, 9, 9), dtype=complex))
    with pytest.raises(TypeError, match="HyperspectralCube"):
        d3d.prepare_cube([[1., 2.]])
    with pytest.raises(ValueError, match="correct shape"):
        d3d.prepare_cube(small_cube(), variance=np.ones((8, 9, 8)), rescale=True)
    with pytest.raises(TypeError, match="variance"):
        d3d.prepare_cube(small_cube(), variance=[1.], rescale=True)
    with pytest.raises(ValueError, match="takes the keys"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, prepare=dict(window=5))
    with pytest.raises(ValueError, match="True or a dict"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, prepare=51)
    assert prepare.check_keywords(None) is None and prepare.check_keywords(False) is None
    assert prepare.check_keywords(True) == dict(continuum_window=51, reject=3.0, noise_mask=None,
                                                rescale=False)
    assert prepare.check_keywords(dict(reject=None, continuum_window=np.int64(7)))["reject"] is None


def test_resume_refuses_other_settings():
    a = dict(continuum_window=51, reject=3.0, rescale=False, noise_spaxels=-1)
    state = dict(prepare_settings=prepare.settings_record(a))
    prepare.check_resume(state, state, dict(a))
    prepare.check_resume({}, {}, None)
    none = dict(a, reject=None)
    state_none = dict(prepare_settings=prepare.settings_record(none))
    prepare.check_resume(state_none, state_none, none)           # (NaN = no rejection compares equal)
    for other in (dict(a, continuum_window=31), dict(a, reject=2.5), none, dict(a, rescale=True),
                  dict(a, noise_spaxels=40), None):
        with pytest.raises(ValueError, match="preparation settings"):
            prepare.check_resume(state, state, other)
    with pytest.raises(ValueError, match="preparation settings"):
        prepare.check_resume({}, {}, a)


# ---- the oracle on hand-made spectra -----------------------------------------------------

def spectrum(values):
    return np.array(values, dtype=np.float64).reshape(-1, 1, 1)


def test_running_median_even_window_with_ties_and_edges():
    got = P.running_median(spectrum([3., 1., 1., 2., 5., 5.]), None, 1)[:, 0, 0]
    # windows {3,1} {3,1,1} {1,1,2} {1,2,5} {2,5,5} {5,5}
    assert np.array_equal(got, [2., 1., 1., 2., 5., 5.])
    # an invalid voxel leaves an even window: {3,1} {3,1} {1,2} {2,5} {2,5,5} {5,5}
    valid = spectrum([1, 1, 0, 1, 1, 1])
    got = P.running_median(spectrum([3., 1., 1., 2., 5., 5.]), valid, 1)[:, 0, 0]
    assert np.array_equal(got, [2., 2., 1.5, 3.5, 5., 5.])
    # h >= D: the whole spectrum from every channel
    assert np.array_equal(P.running_median(spectrum([4., 0., 1., 9.]), None, 7)[:, 0, 0], [2.5] * 4)


def test_running_median_skips_nan_and_inf_and_gives_nan_for_an_empty_window():
    inf = float("inf")
    got = P.running_median(spectrum([NAN, NAN, NAN, 1., inf, 7., -inf]), None, 1)[:, 0, 0]
    # windows {} {} {1} {1} {1,7} {7} {7}: defined at invalid voxels too
    assert np.array_equal(got, [NAN, NAN, 1., 1., 4., 7., 7.], equal_nan=True)


def test_channel_stats_by_hand():
    cube = np.array([[[1., 2.], [4., 100.]],          # n = 4: m = 3, |x - m| = 2 1 1 97: mad 1.5
                     [[5., NAN], [5., 5.]],           # n = 3: m = 5, mad 0
                     [[NAN, NAN], [NAN, float("inf")]],  # n = 0
                     [[7., 1.], [2., 3.]]])           # select keeps 7 and 3: m = 5, mad 2
    m, mad, n = P.channel_stats(cube[:3])
    assert np.array_equal(n, [4, 3, 0])
    assert np.array_equal(m, [3., 5., NAN], equal_nan=True)
    assert np.array_equal(mad, [1.5, 0., NAN], equal_nan=True)
    assert np.array_equal(P.sigma_of(mad, n), [1.4826 * 1.5, NAN, NAN], equal_nan=True)
    m, mad, n = P.channel_stats(cube[3:], np.array([[1, 0], [0, 2]]))
    assert (m[0], mad[0], n[0]) == (5., 2., 2)
    assert np.isnan(P.sigma_of(np.array([2.]), np.array([1])))[0]       # n < 2


def test_variance_step():
    sigma = np.array([2., NAN, 3.])
    v = P.variance(sigma, (3, 2, 2))
    assert np.array_equal(v[:, 0, 0], [4., 1e12, 9.]) and v.shape == (3, 2, 2)
    assert np.array_equal(prepare.channel_variance(sigma, (3, 2, 2)), v)
    given = np.arange(1., 13.).reshape(3, 2, 2)
    given[2] = 0.                                    # a zero median: the channel stays
    got = P.variance(sigma, (3, 2, 2), given)
    assert np.array_equal(got[0], given[0] * 4. / 2.5)
    assert np.array_equal(got[1:], given[1:])
    medians = P.channel_stats(given)[0]
    assert np.array_equal(prepare.channel_variance(sigma, (3, 2, 2), given, medians), got)


# ---- the planted raw cube ----------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    pl = P.Planted()
    centres, widths = LS.default_grid(pl.shape[0])
    bank = LS.template_bank(pl.shape[0], pl.lsf, centres, widths)

    def share(data, var):
        """spaxels the matched filter detects at S/N >= 5 within one channel of the truth"""
        best, stat, _ = LS.statistic(data, var, pl.mask, bank, centres.size)
        res = search.LineSearch(best, stat, centres, widths)
        c = centres[np.where(best >= 0, best, 0) % centres.size]
        with np.errstate(invalid="ignore"):
            return float(((res.snr >= 5.) & (np.abs(c - pl.truth[..., 1]) <= 1.)).mean())

    out = {}
    for reject in (3.0, None):
        cont, res, m, sigma, n = P.prepare(pl.raw, pl.noise_mask, 25, reject)
        out[reject] = dict(cont=cont, res=res, sigma=sigma, n=n,
                           share=share(res, P.variance(sigma, pl.shape)),
                           rms=float(np.sqrt(np.nanmean(((cont - pl.continuum) / pl.sigma[:, None, None]) ** 2))))
    out["raw"] = share(pl.raw, pl.true_variance)
    out["clean"] = share(pl.line_cube, pl.true_variance)
    return pl, out


def test_preparation_brings_the_matched_filter_back(planted):
    pl, out = planted
    print("within one channel at S/N >= 5: raw cube, true variance %.3f; prepared cube, estimated variance "
          "%.3f (reject=3) %.3f (reject=None); continuum-free cube, true variance %.3f"
          % (out["raw"], out[3.0]["share"], out[None]["share"], out["clean"]))
    assert out[3.0]["share"] > out["raw"]
    assert out[None]["share"] > out["raw"]


def test_rejection_pass_improves_the_continuum(planted):
    pl, out = planted
    print("rms continuum error in sigma: reject=3 %.3f, reject=None %.3f" % (out[3.0]["rms"], out[None]["rms"]))
    assert out[3.0]["rms"] < out[None]["rms"]


def test_planted_cube_edge_cases(planted):
    pl, out = planted
    r = out[3.0]
    assert np.isnan(r["cont"][:, 0, 0]).all() and np.isnan(r["res"][:, 0, 0]).all()
    z, y, x = pl.shape[0] // 3, pl.shape[1] // 2, pl.shape[2] // 2 + 1
    assert np.isfinite(r["cont"][z, y, x]) and np.isnan(r["res"][z, y, x])
    assert np.isfinite(r["sigma"]).all() and (r["n"] <= pl.noise_mask.sum()).all()
    ratio = np.median(r["sigma"] / pl.sigma)
    print("estimated / true channel sigma, median: %.3f" % ratio)


# ---- the symbols -------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    names = ("d3d_running_median", "d3d_channel_stats", "d3d_prepare")
    for name in names:
        assert name in _lib.SYMBOLS and name in _lib.PREP_PROTOTYPES
    decl = text.index("int d3d_running_median(")
    comment = text[text.rindex("/*", 0, decl):decl]
    for cited in ("lib/run.py:171-192", "lib/run.py:180", "half_window", "1.4826", "nanmedian"):
        assert cited in comment
    for name in names[1:]:
        assert text.index("int %s(" % name) > decl
    for name in ("running_median", "channel_stats", "prepare"):
        assert hasattr(_lib.Engine, name)
    for name in ("prepare_cube", "Prepared", "prepare"):
        assert hasattr(d3d, name)
    import __graft_entry__ as entry
    assert "d3d_prep.hip" in entry.SOURCES
    makefile = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*d3d_prep\.hip", makefile, re.M)
