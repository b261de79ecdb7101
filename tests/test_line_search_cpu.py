"""
CPU tests (no GPU) of the matched-filter line search (deconv3d_amd/search.py, Run(initial_search=)):
keywords and conflicts are refused before any device work; the sub-grid refinement on hand-made
statistics; the CPU restatement of the statistic (tests/line_search_oracle.py) recovers planted
lines; the C entry point is declared, bound, and cites the reference lines it replaces.
"""
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, search
from oracle import deconv3d_oracle as O
from tests import line_search_oracle as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- refusals before device work ------------------------------------------------------

@pytest.mark.parametrize("kw, match", [
    (dict(centres=[0., 1., 3.]), "uniformly spaced"),
    (dict(centres=[3., 2., 1.]), "uniformly spaced"),
    (dict(centres=[]), "centres="),
    (dict(centres=[0., float("nan")]), "centres="),
    (dict(widths=[]), "widths="),
    (dict(widths=[1., 0.]), "widths="),
    (dict(widths=[-1.]), "widths="),
    (dict(widths=[float("inf")]), "widths="),
])
def test_bad_grids_are_refused_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        d3d.line_search(small_cube(), d3d.MUSE(), **kw)
    with pytest.raises(ValueError, match=match):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, initial_search=kw)
    with pytest.raises(ValueError, match=match):
        d3d.above_snr(small_cube(), d3d.MUSE(), **kw)


@pytest.mark.parametrize("kw", [dict(jitter=(0.5,)), dict(jitter=(-1., 0.1)), dict(jitter="ab"),
                                dict(jitter=(0.5, float("nan"))), dict(depth=3)])
def test_bad_initial_search_keys_are_refused(kw):
    with pytest.raises(ValueError, match="jitter|takes the keys"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, initial_search=kw)


def test_initial_search_conflicts_are_refused_before_any_device_work():
    with pytest.raises(ValueError, match="initial_search= and initial_parameters="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, initial_search=True,
                initial_parameters=np.array([1., 4., 1.]))
    with pytest.raises(ValueError, match="initial_search= with resume_state="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=4, initial_search=True,
                resume_state=dict(iteration=2))
    assert search.check_keywords(None) is None and search.check_keywords(False) is None
    cfg = search.check_keywords(True)
    assert cfg["centres"] is None and cfg["widths"] is None and cfg["jitter"] == (0.5, 0.1)


def test_default_grid():
    centres, widths, step = search.check_grid(None, None, 128)
    assert np.array_equal(centres, np.arange(128.)) and step == 1.
    assert widths.shape == (8,) and widths[0] == 0.75 and np.isclose(widths[-1], 128 / 6.)
    assert np.allclose(widths[1:] / widths[:-1], widths[1] / widths[0])
    assert np.isclose(search.default_widths(6)[-1], 1.5)
    for got, want in zip(LS.default_grid(21), search.check_grid(None, None, 21)):
        assert np.array_equal(got, want)


# ---- refinement ----------------------------------------------------------------------

CENTRES = np.array([10., 10.5, 11., 11.5])
WIDTHS = np.array([1., 2.])


def refine_one(k, N, Q, sm, sp, **kw):
    snr, p = search.refine(np.array([[k]]), np.array([[[N, Q, sm, sp]]]), CENTRES, WIDTHS, **kw)
    return snr[0, 0], p[0, 0]


def test_refinement_formula():
    # s0 = 8 / sqrt(4) = 4; neighbours 3 and 3.5: delta = 0.5 (3 - 3.5) / (3 - 8 + 3.5) = 1 / 6
    snr, p = refine_one(4 + 2, 8., 4., 3., 3.5)
    assert snr == 4.
    assert p[0] == 2. and p[2] == 2.
    assert np.isclose(p[1], 11. + 0.5 / 6., rtol=0, atol=1e-15)
    # symmetric neighbours: the grid point itself
    assert refine_one(1, 8., 4., 3., 3.)[1][1] == 10.5


def test_no_shift_at_the_grid_edge_or_with_positive_curvature():
    nan = float("nan")
    assert refine_one(0, 8., 4., nan, 3.5)[1][1] == 10.
    assert refine_one(3, 8., 4., 3.5, nan)[1][1] == 11.5
    assert refine_one(2, 8., 4., 5., 6.)[1][1] == 11.      # s- - 2 s0 + s+ = 3 > 0
    assert refine_one(2, 8., 4., 4., 4.)[1][1] == 11.      # flat: denominator 0


def test_shift_is_clipped_to_half_a_step():
    # delta = 0.5 (3.99 - 0) / (3.99 - 8 + 0) ~ -0.4975 -> inside; (0 - 3.999999) -> 0.49999..
    assert np.isclose(refine_one(2, 8., 4., 3.99, 0.)[1][1], 11. - 0.5 * 0.5 * 3.99 / 4.01)
    # a far lower neighbour on one side only: 0.5 (-100 - 3.9) / (-100 - 8 + 3.9) = 0.499 (inside);
    # neighbours ABOVE the peak on one side give |delta| > 1/2: clipped
    assert refine_one(2, 8., 4., 1., 6.9)[1][1] == 11. + 0.5 * 0.5      # delta = 0.5 (-5.9) / (-0.1) = 29.5
    assert refine_one(2, 8., 4., 6.9, 1.)[1][1] == 11. - 0.5 * 0.5


def test_parameters_are_clipped_to_the_bounds_and_undetected_spaxels_are_nan():
    snr, p = refine_one(3, 8., 4., 3., float("nan"), min_boundaries=[0., 0., 1.5],
                        max_boundaries=[1.5, 11.2, 9.])
    assert list(p) == [1.5, 11.2, 1.5] and snr == 4.
    snr, p = refine_one(-1, 0., 0., 0., 0.)
    assert np.isnan(snr) and np.isnan(p).all()
    res = search.LineSearch(np.array([[-1, 2]]), np.array([[[0., 0., 0., 0.], [8., 4., 3., 3.]]]),
                            CENTRES, WIDTHS)
    assert np.array_equal(res.mask(4.), [[0., 1.]]) and np.array_equal(res.mask(4.5), [[0., 0.]])
    assert np.array_equal(res.detected, [[False, True]])


def test_jittered_start_moves_c_and_w_only_and_stays_inside_the_bounds():
    p = np.tile(np.array([2., 10., 1.]), (6, 5, 1))
    lo, hi = np.array([0., 0., 0.]), np.array([5., 10.2, 3.])
    out = search.jittered_start(p, (0.5, 0.1), np.random.default_rng(3), lo, hi)
    assert np.array_equal(out[..., 0], p[..., 0])
    assert (out[..., 1] != 10.).all() and (out[..., 2] != 1.).all()
    assert (out >= lo).all() and (out <= hi).all() and (out[..., 1] == 10.2).any()
    assert np.array_equal(search.jittered_start(p, (0., 0.), np.random.default_rng(3), lo, hi), p)


def test_host_lsf_convolution_is_the_oracles():
    rng = np.random.default_rng(5)
    for D in (21, 32, 30):
        lines = rng.random((4, D))
        lsf = O.gaussian_lsf_vector(D, 1.3)
        want = np.array([O.convolve_1d_closed(row, lsf) for row in lines])
        np.testing.assert_allclose(search.lsf_convolve_rows(lines, lsf), want, rtol=0, atol=1e-15)
    assert search.lsf_convolve_rows(lines, None) is lines


# ---- the statistic recovers planted lines ----------------------------------------------

@pytest.mark.parametrize("shape, seed", [((32, 16, 16), 4242), ((21, 12, 10), 7), ((64, 20, 20), 3)])
def test_helper_recovers_planted_lines(shape, seed):
    D, H, W = shape
    fsf = O.gaussian_fsf_image(3.0)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, truth = O.synthetic_case(D, H, W, fsf, lsf, seed=seed)[:4]
    centres, widths = LS.default_grid(D)
    best, stat, gap = LS.statistic(data, var, mask, LS.template_bank(D, lsf, centres, widths),
                                   centres.size)
    res = search.LineSearch(best, stat, centres, widths)
    strong = res.snr >= 5.
    share = strong.mean()
    near = np.abs(centres[best[strong] % centres.size] - truth[..., 1][strong]) <= 1.
    print("%s seed %d: S/N >= 5 in %.1f %%, within one channel %.1f %%, gap %.2e"
          % (shape, seed, 100 * share, 100 * near.mean(), gap))
    assert share >= 0.5
    assert near.mean() >= 0.80
    assert gap >= 1e-8
    # the refined centre stays within half a step of the grid's
    assert np.all(np.abs(res.parameters[..., 1][strong] - centres[best[strong] % centres.size]) <= 0.5)


# ---- the symbol ------------------------------------------------------------------------

def test_entry_point_is_declared_bound_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    assert "d3d_line_search" in _lib.SYMBOLS and "d3d_line_search" in _lib.SEARCH_PROTOTYPES
    decl = text.index("int d3d_line_search(")
    comment = text[text.rindex("/*", 0, decl):decl]
    for lines in ("lib/run.py:310-314", "lib/masks.py:17-29"):
        assert lines in comment
    assert re.search(r"best_out\[", comment) and "centres" in comment
    assert hasattr(_lib.Engine, "line_search")
    for name in ("line_search", "LineSearch", "above_snr", "search"):
        assert hasattr(d3d, name)
    import __graft_entry__ as entry
    assert "d3d_search.hip" in entry.SOURCES
    makefile = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*d3d_search\.hip", makefile, re.M)
