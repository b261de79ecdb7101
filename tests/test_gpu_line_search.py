"""
GPU tests of the matched-filter line search (d3d_line_search, deconv3d_amd/search.py,
Run(initial_search=), masks.above_snr) against its CPU restatement (tests/line_search_oracle.py).

Tolerances: N_best and Q_best relative 1e-10 -- the project's tolerance for window sums
 --, the two neighbour statistics 1e-10 of s_best, ``best`` equal exactly.  The last
is legitimate only where the helper's best and second-best candidates are further apart than the
two implementations can differ: every comparison first asserts that the smallest relative gap
of any spaxel is at least GAP_MIN = 1e-7, a thousand times the 1e-10 to which the statistics
agree (measured on the CPU: 4e-6 or more on every case below).
"""
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, search
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import line_search_oracle as LS

pytestmark = pytest.mark.gpu

GAP_MIN = 1e-7
DOUBLET = ([0., 3.2], [1., 0.6])


@functools.lru_cache(maxsize=None)
def case(name):
    """(data, var, mask, fsf, lsf, centres, widths, model) of one comparison; never modified."""
    model = None
    if name in ("c1", "half", "doublet"):
        D, H, W, seed = 32, 16, 16, 4242
    elif name == "odd":              # odd depth (pad channel), non-power-of-two (partial-wrap LSF),
        D, H, W, seed = 21, 13, 11, 7   # 143 spaxels: no multiple of 8, 4 or 2
    elif name == "dirty":
        D, H, W, seed = 64, 20, 20, 3
    elif name == "nolsf":
        D, H, W, seed = 24, 8, 9, 11
    elif name == "deep":             # beyond 1024 channels: two spaxels per workgroup
        D, H, W, seed = 1030, 3, 3, 5
    else:
        raise KeyError(name)
    fsf = O.gaussian_fsf_image(3.0)
    lsf = None if name == "nolsf" else O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask = O.synthetic_case(D, H, W, fsf, lsf, seed=seed)[:3]
    centres, widths = LS.default_grid(D)
    if name == "odd":                # 3 x 21 = 63 candidates: less than a wavefront
        widths = np.geomspace(0.75, 3.5, 3)
    elif name == "half":             # half-channel grid: 63 x 8 = 504 candidates
        centres = np.arange(0., D - 0.75, 0.5)
    elif name == "doublet":
        model = d3d.GaussianMultipletLineModel(*DOUBLET)
    elif name == "deep":             # 40 channels around the planted lines of the columns 0 and 1
        centres = np.arange(380., 420.)
    elif name == "dirty":
        data, var, mask = data.copy(), var.copy(), mask.copy()
        data[5, 3, 4] = data[40:44, 9, 2] = data[63, 19, 19] = np.nan    # NaN voxels
        data[:, 7, 7] = np.nan                                        # an all-NaN spectrum
        var[10, 2, 2] = var[30:34, 12, 5] = 0.                        # zero variances
        mask[10:14, 10:15] = 0                                        # a masked block
    for a in (data, var, mask, centres, widths):
        a.setflags(write=False)
    return data, var, mask, fsf, lsf, centres, widths, model


@functools.lru_cache(maxsize=None)
def reference(name):
    """(best, stat, gap, bank) of the helper, computed once per case."""
    data, var, mask, fsf, lsf, centres, widths, model = case(name)
    bank = LS.template_bank(data.shape[0], lsf, centres, widths, model)
    return LS.statistic(data, var, mask, bank, centres.size) + (bank,)


def engine_for(name):
    data, var, mask, fsf, lsf, centres, widths, model = case(name)
    eng = _lib.Engine(data.shape, fsf.shape)
    eng.set_taps(fsf, lsf)
    eng.set_data(data, var, mask=mask)
    if model is not None:
        eng.set_line_shape(model.offsets, model.ratios)
    return eng


def assert_matches_helper(name, best, stat):
    want_best, want_stat, gap, _ = reference(name)
    print("%s: smallest best / second-best gap %.3e, %d of %d detected"
          % (name, gap, int((want_best >= 0).sum()), want_best.size))
    assert gap >= GAP_MIN
    np.testing.assert_array_equal(best, want_best)
    det = want_best >= 0
    assert det.any()
    assert (stat[~det] == 0.).all()
    np.testing.assert_allclose(stat[det][:, :2], want_stat[det][:, :2], rtol=1e-10, atol=0.)
    s_best = want_stat[det][:, 0] / np.sqrt(want_stat[det][:, 1])
    for q in (2, 3):
        got, want = stat[det][:, q], want_stat[det][:, q]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-10 * s_best[ok])


@pytest.mark.parametrize("name", ["c1", "odd", "dirty", "nolsf", "doublet", "half", "deep"])
def test_device_statistic_is_the_helpers(name):
    centres, widths = case(name)[5:7]
    with engine_for(name) as eng:
        best, stat = eng.line_search(centres, widths)
    assert best.dtype == np.int32
    assert_matches_helper(name, best, stat)


def test_dirty_case_has_what_it_is_about():
    data, var, mask = case("dirty")[:3]
    best = reference("dirty")[0]
    assert best[7, 7] == -1                          # all-NaN: Q = 0 for every candidate
    assert (best[10:14, 10:15] == -1).all()          # masked
    assert best[3, 4] >= 0 and best[9, 2] >= 0       # NaN voxels only lose their weight
    assert best[2, 2] >= 0


def test_a_host_bank_of_the_helpers_templates_gives_the_helpers_answer():
    # (odd depth: rows of D channels into rows of D + 1)
    centres, widths = case("odd")[5:7]
    with engine_for("odd") as eng:
        best, stat = eng.line_search(centres, widths, bank=reference("odd")[3])
    assert_matches_helper("odd", best, stat)


def test_a_host_bank_equal_to_the_devices_gives_identical_outputs():
    data, var, mask, fsf, lsf, centres, widths, _ = case("nolsf")
    D = data.shape[0]
    rows = np.ones((widths.size, centres.size, 3))
    rows[..., 1] = centres[None, :]
    rows[..., 2] = widths[:, None]
    # the device's own lines of these (1, c, w) rows: without an LSF the bank is the clean line cube
    with _lib.Engine((D, widths.size, centres.size), fsf.shape) as liner:
        liner.set_taps(fsf, None)
        liner.set_data(np.zeros((D, widths.size, centres.size)))
        bank = liner.simulate(rows, convolved=False).reshape(D, -1).T.copy()
    with engine_for("nolsf") as eng:
        best, stat = eng.line_search(centres, widths)
        best_b, stat_b = eng.line_search(centres, widths, bank=bank)
    np.testing.assert_array_equal(best_b, best)
    assert stat_b.tobytes() == stat.tobytes()
    assert (best >= 0).any()


def test_refusals():
    data, var, mask, fsf, lsf, centres, widths, _ = case("c1")
    with _lib.Engine(data.shape, fsf.shape) as eng:
        with pytest.raises(RuntimeError, match="taps/data not set"):
            eng.line_search(centres, widths)
        eng.set_taps(fsf, lsf)
        with pytest.raises(RuntimeError, match="taps/data not set"):
            eng.line_search(centres, widths)
    with engine_for("c1") as eng:
        # 8 widths x 131073 centres x 32 channels x 8 bytes: one row above 256 MiB
        with pytest.raises(NotImplementedError, match="centres"):
            eng.line_search(np.arange(131073) * 1e-4, widths)
        with pytest.raises(ValueError, match="widths"):
            eng.line_search(centres, [1., -2.])
        with pytest.raises(ValueError):
            eng.line_search(centres, [])
        best, _ = eng.line_search(centres, widths)      # (the context is still good)
        np.testing.assert_array_equal(best, reference("c1")[0])
    with _lib.Engine(data.shape, fsf.shape) as eng:
        eng.set_tile(0, 0, data.shape[2], 0, data.shape[1], 0, data.shape[2])
        eng.set_taps(fsf, lsf)
        eng.set_data(data, var, mask=mask)
        with pytest.raises(NotImplementedError, match="tile"):
            eng.line_search(centres, widths)


def test_a_search_writes_none_of_the_chains_state():
    data, var, mask, fsf, lsf, centres, widths, _ = case("c1")
    init, min_b, max_b = O.synthetic_case(32, 16, 16, fsf, lsf, seed=4242)[4:]
    out = []
    for searched in (False, True, True):
        with engine_for("c1") as eng:
            eng.set_params(init)
            eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=31, refresh_every=0)
            eng.residual(fetch=False)
            eng.mh_sweeps(1, 1)
            if searched:                                # (between sweeps: pending updates in flight)
                eng.line_search(centres, widths)
            eng.mh_sweeps(2, 2)
            out.append((eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog()))
    for got in out[1:]:
        for a, b in zip(got, out[0]):
            assert a.tobytes() == b.tobytes()


# ---- end to end ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def run_inputs():
    data, var, mask, fsf, lsf = case("c1")[:5]
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    return inst, d3d.MUSE().build_cube(np.array(data)), np.array(var)


def test_run_starts_chain_0_from_the_searched_map():
    inst, cube, var = run_inputs()
    run = d3d.Run(cube, inst, variance=var, max_iterations=1, seed=3, initial_search=True)
    plain = d3d.Run(cube, inst, variance=var, max_iterations=1, seed=3)
    assert plain.search is None
    found = run.search.detected
    np.testing.assert_array_equal(run.search.best_index, reference("c1")[0])
    assert found.sum() > 200
    np.testing.assert_array_equal(run.chain[0][found], run.search.parameters[found])
    np.testing.assert_array_equal(run.chain[0][~found], plain.chain[0][~found])
    assert (run.chain[0] >= run.min_boundaries).all() and (run.chain[0] <= run.max_boundaries).all()


def test_chains_start_dispersed_around_the_searched_map():
    inst, cube, var = run_inputs()
    run = d3d.Run(cube, inst, variance=var, max_iterations=1, seed=3, chains=3,
                  initial_search=dict(jitter=(0.5, 0.1)))
    found = run.search.detected
    np.testing.assert_array_equal(run.chains[0][0][found], run.search.parameters[found])
    for r in (1, 2):
        start = run.chains[r][0]
        assert (start >= run.min_boundaries).all() and (start <= run.max_boundaries).all()
        np.testing.assert_array_equal(start[found][:, 0], run.chains[0][0][found][:, 0])
        inside = found & (run.search.parameters[..., 1] > 1.) & (run.search.parameters[..., 1] < 30.)
        assert (start[inside][:, 1:] != run.chains[0][0][inside][:, 1:]).all()
        assert np.abs(start[inside][:, 1] - run.chains[0][0][inside][:, 1]).max() < 0.5 * 6
    assert not np.array_equal(run.chains[1][0], run.chains[2][0])


def test_above_snr_is_the_searchs_mask():
    inst, cube, var = run_inputs()
    res = d3d.line_search(cube, inst, variance=var)
    assert_matches_helper("c1", res.best_index, res.stat)
    for thr in (5., 8.):
        got = d3d.above_snr(cube, inst, threshold=thr, variance=var)
        np.testing.assert_array_equal(got, res.mask(thr))
        assert set(np.unique(got)) == {0., 1.}
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.mask(5.) == 1., res.snr >= 5.)


def test_a_searched_start_fits_better_after_20_sweeps_than_a_uniform_one():
    inst, cube, var = run_inputs()
    kw = dict(variance=var, max_iterations=21, seed=3, min_acceptance_rate=0.)
    searched = d3d.Run(cube, inst, initial_search=True, **kw)
    uniform = d3d.Run(cube, inst, **kw)
    chi2_s, chi2_u = searched.engine.chi2_map()[1], uniform.engine.chi2_map()[1]
    print("half chi2 after 20 sweeps: searched start %.6g, uniform start %.6g" % (chi2_s, chi2_u))
    assert chi2_s < chi2_u
