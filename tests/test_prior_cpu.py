"""
CPU tests (no GPU) of the smoothness prior between neighbouring spaxels (Run(smoothness=...),
deconv3d_amd/prior.py, tests/prior_oracle.py): the keyword is validated, and a host-evaluated
model, a 1-wide FSF and a checkpoint written with other sigmas refused, before any device work;
the helper that restates the oracle's update with the prior is the oracle's without it; its
neighbour sets are right on a hand-made map; the C entry points are declared, bound, and cite the
reference lines they extend; and the prior does what it is for on the oracle.
"""
import math
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, prior
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import prior_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_prior_begin", "d3d_prior_get", "d3d_prior_end", "d3d_prior_energy")


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- keywords ------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [
    dict(c=-1.), dict(c=0.), dict(a=float("nan")), dict(w=-0.5, c=1.), dict(c="wide"), dict(c=True),
    dict(v=1.), dict(c=1., sigma=2.), (1., 2.), (1., 2., 3., 4.), (1., -2., 3.), (1., float("nan"), 3.),
    1.0, "1,1,1",
])
def test_run_refuses_bad_keywords_before_any_device_work(value):
    with pytest.raises(ValueError, match="smoothness"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, smoothness=value)


def test_keywords_become_sigmas_and_weights():
    assert prior.check_keywords(None) is None
    assert prior.check_keywords(dict(c=1.)) == (math.inf, 1., math.inf)
    assert prior.check_keywords(dict(a=None, c=0.5, w=float("inf"))) == (math.inf, 0.5, math.inf)
    assert prior.check_keywords((2., None, 0.25)) == (2., math.inf, 0.25)
    assert prior.check_keywords(np.array([2., 4., 0.5])) == (2., 4., 0.5)
    assert prior.check_keywords({}) == (math.inf,) * 3
    np.testing.assert_array_equal(prior.lam_of((2., math.inf, 0.25)), [0.25, 0., 16.])
    np.testing.assert_array_equal(prior.keyword_record((2., math.inf, 0.25)), [2., math.inf, 0.25])
    assert prior.NAMES == ("a", "c", "w")


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="smoothness=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, smoothness=dict(c=1.))


@pytest.mark.parametrize("shape", [(1, 3), (3, 1), (1, 1)])
def test_run_refuses_an_fsf_one_spaxel_wide(shape):
    """Adjacent spaxels would share a colour class: refused, never sampled wrongly."""
    fsf = np.ones(shape) / (shape[0] * shape[1])
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(O.gaussian_lsf_vector(8, 0.9)),
                          fsf=ImageFieldSpreadFunction(fsf))
    with pytest.raises(ValueError, match="smoothness= with a %d x %d FSF" % shape):
        d3d.Run(small_cube(), inst, max_iterations=40, smoothness=dict(c=1.))
    with pytest.raises(ValueError, match="FSF"):
        prior.check_fsf((1., 1., 1.), shape)
    prior.check_fsf(None, shape)
    prior.check_fsf((1., 1., 1.), (3, 3))


def state_of(sigmas=None):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=1)
    if sigmas is not None:
        state["smoothness_sigmas"] = prior.keyword_record(sigmas)
    return state


@pytest.mark.parametrize("saved, kw, what", [
    ((math.inf, 1., math.inf), dict(smoothness=dict(c=0.5)), r"smoothness=\(inf, 1, inf\).*smoothness=\(inf, 0.5, inf\)"),
    ((math.inf, 1., math.inf), dict(smoothness=dict(c=1., w=2.)), "this run has smoothness="),
    ((math.inf, 1., math.inf), dict(), "this run has none"),
    (None, dict(smoothness=dict(c=1.)), "written without smoothness="),
])
def test_run_refuses_a_state_written_with_other_sigmas(saved, kw, what):
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(saved), **kw)


def test_resume_accepts_the_same_sigmas():
    s = prior.check_keywords(dict(c=1., a=3.))
    state = state_of(s)
    prior.check_resume(state, state, s)
    prior.check_resume(state_of(), state_of(), None)


# ---- the C ABI ------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("smoothness prior between neighbouring spaxels"):text.index("spatial tiling")]
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.PRIOR_PROTOTYPES
        decl = section.index("int %s(" % name)
        comment = section[section.rindex("/*", 0, decl):decl]
        assert re.search(r"lib/run\.py:\d+", comment), name
    for lines in ("lib/run.py:426-438", "lib/run.py:491-496"):
        assert lines in section
    for name in ("prior_begin", "prior_get", "prior_end", "prior_energy"):
        assert callable(getattr(_lib.Engine, name))
    assert callable(d3d.Run.roughness)


# ---- the helper -----------------------------------------------------------------------------

def tiny_state(seed=3, mask=None):
    D, H, W = 12, 6, 7
    fsf = np.outer([0.2, 0.5, 0.3], [0.25, 0.5, 0.25])
    lsf = O.gaussian_lsf_vector(D, 0.9)
    data, var, m, truth, init, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=seed)
    if mask is not None:
        m = mask
    return lambda: O.MHState(data, var, m, fsf, lsf, init, min_b, max_b, seed=11)


def test_without_weights_the_helper_is_the_oracle_exactly():
    mask = np.ones((6, 7))
    mask[2, 3] = mask[5, 0] = 0
    make = tiny_state(mask=mask)
    a, b = make(), make()
    for s in (1, 2, 3):
        O.mh_sweep(a, s)
        PO.mh_sweep(b, s, (0., 0., 0.))
        np.testing.assert_array_equal(a.params, b.params)
        np.testing.assert_array_equal(a.err, b.err)
        np.testing.assert_array_equal(a.dlog, b.dlog)
        assert a.accepted == b.accepted
    c = make()
    PO.mh_sweep(c, 1, (0.5, 2., 3.))
    d = make()
    O.mh_sweep(d, 1)
    assert not np.array_equal(c.params, d.params)      # (and with weights it is another chain)


def test_neighbour_sets_and_energy_of_a_hand_made_map():
    """3 x 3, mask
           1 1 0
           1 1 1
           0 1 0     and, second mask, the centre alone."""
    mask = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 0]])
    assert PO.neighbours(mask, 0, 0) == [(1, 0), (0, 1)]                      # a corner
    assert PO.neighbours(mask, 0, 1) == [(1, 1), (0, 0)]                      # an edge, one neighbour masked
    assert PO.neighbours(mask, 1, 1) == [(0, 1), (2, 1), (1, 0), (1, 2)]      # all four
    assert PO.neighbours(mask, 1, 2) == [(1, 1)]                              # masked above and below
    assert PO.neighbours(mask, 2, 1) == [(1, 1)]
    alone = np.zeros((3, 3))
    alone[1, 1] = 1
    assert PO.neighbours(alone, 1, 1) == []                                   # isolated
    p = np.zeros((3, 3, 3))
    p[..., 0] = [[1., 2., 100.], [4., 8., 16.], [100., 32., 100.]]
    p[..., 1] = 2. * p[..., 0]
    p[..., 2] = -p[..., 0]
    # pairs: (0,0)-(0,1) 1, (1,0)-(1,1) 16, (1,1)-(1,2) 64, (0,0)-(1,0) 9, (0,1)-(1,1) 36, (1,1)-(2,1) 576
    assert PO.energy(p, mask) == (702., 4. * 702., 702., 6)
    assert PO.energy(p, alone) == (0., 0., 0., 0)
    assert PO.energy(p[:1, :1], np.ones((1, 1))) == (0., 0., 0., 0)
    assert PO.energy(p[:1], np.ones((1, 3))) == (1. + 98. ** 2, 4. * (1. + 98. ** 2), 1. + 98. ** 2, 2)


def test_the_update_uses_the_neighbours_as_they_are_when_it_is_decided():
    """One update with a neighbour changed just before it: delta and the amplitude follow the
    changed value (the log ratio moves by the prior's term exactly as the formula says)."""
    make = tiny_state()
    lam = np.array([0.7, 2., 3.])
    a, b = make(), make()
    y, x = 2, 3
    b.params[y, x + 1, 1] += 0.25            # (residual left alone: only the prior sees it)
    PO.mh_update(a, y, x, 1, lam)
    PO.mh_update(b, y, x, 1, lam)
    plain = make()
    O.mh_update(plain, y, x, 1)
    u = np.array(O.philox_pair(11, y * 7 + x, 1, O.BLK_JUMP_AC) + O.philox_pair(11, y * 7 + x, 1, O.BLK_JUMP_W))
    p_old = plain.last[0]
    p_new = p_old + plain.amp * np.tan(np.pi * (u[:3] - 0.5))
    for st in (a, b):
        want = 0.
        for ny, nx in PO.neighbours(st.mask, y, x):
            theta = make().params[ny, nx].copy()
            if st is b and (ny, nx) == (y, x + 1):
                theta[1] += 0.25
            for k in (1, 2):
                want += lam[k] * (p_new[k] - p_old[k]) * (p_new[k] + p_old[k] - 2. * theta[k])
        assert st.dlog[y, x] == pytest.approx(plain.dlog[y, x] - 0.5 * want, rel=1e-12, abs=1e-12)
    assert a.dlog[y, x] != b.dlog[y, x]


# ---- does it help? ----------------------------------------------------------------------------

def test_the_prior_halves_the_error_of_the_centre_map_on_the_oracle():
    """oracle.synthetic_case(32, 12, 12), Gaussian FSF FWHM 3 (9 x 9), LSF sigma 0.9088, started at
    the truth, 160 sweeps in colour order, mean of sweeps 60 .. 159, seed 12345: the rms error of
    the mean c map over all 144 spaxels is 4.07 without a prior and 0.50 with sigma_c = 1."""
    D, H, W = 32, 12, 12
    fsf = O.gaussian_fsf_image(3.0)
    lsf = O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, truth, _, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=12345)
    rms = {}
    for name, lam in (("none", (0., 0., 0.)), ("sigma_c = 1", (0., 1., 0.))):
        st = O.MHState(data, var, mask, fsf, lsf, truth, min_b, max_b, seed=12345)
        mean = np.zeros((H, W))
        for s in range(160):
            PO.mh_sweep(st, s, lam)
            if s >= 60:
                mean += st.params[..., 1] / 100.
        rms[name] = float(np.sqrt(np.mean((mean - truth[..., 1]) ** 2)))
    print("rms error of the mean c map: without %.3f, with sigma_c = 1 %.3f" % (rms["none"], rms["sigma_c = 1"]))
    assert rms["sigma_c = 1"] < 0.5 * rms["none"]
