"""
CPU tests (no GPU) of the Student-t likelihood (Run(robust=...), deconv3d_amd/robust.py,
tests/robust_oracle.py): the oracle's draw has the Gamma distribution it claims and the weight mean
the formula gives; its array Philox is the oracle's; the keyword is validated, and tempering=, a
host-evaluated model and a checkpoint written with other values are refused, before any device
work; the C entry points are declared, bound, built and cite the reference lines they extend.
"""
import os
import re

import numpy as np
import pytest
from scipy import stats

import deconv3d_amd as d3d
from deconv3d_amd import _lib, robust
from oracle import deconv3d_oracle as O
from tests import robust_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_robust_begin", "d3d_robust_step", "d3d_robust_get", "d3d_robust_end")
N_DRAWS = 20000


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


# ---- the draw -------------------------------------------------------------------------------

def test_array_philox_is_the_oracles():
    voxels = np.array([0, 1, 77, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.uint64)
    for seed, sweep, block in ((12345, 1, 0), (2 ** 40 + 3, 2 ** 31 + 7, 3)):
        ux, uy = RO.philox_pairs(seed, voxels, sweep, block)
        for i, v in enumerate(voxels):
            r = O.philox4x32_10((int(v), sweep, block, RO.TAG), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
            assert ux[i] == O.u64_to_unit((r[1] << 32) | r[0])
            assert uy[i] == O.u64_to_unit((r[3] << 32) | r[2])
    # (the sweep's own blocks have 0 in the fourth word: another stream)
    assert RO.TAG != 0
    assert RO.philox_pairs(12345, voxels[:1], 1, 0)[0][0] != O.philox_pair(12345, 0, 1, 0)[0]


@pytest.mark.parametrize("nu", [1, 2, 3, 4, 9, 30])
def test_the_draw_is_a_gamma_of_shape_half_nu_plus_one(nu):
    us = RO.uniforms(99, np.arange(N_DRAWS, dtype=np.uint64), 5, RO.n_uniforms(nu))
    assert len(us) == (nu + 1) // 2 + (2 if nu % 2 == 0 else 0)
    g = RO.gamma_draw(nu, us)
    ks = stats.kstest(g, stats.gamma((nu + 1) / 2.).cdf)
    print("nu", nu, ks)
    assert ks.pvalue > 1e-3, (nu, ks)        # the threshold of tests/test_gpu_rtnorm.py


@pytest.mark.parametrize("nu, r, i0", [(1, 0., 1.), (3, 2.5, 4.), (4, 50., 1.), (8, 0.3, 0.01), (30, 7., 2.)])
def test_the_mean_weight_at_a_fixed_residual(nu, r, i0):
    """E[lambda | r] = (nu + 1) / (nu + r^2 i0), within 4 standard errors of 20 000 draws (the
    variance of a Gamma(k, rate b) is k / b^2)."""
    err = np.full((N_DRAWS, 1, 1), r)
    lam = RO.draw_weights(7, 3, nu, err, np.full(err.shape, i0))
    rate = (nu + r * r * i0) / 2.
    want, se = (nu + 1) / 2. / rate, np.sqrt((nu + 1) / 2.) / rate / np.sqrt(N_DRAWS)
    print("nu", nu, "mean", lam.mean(), "want", want, "se", se)
    assert abs(lam.mean() - want) <= 4. * se


def test_base_ivar_and_the_chains_mean():
    data = np.ones((2, 2, 2))
    data[0, 0, 0] = np.nan
    var = np.full((2, 2, 2), 4.)
    var[1, 1, 1] = 0.
    i0 = RO.base_ivar(data, var)
    assert i0[0, 0, 0] == 0. and i0[1, 1, 1] == 1e-12 and i0[0, 1, 1] == 0.25

    class State(object):            # what RobustChain.reweight reads of an O.MHState
        seed = 5
    st = State()
    st.data, st.var = data, var
    st.err = np.random.default_rng(2).normal(0., 3., data.shape)
    chain = RO.RobustChain(st, 2, accumulate_from=4)
    draws = []
    for s in (3, 4, 5, 6):
        ivar = chain.reweight(s)
        lam = RO.draw_weights(5, s, 2, st.err, i0)
        np.testing.assert_array_equal(chain.weights, lam)
        assert ivar[0, 0, 0] == 0. and np.isinf(st.var[0, 0, 0])
        np.testing.assert_array_equal(ivar[i0 != 0.], (lam * i0)[i0 != 0.])
        if s >= 4:
            draws.append(lam)
    assert chain.count == 3                                         # sweep 3 lies before accumulate_from
    live = i0 != 0.
    np.testing.assert_allclose(chain.weight_mean()[live], np.mean(draws, axis=0)[live], rtol=1e-14)
    assert np.isnan(chain.weight_mean()[0, 0, 0])


# ---- keywords ---------------------------------------------------------------------------------

def test_keywords_become_a_dict():
    assert robust.check_keywords(None) is None
    assert robust.check_keywords(4) == dict(nu=4, every=1, start=0)
    assert robust.check_keywords(dict(nu=np.int64(7), every=3)) == dict(nu=7, every=3, start=0)
    assert robust.check_keywords(dict(nu=1, start=10 ** 9)) == dict(nu=1, every=1, start=10 ** 9)
    assert robust.last_due(dict(nu=4, every=3, start=2), 1) is None
    assert [robust.last_due(dict(nu=4, every=3, start=2), s) for s in (2, 4, 5, 6)] == [2, 2, 5, 5]


@pytest.mark.parametrize("value", [
    0, 31, -3, 4.0, "4", True, dict(), dict(every=2), dict(nu=4, every=0), dict(nu=4, start=-1),
    dict(nu=4, every=1.5), dict(nu=4, burn=3), dict(nu=None), (4, 1),
])
def test_run_refuses_bad_keywords_before_any_device_work(value):
    with pytest.raises(ValueError, match="robust"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, robust=value)


def test_run_refuses_tempering():
    with pytest.raises(ValueError, match="robust= with tempering="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, robust=4, tempering=dict(rungs=2, beta_min=0.5))


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="robust=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, robust=4)


def state_of(cfg=None):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=1)
    if cfg is not None:
        state["robust_keywords"] = robust.keyword_record(robust.check_keywords(cfg))
    return state


@pytest.mark.parametrize("saved, kw, what", [
    (4, dict(robust=3), r"robust=dict\(nu=4, every=1, start=0\).*robust=dict\(nu=3, every=1, start=0\)"),
    (dict(nu=4, every=2), dict(robust=4), "this run has robust="),
    (4, dict(), "this run has none"),
    (None, dict(robust=4), "written without robust="),
])
def test_run_refuses_a_state_written_with_other_values(saved, kw, what):
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(saved), **kw)


def test_resume_accepts_the_same_values():
    state = state_of(dict(nu=4, every=2, start=5))
    robust.check_resume(state, state, robust.check_keywords(dict(nu=4, every=2, start=5)))
    robust.check_resume(state_of(), state_of(), None)


# ---- the report --------------------------------------------------------------------------------

def test_report_and_pooling_by_count(tmp_path):
    cfg = robust.check_keywords(4)
    mean_a, mean_b = np.full((2, 1, 2), 0.2), np.full((2, 1, 2), 0.8)
    mean_a[0, 0, 0] = mean_b[0, 0, 0] = np.nan
    calls = []

    def fetch_a(weights, weight_mean):
        calls.append((weights, weight_mean))
        return (np.ones((2, 1, 2)) if weights else None), (mean_a if weight_mean else None), 1

    a = robust.RobustReport(cfg, 1, fetch_a)
    b = robust.RobustReport(cfg, 3, lambda w, m: (np.ones((2, 1, 2)), mean_b, 3))
    assert (a.nu, a.every, a.start, a.count) == (4, 1, 0, 1) and calls == []      # nothing fetched yet
    np.testing.assert_array_equal(a.downweighted(), [[[0, 1]], [[1, 1]]])
    a.weight_mean
    assert calls == [(False, True)]                                                # once
    both = robust.pooled([a, b])
    assert both.count == 4
    np.testing.assert_allclose(both.weight_mean[1], 0.2 * 0.25 + 0.8 * 0.75, rtol=1e-15)
    assert np.isnan(both.weight_mean[0, 0, 0])
    empty = robust.RobustReport(cfg, 0, lambda w, m: (np.ones((2, 1, 2)), np.zeros((2, 1, 2)), 0))
    assert np.isnan(empty.weight_mean).all() and empty.downweighted().sum() == 0
    both.save(str(tmp_path / "r"))
    saved = np.load(str(tmp_path / "r_robust.npz"))
    assert int(saved["nu"]) == 4 and int(saved["count"]) == 4
    assert os.path.exists(str(tmp_path / "r_robust_weight_mean.fits"))


# ---- the C ABI -----------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_built_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("Student-t likelihood: per-voxel noise weights"):]
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.ROBUST_PROTOTYPES
        decl = section.index("int %s(" % name)
        comment = section[section.rindex("/*", 0, decl):decl]
        assert re.search(r"lib/run\.py:\d+", comment), name
    for lines in ("lib/run.py:171-192", "lib/run.py:407-426"):
        assert lines in section
    for name in ("robust_begin", "robust_step", "robust_get", "robust_end"):
        assert callable(getattr(_lib.Engine, name))
    make = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\bd3d_robust\.hip\b", make, flags=re.M)
    import __graft_entry__ as entry
    assert "d3d_robust.hip" in entry.SOURCES                                   # d3d_source_hash covers it
    src = open(os.path.join(ROOT, "deconv3d_amd", "csrc", "d3d_robust.hip")).read()
    assert "fp contract(off)" in src and "0x%08x" % RO.TAG in src.lower()
