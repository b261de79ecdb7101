"""
CPU tests (no GPU) of the per-spaxel jump scales (Run(adapt_sweeps=N), deconv3d_amd/adapt.py):
the keywords are validated, and a checkpoint written with other keywords refused, before any
device work; the C entry points are declared, bound, and cite the reference lines they extend.
"""
import os
import re

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, adapt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("d3d_adapt_begin", "d3d_adapt_get", "d3d_adapt_set", "d3d_adapt_end")


def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


@pytest.mark.parametrize("kw", [
    dict(adapt_sweeps=0), dict(adapt_sweeps=-5), dict(adapt_sweeps=2.5), dict(adapt_sweeps="4"),
    dict(adapt_sweeps=True),
    dict(adapt_sweeps=10, adapt_window=0), dict(adapt_sweeps=10, adapt_window=-1),
    dict(adapt_sweeps=10, adapt_window=2.5), dict(adapt_sweeps=10, adapt_window=11),
    dict(adapt_sweeps=10, adapt_window=5, adapt_target=0.), dict(adapt_sweeps=10, adapt_window=5, adapt_target=1.),
    dict(adapt_sweeps=10, adapt_window=5, adapt_target=float("nan")),
    dict(adapt_sweeps=10, adapt_window=5, adapt_gain=0.), dict(adapt_sweeps=10, adapt_window=5, adapt_gain=-1.),
    dict(adapt_sweeps=10, adapt_window=5, adapt_gain=float("inf")),
    dict(adapt_sweeps=10, adapt_window=5, adapt_scale_range=(0., 1.)),
    dict(adapt_sweeps=10, adapt_window=5, adapt_scale_range=(1e-3, float("inf"))),
    dict(adapt_sweeps=10, adapt_window=5, adapt_scale_range=(2., 1.)),
    dict(adapt_sweeps=10, adapt_window=5, adapt_scale_range=3.),
])
def test_run_refuses_bad_keywords_before_any_device_work(kw):
    with pytest.raises(ValueError, match="adapt_"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, **kw)


def test_run_refuses_moments_of_a_chain_that_still_adapts():
    with pytest.raises(ValueError, match="posterior_burn_in=10 lies before adapt_sweeps=20"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, adapt_sweeps=20, adapt_window=5,
                posterior_burn_in=10)


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    with pytest.raises(NotImplementedError, match="adapt_sweeps=: the line model Lorentzian"):
        d3d.Run(small_cube(), d3d.MUSE(), model=Lorentzian, max_iterations=40, adapt_sweeps=20,
                adapt_window=5)


def test_defaults_pass_and_are_recorded_in_order():
    cfg = adapt.check_keywords(200)
    assert cfg == (200, 50, 0.25, 2.0, (1e-3, 1e3))
    np.testing.assert_array_equal(adapt.keyword_record(cfg), [200, 50, 0.25, 2.0, 1e-3, 1e3])
    assert len(adapt.KEYWORDS) == 6


def state_of(cfg, n_chains=1, hw=(9, 9)):
    return dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=n_chains,
                adapt_keywords=adapt.keyword_record(cfg),
                adapt_scale=np.full((n_chains,) + hw, 1.5),
                adapt_accepted=np.full((n_chains,) + hw, 3, dtype=np.uint32),
                adapt_n_win=np.full(n_chains, 4, dtype=np.int64),
                adapt_k=np.full(n_chains, 2, dtype=np.int64))


def test_resume_restores_what_the_checkpoint_holds():
    cfg = adapt.check_keywords(20, 5)
    state = state_of(cfg, n_chains=2)
    got = adapt.check_resume(state, state, cfg, 2, (9, 9))
    assert len(got) == 2
    scale, acc, n_win, k = got[1]
    assert scale.shape == (9, 9) and acc.dtype == np.uint32 and (n_win, k) == (4, 2)
    assert adapt.check_resume(dict(iteration=3), dict(iteration=3), None, 1, (9, 9)) is None


@pytest.mark.parametrize("kw, what", [
    (dict(adapt_sweeps=20, adapt_window=4), "adapt_window=5.*adapt_window=4"),
    (dict(adapt_sweeps=20, adapt_window=5, adapt_target=0.3), "adapt_target=0.25.*adapt_target=0.3"),
    (dict(adapt_sweeps=20, adapt_window=5, adapt_gain=1.), "adapt_gain=2.*adapt_gain=1"),
    (dict(adapt_sweeps=20, adapt_window=5, adapt_scale_range=(1e-2, 1e3)), "adapt_scale_min"),
    (dict(adapt_sweeps=25, adapt_window=5), "adapt_sweeps=20.*adapt_sweeps=25"),
    (dict(), "this run has none"),
])
def test_run_refuses_a_state_written_with_other_keywords(kw, what):
    state = state_of(adapt.check_keywords(20, 5))
    with pytest.raises(ValueError, match=what):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state, **kw)


def test_run_refuses_to_start_adapting_from_a_state_without_scales():
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=1)
    with pytest.raises(ValueError, match="written without adapt_sweeps="):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state, adapt_sweeps=20,
                adapt_window=5)


def test_a_long_adaptation_is_warned_about(caplog):
    with caplog.at_level("WARNING", logger="deconv3d"):
        with pytest.raises(ValueError):     # (stops at the next check, still before the device)
            d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, adapt_sweeps=35, adapt_window=5,
                    mask=np.ones((2, 2)))
    assert any("80 %" in r.getMessage() for r in caplog.records)


def test_entry_points_are_declared_bound_and_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    section = text[text.index("per-spaxel jump scales"):text.index("spatial tiling")]
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name in _lib.ADAPT_PROTOTYPES
        # the comment in front of the declaration cites the lines of the reference it extends
        decl = section.index("int %s(" % name)
        comment = section[section.rindex("/*", 0, decl):decl]
        assert re.search(r"lib/run\.py:\d+", comment), name
    for lines in ("lib/run.py:251-262", "lib/run.py:344-364", "lib/run.py:570-579"):
        assert lines in section
