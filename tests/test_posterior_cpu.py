"""
Host side of the posterior moments (deconv3d_amd/posterior.py, Run's posterior_* arguments):
the pooling of (n, mean, M2) triples against numpy, the standard deviation's edge cases, and the
refusals of Run that need no device.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib, posterior


def triple(block, shape):
    """(n, mean, M2) of a block of samples, by numpy."""
    if len(block) == 0:
        return 0, np.full(shape, np.nan), np.full(shape, np.nan)    # (must not be read)
    mean = block.mean(axis=0)
    return len(block), mean, ((block - mean) ** 2).sum(axis=0)


@pytest.mark.parametrize("sizes", [(17,), (9, 23), (5, 1, 0, 24, 7), (0, 3, 0), (1, 1, 1, 1)])
def test_pool_equals_numpy_over_the_concatenation(sizes):
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    shape = (6, 5, 4)
    # a mean far from zero with a small spread: where a naive sum of squares loses digits
    samples = 1e3 + rng.normal(0., 2., size=(sum(sizes),) + shape) * rng.uniform(0.1, 10., size=shape)
    blocks, at = [], 0
    for n in sizes:
        blocks.append(triple(samples[at:at + n], shape))
        at += n
    n, mean, m2 = posterior.pool(blocks)
    assert n == sum(sizes)
    np.testing.assert_allclose(mean, samples.mean(axis=0), rtol=1e-12, atol=0.)
    np.testing.assert_allclose(m2 / (n - 1), samples.var(axis=0, ddof=1), rtol=1e-12, atol=0.)
    np.testing.assert_allclose(posterior.std_from_m2(n, m2), samples.std(axis=0, ddof=1), rtol=1e-12, atol=0.)


def test_pool_of_empty_and_single_blocks():
    shape = (3, 2)
    n, mean, m2 = posterior.pool([triple(np.zeros((0,) + shape), shape)] * 2)
    assert n == 0 and not np.isnan(mean).any() and not np.isnan(m2).any()
    one = np.arange(6.).reshape((1,) + shape)
    n, mean, m2 = posterior.pool([triple(one, shape), triple(np.zeros((0,) + shape), shape)])
    assert n == 1
    np.testing.assert_array_equal(mean, one[0])
    np.testing.assert_array_equal(m2, 0.)
    assert np.isnan(posterior.std_from_m2(1, m2)).all() and np.isnan(posterior.std_from_m2(0, m2)).all()
    with pytest.raises(ValueError):
        posterior.pool([])
    with pytest.raises(ValueError):
        posterior.pool([(2, np.zeros(3), np.zeros(3)), (2, np.zeros(4), np.zeros(4))])
    with pytest.raises(ValueError):
        posterior.pool([(-1, np.zeros(3), np.zeros(3))])


def test_moments_object_is_lazy_nan_aware_and_pools():
    rng = np.random.default_rng(3)
    D, H, W = 4, 3, 2
    calls = []

    def source(samples_map, samples_cube):
        def fetch(which):
            calls.append(which)
            s = samples_map if which == posterior.PARAMETERS else samples_cube
            return triple(s, s.shape[1:])[1:]
        return fetch

    maps = [rng.normal(size=(n, H, W, 4)) for n in (5, 8)]
    cubes = [rng.normal(size=(n, D, H, W)) for n in (5, 8)]
    template = d3d.MUSE().build_cube(np.zeros((D, H, W)))
    parts = [posterior.PosteriorMoments(len(m), source(m, c), template) for m, c in zip(maps, cubes)]
    assert calls == []                                    # nothing fetched before first access
    both = posterior.pooled(parts, template)
    assert both.count == 13 and calls == []
    all_maps, all_cubes = np.concatenate(maps), np.concatenate(cubes)
    np.testing.assert_allclose(both.parameters_mean, all_maps.mean(0)[..., :3], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(both.flux_std, all_maps.std(0, ddof=1)[..., 3], rtol=1e-12)
    assert sorted(calls) == [posterior.PARAMETERS] * 2     # once per part, kept afterwards
    np.testing.assert_allclose(both.convolved_std, all_cubes.std(0, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(parts[0].clean_mean, cubes[0].mean(0), rtol=1e-12, atol=1e-15)
    cube = both.convolved_cube()
    assert isinstance(cube, d3d.Cube) and cube.data.shape == (D, H, W) and cube.z is template.z
    assert both.parameters_mean.shape == (H, W, 3) and both.flux_mean.shape == (H, W)
    # no sample: NaN arrays; one sample: its value, NaN error bar
    empty = posterior.PosteriorMoments(0, lambda which: (np.zeros((D, H, W)), np.zeros((D, H, W))))
    assert np.isnan(empty.clean_mean).all() and np.isnan(empty.clean_std).all()
    single = posterior.PosteriorMoments(1, lambda which: (np.ones((D, H, W)), np.zeros((D, H, W))))
    assert (single.convolved_mean == 1.).all() and np.isnan(single.convolved_std).all()


def test_moments_save_writes_fits_and_npz(tmp_path):
    rng = np.random.default_rng(5)
    D, H, W = 5, 4, 3
    cubes, maps = rng.normal(size=(6, D, H, W)), rng.normal(size=(6, H, W, 4))
    template = d3d.MUSE().build_cube(np.zeros((D, H, W)))
    pm = posterior.PosteriorMoments(
        6, lambda which: triple(maps if which == posterior.PARAMETERS else cubes * (1 + which),
                                (maps if which == posterior.PARAMETERS else cubes).shape[1:])[1:], template)
    prefix = str(tmp_path / "run")
    pm.save(prefix)
    back = d3d.Cube.from_fits(prefix + "_posterior_convolved_std.fits")
    np.testing.assert_allclose(back.data, (cubes * 3).std(0, ddof=1), rtol=1e-12)
    back = d3d.Cube.from_fits(prefix + "_posterior_clean_mean.fits")
    np.testing.assert_allclose(back.data, (cubes * 2).mean(0), rtol=1e-12, atol=1e-15)
    z = np.load(prefix + "_posterior_parameters.npz")
    assert int(z["count"]) == 6
    np.testing.assert_allclose(z["flux_mean"], maps.mean(0)[..., 3], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("kw", [dict(posterior_burn_in=0), dict(posterior_burn_in=-3),
                                dict(posterior_burn_in=2.5), dict(posterior_burn_in="4"),
                                dict(posterior_burn_in=True),
                                dict(posterior_burn_in=5, posterior_every=0),
                                dict(posterior_burn_in=5, posterior_every=1.5)])
def test_run_refuses_a_bad_schedule_before_any_device_work(kw):
    cube = d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)))
    with pytest.raises(ValueError, match="posterior_"):
        d3d.Run(cube, d3d.MUSE(), max_iterations=4, **kw)


def test_run_refuses_a_host_evaluated_model_by_name():
    class Lorentzian(d3d.SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            a, c, w = parameters
            return a / (1. + ((x - c) / w) ** 2)

    cube = d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)
    with pytest.raises(NotImplementedError, match="Lorentzian"):
        d3d.Run(cube, d3d.MUSE(), model=Lorentzian, max_iterations=4, posterior_burn_in=2)


def test_binding_declares_the_entry_points():
    for name in ("d3d_post_begin", "d3d_post_schedule", "d3d_post_accumulate", "d3d_post_count",
                 "d3d_post_get", "d3d_post_end"):
        assert name in _lib.SYMBOLS
    assert d3d.PosteriorMoments is posterior.PosteriorMoments
