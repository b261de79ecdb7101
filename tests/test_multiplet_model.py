"""
CPU tests (no GPU) of GaussianMultipletLineModel: the plugin contract it shares with
SingleGaussianLineModel, its curve, its validation rules, the rest-wavelength
constructor and the routing of Run between the device kernels and the host path.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd.line_models import (GaussianMultipletLineModel, SingleGaussianLineModel,
                                      device_line_shape, model_is_on_device)


class _Runner:
    """What the bounds read of a Run: the cube's data and the FSF."""

    def __init__(self, data, fsf):
        self.cube = d3d.MUSE().build_cube(data)
        self.fsf = fsf


def test_names_gibbs_index_and_bounds_are_the_single_gaussians():
    rng = np.random.default_rng(1)
    data = rng.random((40, 6, 7)) * 3.0
    data[3, 2, 2] = np.nan
    runner = _Runner(data, np.array([[0.1, 0.2], [0.3, 0.4]]))
    one, multi = SingleGaussianLineModel(), GaussianMultipletLineModel([0., 3.8], [1., 1.4])
    assert multi.parameters() == one.parameters() == ['a', 'c', 'w']
    assert multi.gibbs_parameter_index() == one.gibbs_parameter_index() == 0
    assert multi.min_boundaries(runner) == one.min_boundaries(runner) == [0, 0, 0]
    assert multi.max_boundaries(runner) == one.max_boundaries(runner)
    assert multi.max_boundaries(runner)[1:] == [39, 40]
    assert not isinstance(multi, SingleGaussianLineModel)


@pytest.mark.parametrize("offsets,ratios", [([0., 3.8], [1., 1.4]),
                                            ([0., -14.5, 15.2], [1., 0.34, 0.11]),
                                            ([0., 1., 2., -7.5], [1., 0., 2.5, 0.3])])
def test_modelize_is_the_explicit_sum(offsets, ratios):
    m = GaussianMultipletLineModel(offsets, ratios)
    x = np.arange(64, dtype=float)
    a, c, w = 2.5, 30.3, 1.7
    want = a * sum(r * np.exp(-((x - c) - d) ** 2 / (2. * w ** 2)) for d, r in zip(offsets, ratios))
    np.testing.assert_allclose(m.modelize(None, x, [a, c, w]), want, rtol=1e-14, atol=1e-300)
    assert m.offsets == tuple(offsets) and m.ratios == tuple(ratios)
    assert device_line_shape(m) == (tuple(offsets), tuple(ratios))


def test_one_component_is_the_single_gaussian_bit_for_bit():
    m, one = GaussianMultipletLineModel([0], [1]), SingleGaussianLineModel()
    x = np.arange(128, dtype=float)
    rng = np.random.default_rng(2)
    for _ in range(20):
        p = [rng.uniform(0, 10), rng.uniform(-5, 133), rng.uniform(0.05, 20)]
        np.testing.assert_array_equal(m.modelize(None, x, p), one.modelize(None, x, p))


@pytest.mark.parametrize("offsets,ratios,rule", [
    ([], [], "1 to 4 components"),
    ([0., 1., 2., 3., 4.], [1.] * 5, "1 to 4 components"),
    ([0., 1.], [1.], "same length"),
    ([0., np.nan], [1., 1.], "finite"),
    ([0., 1.], [1., np.inf], "finite"),
    ([1., 0.], [1., 1.], "offsets\\[0\\] must be 0"),
    ([0., 1.], [0.5, 1.], "ratios\\[0\\] must be 1"),
    ([0., 1.], [1., -0.1], "ratios must be >= 0"),
    ([0., 2., 2.], [1., 1., 1.], "offsets must be distinct"),
    ([0., 0.], [1., 1.], "offsets must be distinct"),
    (["a", 1.], [1., 1.], "numbers"),
])
def test_every_validation_rule_raises(offsets, ratios, rule):
    with pytest.raises(ValueError, match=rule):
        GaussianMultipletLineModel(offsets, ratios)


def test_from_rest_wavelengths_gives_the_oii_doublet_on_a_muse_cube():
    cube = d3d.MUSE().build_cube(np.zeros((64, 8, 8)))
    assert cube.z_step == pytest.approx(1.25e-4)                  # 1.25 A in micrometres
    oii = GaussianMultipletLineModel.from_rest_wavelengths(cube, [0.372603, 0.372882], [1.0, 1.4],
                                                           redshift=0.7)
    assert oii.offsets[0] == 0.
    assert oii.offsets[1] == pytest.approx((0.372882 - 0.372603) * 1.7 / 1.25e-4, rel=1e-12)
    assert oii.offsets[1] == pytest.approx(3.7944, abs=1e-4)
    assert oii.ratios == (1.0, 1.4)
    with pytest.raises(ValueError, match="ratios\\[0\\] must be 1"):
        GaussianMultipletLineModel.from_rest_wavelengths(cube, [0.372603, 0.372882], [1.4, 1.0], 0.7)


def test_routing_to_the_device_or_the_host():
    class Renamed(GaussianMultipletLineModel):
        def parameters(self):
            return ['flux', 'centre', 'width']

    class OwnCurve(GaussianMultipletLineModel):
        def modelize(self, runner, x, parameters):
            return GaussianMultipletLineModel.modelize(self, runner, x, parameters)

    class OwnJump(GaussianMultipletLineModel):
        def post_jump(self, runner, old_parameters, new_parameters):
            new_parameters[2] = abs(new_parameters[2])

    doublet = ([0., 3.8], [1., 1.4])
    assert model_is_on_device(GaussianMultipletLineModel(*doublet))
    assert model_is_on_device(GaussianMultipletLineModel([0.], [1.]))
    assert model_is_on_device(Renamed(*doublet))
    assert not model_is_on_device(OwnCurve(*doublet))
    assert not model_is_on_device(OwnJump(*doublet))
    # the single Gaussian keeps its rule
    assert model_is_on_device(SingleGaussianLineModel())
    assert device_line_shape(SingleGaussianLineModel()) == ((0.,), (1.,))

    class OwnGaussian(SingleGaussianLineModel):
        def modelize(self, runner, x, parameters):
            return SingleGaussianLineModel.modelize(self, runner, x, parameters)

    assert not model_is_on_device(OwnGaussian())
    assert not model_is_on_device(d3d.LineModel())


def test_the_device_shape_is_the_one_modelize_sums_over():
    """The device's line shape is read from the attributes modelize uses: a subclass (or a
    caller) that changes them changes both."""
    class Shifted(GaussianMultipletLineModel):
        def __init__(self):
            GaussianMultipletLineModel.__init__(self, [0., 3.8], [1., 1.4])
            self.offsets = (0., 4.2)

    m = Shifted()
    assert model_is_on_device(m)
    assert device_line_shape(m) == ((0., 4.2), (1., 1.4))
    x = np.arange(32, dtype=float)
    want = 2. * (np.exp(-(x - 10.) ** 2 / 8.) + 1.4 * np.exp(-((x - 10.) - 4.2) ** 2 / 8.))
    np.testing.assert_allclose(m.modelize(None, x, [2., 10., 2.]), want, rtol=1e-14)


def test_exported_from_the_package():
    assert d3d.GaussianMultipletLineModel is GaussianMultipletLineModel
    from deconv3d_amd import _lib
    assert "d3d_set_line_shape" in _lib.SYMBOLS
    assert hasattr(_lib.Engine, "set_line_shape")
