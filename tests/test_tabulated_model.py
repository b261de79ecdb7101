"""
CPU tests (no GPU) of TabulatedLineModel: the constructor's rules and normalisation, the curve
against the independent restatement of tests/tabulated_oracle.py bit for bit (w = 0, both ends
of the table, NaN), the flux factor, the routing between the device kernels and the host path,
the table digest of the checkpoint, the C entry point's declaration, and the Run keyword checks
that happen before any device work.
"""
import math
import os

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.line_models import (GaussianMultipletLineModel, SingleGaussianLineModel,
                                      TabulatedLineModel, device_line_shape, device_line_table,
                                      model_is_on_device)
from tests import tabulated_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_of(key, **kw):
    return TabulatedLineModel(*TO.PROFILES[key](), **kw)


# ---- constructor ------------------------------------------------------------------------------

@pytest.mark.parametrize("profile,support,rule", [
    (np.ones(7), 1., "8 to 65537 samples"),
    (np.ones(65538), 1., "8 to 65537 samples"),
    (np.ones((4, 4)), 1., "one-dimensional"),
    (np.ones(16), 0., "support"),
    (np.ones(16), -2., "support"),
    (np.ones(16), float("nan"), "support"),
    (np.ones(16), float("inf"), "support"),
    ([1.] * 8 + [float("nan")], 1., "finite"),
    ([1.] * 8 + [float("inf")], 1., "finite"),
    (np.zeros(16), 1., "zero everywhere"),
    ([0.5] * 8 + [-2.], 1., "must be positive"),
    (["a"] * 8, 1., "numbers"),
])
def test_the_constructor_refuses(profile, support, rule):
    with pytest.raises(ValueError, match=rule):
        TabulatedLineModel(profile, support)


def test_the_multiplet_rules_hold_for_offsets_and_ratios():
    tab, sup = TO.profile_C()
    with pytest.raises(ValueError, match="offsets\\[0\\] must be 0"):
        TabulatedLineModel(tab, sup, offsets=[1., 0.], ratios=[1., 1.])
    with pytest.raises(ValueError, match="ratios must be >= 0"):
        TabulatedLineModel(tab, sup, offsets=[0., 1.], ratios=[1., -1.])
    m = TabulatedLineModel(tab, sup, offsets=[0., 3.8], ratios=[1., 1.4])
    assert device_line_shape(m) == ((0., 3.8), (1., 1.4))
    assert device_line_shape(TabulatedLineModel(tab, sup)) == ((0.,), (1.,))


def test_the_table_is_normalised_to_a_peak_of_one():
    tab, sup = TO.profile_S()
    assert tab.max() > 1.4
    m = TabulatedLineModel(tab, sup)
    assert m.table.max() == 1. and np.abs(m.table).max() == 1.
    np.testing.assert_array_equal(m.table, tab / tab.max())
    np.testing.assert_array_equal(m.table, TO.normalised(tab))
    c = model_of("C")
    assert c.table.min() == -0.3 and c.table[3] == 1.         # negative lobes stay
    # a negative lobe deeper than the peak is high: the largest magnitude must be positive
    with pytest.raises(ValueError, match="must be positive"):
        TabulatedLineModel([0., 0.2, 1., -1.5, 0.3, 0., 0., 0.], 2.)
    # the caller's array is not touched, the model's own is read-only
    assert tab.max() > 1.4
    with pytest.raises(ValueError):
        m.table[0] = 3.


def test_names_gibbs_index_and_bounds_are_the_single_gaussians():
    class Runner:
        cube = d3d.MUSE().build_cube(np.random.default_rng(1).random((40, 6, 7)) * 3.)
        fsf = np.array([[0.1, 0.2], [0.3, 0.4]])

    one, tab = SingleGaussianLineModel(), model_of("S")
    assert tab.parameters() == one.parameters() == ['a', 'c', 'w']
    assert tab.gibbs_parameter_index() == 0
    assert tab.min_boundaries(Runner) == one.min_boundaries(Runner)
    assert tab.max_boundaries(Runner) == one.max_boundaries(Runner)


def test_from_function_samples_the_callable():
    m = TabulatedLineModel.from_function(lambda u: math.exp(-u * u / 2.), 8.)
    g = model_of("G")
    assert m.table.size == 2049 and m.support == 8.
    np.testing.assert_allclose(m.table, g.table, rtol=0, atol=1e-15)
    d = TabulatedLineModel.from_function(lambda u: 1. / (1. + u * u), 10., samples=129,
                                         offsets=[0., 2.], ratios=[1., 0.5])
    assert d.table.size == 129 and d.offsets == (0., 2.) and d.table[64] == 1.


# ---- the curve --------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["G", "S", "L", "C"])
def test_modelize_is_the_restated_interpolant_bit_for_bit(key):
    tab, sup = TO.PROFILES[key]()
    m = TabulatedLineModel(tab, sup)
    want = TO.line(tab, sup)
    x = np.arange(48, dtype=np.float64)
    rng = np.random.default_rng(sum(map(ord, key)))
    for _ in range(25):
        a, c, w = rng.uniform(0.1, 9.), rng.uniform(-6., 54.), rng.uniform(0.02, 12.)
        np.testing.assert_array_equal(m.modelize(None, x, [a, c, w]), want(x, a, c, w))
    # w = 0: the value at u = 0 where x == c, 0 elsewhere
    got = m.modelize(None, x, [2., 7., 0.])
    np.testing.assert_array_equal(got, want(x, 2., 7., 0.))
    assert got[7] == 2. * TO.phi_scalar(TO.normalised(tab), sup, 0., 1.) and np.count_nonzero(got) == 1
    assert np.count_nonzero(m.modelize(None, x, [2., 7.5, 0.])) == 0
    # NaN parameters give a line of zeros
    for p in ([1., float("nan"), 2.], [1., 5., float("nan")]):
        np.testing.assert_array_equal(m.modelize(None, x, p), np.zeros(48))
        np.testing.assert_array_equal(want(x, *p), np.zeros(48))


def test_doublet_is_the_restated_sum_bit_for_bit():
    tab, sup = TO.profile_C()
    off, rat = [0., 3.8], [1., 1.4]
    m = TabulatedLineModel(tab, sup, offsets=off, ratios=rat)
    want = TO.line(tab, sup, off, rat)
    x = np.arange(30, dtype=np.float64)
    rng = np.random.default_rng(3)
    for _ in range(25):
        a, c, w = rng.uniform(0.1, 9.), rng.uniform(-3., 33.), rng.uniform(0.05, 5.)
        np.testing.assert_array_equal(m.modelize(None, x, [a, c, w]), want(x, a, c, w))


def test_both_ends_of_the_table_and_the_padding():
    """t exactly 0 and exactly n - 1 (u = -support, +support; support 3.5 and w = 2 are exact in
    binary), just beyond them, and the intervals that read the padded zeros."""
    tab = [0.25, -0.3, 0.2, 1., 0.6, 0.1, -0.1, 0.5]          # ends that are not zero
    m = TabulatedLineModel(tab, 3.5)
    want = TO.line(tab, 3.5)
    c, w = 10., 2.
    x = np.array([c - 7., c + 7., c - 7. - 2. ** -40, c + 7. + 2. ** -40,
                  c - 6., c + 6., c - 5., c + 5., c, c + 0.3])
    got = m.modelize(None, x, [1., c, w])
    np.testing.assert_array_equal(got, want(x, 1., c, w))
    assert got[0] == 0.25 and abs(got[1] - 0.5) < 1e-15                  # t = 0: p1 = tab[0]; t = n - 1: s = 1, p2 = tab[-1]
    assert got[2] == 0. and got[3] == 0.                      # beyond the support
    assert got[6] == -0.3 and got[7] == -0.1 and got[8] == m.phi(0., 1.)
    # first interval by hand (h = 1: t = u + 3.5): p0 = 0 (padding), s = 1/2
    p0, p1, p2, p3, s = 0., 0.25, -0.3, 0.2, 0.5
    by_hand = p1 + 0.5 * s * ((p2 - p0) + s * ((2 * p0 - 5 * p1 + 4 * p2 - p3) + s * (3 * (p1 - p2) + (p3 - p0))))
    assert got[4] == by_hand
    # last interval: j = n - 2, p3 = 0 (padding)
    p0, p1, p2, p3 = 0.1, -0.1, 0.5, 0.
    by_hand = p1 + 0.5 * s * ((p2 - p0) + s * ((2 * p0 - 5 * p1 + 4 * p2 - p3) + s * (3 * (p1 - p2) + (p3 - p0))))
    assert got[5] == by_hand


def test_a_mirrored_table_is_another_curve():
    tab, sup = TO.profile_S()
    m, flipped = TabulatedLineModel(tab, sup), TabulatedLineModel(tab[::-1], sup)
    x = np.arange(32, dtype=np.float64)
    a = m.modelize(None, x, [1., 15.2, 2.])
    b = flipped.modelize(None, x, [1., 15.2, 2.])
    assert np.max(np.abs(a - b)) > 0.3
    assert np.argmax(a) > 15.2 > np.argmax(b)                 # the skew points to larger channels


def test_the_interpolant_reproduces_the_profile():
    g = model_of("G")
    u = np.linspace(-9., 9., 20001)
    e = np.max(np.abs(g.phi(u, 1.) - np.exp(-u ** 2 / 2.)))
    assert e < 5e-8, e


# ---- flux factor ------------------------------------------------------------------------------

def test_flux_factor():
    g = model_of("G")
    assert abs(g.flux_factor - math.sqrt(2. * math.pi)) <= 1e-12
    assert abs(g.flux_factor - TO.trapezoid(*TO.profile_G())) <= 1e-13
    for key in ("S", "L", "C"):
        assert abs(model_of(key).flux_factor - TO.trapezoid(*TO.PROFILES[key]())) <= 1e-12
    d = model_of("G", offsets=[0., 3.8], ratios=[1., 1.4])
    assert d.flux_factor == g.table_integral * 2.4
    assert device_line_table(d)[2] == g.table_integral        # the device multiplies by the ratios


# ---- routing ----------------------------------------------------------------------------------

def test_routing_to_the_device_or_the_host():
    tab, sup = TO.profile_S()

    class Renamed(TabulatedLineModel):
        def parameters(self):
            return ['flux', 'centre', 'width']

    class OwnCurve(TabulatedLineModel):
        def modelize(self, runner, x, parameters):
            return TabulatedLineModel.modelize(self, runner, x, parameters)

    class OwnInterpolant(TabulatedLineModel):
        def phi(self, d, w):
            return np.interp(d / w, np.linspace(-self.support, self.support, self.table.size), self.table)

    class OwnSum(TabulatedLineModel):
        def tabulated(self, x, a, c, w):
            return a * self.phi(x - c, w)

    class OwnJump(TabulatedLineModel):
        def post_jump(self, runner, old_parameters, new_parameters):
            new_parameters[2] = abs(new_parameters[2])

    assert model_is_on_device(TabulatedLineModel(tab, sup))
    assert model_is_on_device(Renamed(tab, sup))
    for cls in (OwnCurve, OwnInterpolant, OwnSum, OwnJump):
        assert not model_is_on_device(cls(tab, sup)), cls.__name__
    m = TabulatedLineModel(tab, sup)
    table, support, flux = device_line_table(m)
    assert table is m.table and support == sup and flux == m.table_integral
    # device_line_shape keeps its contract, and the Gaussians have no table
    assert device_line_shape(SingleGaussianLineModel()) == ((0.,), (1.,))
    assert device_line_table(SingleGaussianLineModel()) is None
    assert device_line_table(GaussianMultipletLineModel([0., 3.8], [1., 1.4])) is None


# ---- digest, C ABI ----------------------------------------------------------------------------

def test_the_digest_changes_with_one_sample_n_or_support():
    tab, sup = TO.profile_S()
    base = TabulatedLineModel(tab, sup).digest()
    assert base == TabulatedLineModel(tab.copy(), sup).digest() and len(base) == 64
    other = tab.copy()
    other[100] = np.nextafter(other[100], 1.)
    assert TabulatedLineModel(other, sup).digest() != base
    assert TabulatedLineModel(tab, np.nextafter(sup, 7.)).digest() != base
    assert TabulatedLineModel(np.append(tab, 0.), sup).digest() != base


def test_entry_point_is_declared_bound_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "deconv3d_hip.h")).read()
    assert "int d3d_set_line_table(d3d_ctx *ctx, int n, double support, const double *table, double flux_factor);" in text
    comment = text[text.index("d3d_set_line_shape(d3d_ctx"):text.index("int d3d_set_line_table")]
    assert "lib/line_models.py:" in comment and "92-109" in comment
    assert "d3d_set_line_table" in _lib.SYMBOLS
    assert hasattr(_lib.Engine, "set_line_table")
    assert d3d.TabulatedLineModel is TabulatedLineModel


# ---- Run, before any device work --------------------------------------------------------------

def small_cube():
    return d3d.MUSE().build_cube(np.random.default_rng(0).random((8, 9, 9)) + 1.)


def state_of(digest=None):
    state = dict(iteration=11, seed=12345, accepted_count=100, sweep_origin=0, n_chains=1)
    if digest is not None:
        state["line_table_digest"] = np.array(digest)
    return state


def test_run_refuses_a_state_written_with_another_table():
    tab, sup = TO.profile_S()
    model = TabulatedLineModel(tab, sup)
    other = tab.copy()
    other[300] *= 1.0000001
    for state, what in ((state_of(TabulatedLineModel(other, sup).digest()), "line table"),
                        (state_of(), "Gaussian lines")):
        with pytest.raises(ValueError, match=what):
            d3d.Run(small_cube(), d3d.MUSE(), model=model, max_iterations=40, resume_state=state)
    # ... and a table's state is refused by a run of Gaussians
    with pytest.raises(ValueError, match="line table"):
        d3d.Run(small_cube(), d3d.MUSE(), max_iterations=40, resume_state=state_of(model.digest()))


def test_an_equivalent_host_evaluated_model_is_still_refused():
    tab, sup = TO.profile_S()

    class Host(TabulatedLineModel):
        def modelize(self, runner, x, parameters):
            return TabulatedLineModel.modelize(self, runner, x, parameters)

    for kw in (dict(smoothness=dict(c=1.)), dict(adapt_sweeps=20, adapt_window=10), dict(posterior_burn_in=10)):
        with pytest.raises(NotImplementedError, match="evaluated on the host"):
            d3d.Run(small_cube(), d3d.MUSE(), model=Host(tab, sup), max_iterations=40, **kw)
