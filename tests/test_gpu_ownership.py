"""
GPU tests of who owns the library's device memory.  Every reading is the read-only option
``device_bytes``: the bytes the library's buffers hold in this process, all contexts together.

  1. an optional feature's end returns what its begin took (and a second begin takes no more); the base
     1/variance has one holder at a time, robust weights or noise scales (a (16, 12, 12) cube);
  2. closing engines and groups returns everything, whatever was armed, grown or allocated on use;
  3. the buffers of a one-call function do not outlive the call;
  4. arming the posterior features does not change the chain, bit for bit.

The cubes are the smallest that reach every allocation: (7, 9, 10) with a 3 x 3 FSF (odd depth: the
padded depth differs), and (6, 8, 8) with a 5 x 3 FSF.
"""
import numpy as np
import pytest

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [((7, 9, 10), (3, 3)), ((6, 8, 8), (5, 3))]


def small_case(shape, fsf_shape, seed=5):
    rng = np.random.default_rng(seed)
    D, H, W = shape
    fsf = 0.2 + rng.random(fsf_shape)
    fsf[fsf_shape[0] // 2, fsf_shape[1] // 2] += 2.
    fsf /= fsf.sum()
    lsf = O.gaussian_lsf_vector(D, 0.7)
    z = np.arange(D, dtype=float)[:, None, None]
    data = 5. * np.exp(-0.5 * ((z - 0.5 * D) / 1.2) ** 2) + rng.normal(0., 0.3, size=shape)
    var = (0.3 * (0.5 + rng.random(shape))) ** 2
    mask = np.ones((H, W))
    mask[1, 2] = 0
    min_b = O.model_min_boundaries()
    max_b = O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(shape=shape, fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, min_b=min_b, max_b=max_b, init=init)


def engine_for(case, seed=4321):
    eng = _lib.Engine(case["shape"], case["fsf"].shape)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    eng.set_params(case["init"])
    eng.mh_config(case["min_b"], case["max_b"], 0.1, float(case["max_b"][0] ** 2), seed=seed, refresh_every=0)
    return eng


def held(eng):
    return eng.get_option("device_bytes")


class Sweeper(object):
    """Two sweeps a call, numbered on from the last call's, the chain streamed to the host."""

    def __init__(self, eng, case):
        self.eng, self.next = eng, 1
        self.hw = case["shape"][1:]
        self.chains = []

    def two(self):
        chain = np.full((self.next + 2,) + self.hw + (3,), np.nan)
        self.eng.mh_sweeps(2, self.next, 1, chain)
        self.chains.append(chain[self.next:self.next + 2].copy())
        self.next += 2


def warm(eng, case):
    """What the chain allocates on first use: the sweeps' tables, the snapshot ring, the prior's partials."""
    sw = Sweeper(eng, case)
    sw.two()
    eng.prior_energy()
    return sw


def labels_of(case):
    H, W = case["shape"][1:]
    return (np.arange(H * W).reshape(H, W) % 3 + 1).astype(np.int32)


def post_hist_regions(eng, case, sw):
    eng.post_begin()
    eng.post_schedule(sw.next, 1)
    eng.hist_begin(pilot=2, span=6.)
    eng.region_begin(labels_of(case), 3, capacity=4, spectra=True)


def arm_everything(eng, case, sw):
    post_hist_regions(eng, case, sw)
    eng.adapt_begin(window=1, last_sweep=100)
    eng.robust_begin(4)


# ---- 1. begin / end symmetry ----------------------------------------------------------------------

def test_end_returns_what_begin_took():
    case = small_case(*SHAPES[0])
    with engine_for(case) as eng:
        sw = warm(eng, case)
        b = held(eng)
        assert b > 0

        def moments(what):
            def begin():
                eng.post_begin(what)
                eng.post_schedule(sw.next, 1)
            return begin

        def moments_and_histograms():
            moments(_lib.POST_CLEAN | _lib.POST_CONVOLVED)()
            eng.hist_begin(pilot=2, span=6.)

        def moments_and_regions():
            moments(_lib.POST_CLEAN)()
            eng.region_begin(labels_of(case), 3, capacity=4, spectra=True)

        features = [("clean moments", moments(_lib.POST_CLEAN), [eng.post_end]),
                    ("convolved moments", moments(_lib.POST_CONVOLVED), [eng.post_end]),
                    ("moments + histograms", moments_and_histograms, [eng.hist_end, eng.post_end]),
                    ("moments + regions", moments_and_regions, [eng.region_end, eng.post_end]),
                    ("jump scales", lambda: eng.adapt_begin(window=1, last_sweep=100), [eng.adapt_end]),
                    ("robust weights", lambda: eng.robust_begin(4), [eng.robust_end])]
        for name, begin, ends in features:
            begin()
            armed = held(eng)
            print("%s: %d bytes over the baseline of %d" % (name, armed - b, b))
            assert armed > b, name
            if len(ends) == 1 and ends[0] in (eng.adapt_end, eng.robust_end):
                begin()                                     # begun twice: the first begin's buffers went
                assert held(eng) == armed, name
            sw.two()
            assert held(eng) == armed, name                 # the sweeps allocate nothing more
            for k, end in enumerate(ends):
                end()
                if k + 1 < len(ends):
                    assert b < held(eng) < armed, name      # the histograms / regions alone went
            assert held(eng) == b, name

        # a second post_begin frees the histograms and regions armed on the first
        readings = []
        for _ in range(2):
            post_hist_regions(eng, case, sw)
            sw.two()
            assert eng.post_count() == 2 and eng.hist_count() == 0 and eng.region_count() == (2, 2)
            readings.append(held(eng))
        assert readings[0] == readings[1] > b
        eng.post_end()                                      # histograms and regions still armed
        assert held(eng) == b


@pytest.mark.parametrize("uniform", [True, False])
def test_the_base_variance_passes_from_robust_weights_to_noise_scales_and_back(uniform):
    """One base 1/variance, one holder at a time: a second robust_begin saves the base cube and not the
    rescaled one, ending the feature that does not hold it changes nothing, and the holder's end gives
    back the cube, the uniform flag and the memory of before the first begin."""
    case = small_case((16, 12, 12), (3, 3))
    with engine_for(case) as eng:
        if uniform:
            eng.set_data(case["data"], None, 0.09, mask=case["mask"])
        assert eng.variance_is_uniform() == uniform
        warm(eng, case)
        base, b = eng.download_slot(_lib.SLOT_IVAR), held(eng)
        assert np.isfinite(base).all() and (base > 0.).any()
        eng.robust_begin(4)
        eng.robust_step(1)
        assert not np.array_equal(eng.download_slot(_lib.SLOT_IVAR), base)
        eng.robust_begin(4)
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), base)
        eng.robust_end()
        eng.noise_begin(np.arange(16) // 4)
        eng.noise_step(1)
        rescaled = eng.download_slot(_lib.SLOT_IVAR)
        assert not np.array_equal(rescaled, base)
        eng.robust_end()                                    # (not the holder)
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), rescaled)
        assert not eng.variance_is_uniform() and eng.noise_count() == 1
        eng.noise_end()
        np.testing.assert_array_equal(eng.download_slot(_lib.SLOT_IVAR), base)
        assert eng.variance_is_uniform() == uniform and held(eng) == b


# ---- 2. destroy frees everything -------------------------------------------------------------------

@pytest.mark.parametrize("shape,fsf_shape", SHAPES)
def test_closing_returns_everything(shape, fsf_shape):
    case = small_case(shape, fsf_shape)
    D, H, W = shape
    fh, fw = fsf_shape
    with _lib.Engine((2, 1, 3), (1, 1)) as e0:
        b0 = held(e0)
        engines = [engine_for(case, seed=11 + r) for r in range(2)]
        third = engine_for(case, seed=99)
        try:
            sweepers = [warm(e, case) for e in engines]
            for e, sw in zip(engines, sweepers):
                arm_everything(e, case, sw)
                sw.two()
            assert held(e0) > b0
            # a partitioned context with a halo plan (allocation only) and a host-evaluated colour class
            third.residual(fetch=False)
            third.set_parts([[0, H // 2, 0, W], [H // 2, H, 0, W]], [0, 1])
            third.halo_plan(0, [[0, 0, 0, 2, 0, 3, 0, 2, 0, 3]])
            ys, xs = np.meshgrid(np.arange(0, H, fh), np.arange(0, W, fw), indexing="ij")
            spaxels = (ys * W + xs).ravel()                 # one colour class: disjoint windows
            assert spaxels.size == (12 if shape == SHAPES[0][0] else 6)
            z = np.arange(D, dtype=float)
            for n in (3, spaxels.size):                     # the second call grows the staging buffer
                lines = np.empty((n, 2, D))
                lines[:, 0] = np.exp(-0.5 * ((z - 0.4 * D) / 1.1) ** 2)
                lines[:, 1] = np.exp(-0.5 * ((z - 0.6 * D) / 0.9) ** 2)
                in3 = np.column_stack((np.ones(n), np.zeros(n), np.full(n, -1.)))
                before = held(e0)
                out = third.mh_colour_lines(1, spaxels[:n], in3, lines)
                assert out.shape == (n, 3) and held(e0) > before
            centres, widths = 0.5 * D + np.arange(-1., 2.), [0.8, 1.5]
            best, stat = engines[0].line_search(centres, widths)
            assert best.shape == (H, W)
            engines[1].prepare(case["data"], 2, reject=3.)
            engines[0].hist_quantiles([0.25, 0.5])
            with _lib.TemperGroup(engines, [1., 0.5], seed=3, patch=2) as group:
                for rnd in range(2):
                    group.swap(rnd)
                assert group.get()["rounds"] == 2 and group.last_patches() is not None
        finally:
            for e in engines + [third]:
                e.close()
        assert held(e0) == b0


# ---- 3. per-call buffers ---------------------------------------------------------------------------

def test_call_buffers_do_not_outlive_the_call():
    case = small_case(*SHAPES[0])
    D = case["shape"][0]
    engines = [engine_for(case, seed=21 + r) for r in range(2)]
    try:
        for e in engines:
            sw = warm(e, case)
            e.post_begin(0)
            e.hist_begin(pilot=2, span=6.)
            e.post_schedule(sw.next, 1)
            sw.two()
        calls = [("line_search", lambda e: e.line_search(0.5 * D + np.arange(-1., 2.), [0.8, 1.5])),
                 ("running_median", lambda e: e.running_median(case["data"], 2)),
                 ("channel_stats", lambda e: e.channel_stats(case["data"])),
                 ("prepare", lambda e: e.prepare(case["data"], 2, reject=3.)),
                 ("prepare, no rejection", lambda e: e.prepare(case["data"], 2)),
                 ("hist_quantiles", lambda e: e.hist_quantiles([0.16, 0.5, 0.84]))]
        for e in engines:
            for name, call in calls:
                before = held(e)
                call(e)
                assert held(e) == before, name
        before = held(engines[0])
        _lib.mh_sweeps_batch(engines, 2, first_sweep=5)
        first = held(engines[0])
        _lib.mh_sweeps_batch(engines, 2, first_sweep=7)
        assert before == first == held(engines[0])
    finally:
        for e in engines:
            e.close()


# ---- 4. the chain is the same chain -----------------------------------------------------------------

def test_armed_posterior_features_leave_the_chain_bit_for_bit():
    case = small_case(*SHAPES[0])
    states = []
    for armed in (False, True):
        with engine_for(case) as eng:
            sw = warm(eng, case)
            if armed:
                post_hist_regions(eng, case, sw)
            sw.two()
            sw.two()
            if armed:
                assert eng.post_count() == 4 and eng.hist_count() == 2
            states.append((np.concatenate(sw.chains), eng.get_params(), eng.get_dlog()))
    assert not np.isnan(states[0][0]).any()
    for plain, with_features in zip(*states):
        np.testing.assert_array_equal(plain, with_features)
