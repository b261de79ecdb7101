"""
CPU tests (no GPU) of tests/composed_oracle.py, the composition tests/test_gpu_composed.py compares the
device with: with every feature neutral it is the oracle's sweep bit for bit, with one feature on that
feature's own chain bit for bit, it can be continued from its own state, and the order of the refresh
and the draw shows in the drawn weights.
"""
import numpy as np
import pytest

from oracle import deconv3d_oracle as O
from tests import composed_oracle as CO
from tests import noise_oracle as NO
from tests import prior_oracle
from tests import robust_oracle as RB

SHAPE = (9, 6, 7)           # odd depth, NaN voxels, a whole NaN spectrum, zero variances, 5 x 5 taps
SWEEPS = 4
LAM = (4.0, 0.5, 2.0)


def problem():
    return CO.problem_of(NO.shape_case(SHAPE))


def plain_state(pb):
    """The oracle's state as a Composed holds it: NaN voxels carry nothing."""
    st = O.MHState(pb["data0"], pb["var"], pb["mask"], pb["fsf"], pb["lsf"], pb["init"], pb["min_b"], pb["max_b"],
                   pb["jump"], pb["ra"], pb["seed"])
    return st


def chain_state(pb, make):
    """A chain class made as Composed makes it (on the given data and variance), then run on the state
    the device runs on."""
    st = O.MHState(pb["data"], pb["var"], pb["mask"], pb["fsf"], pb["lsf"], pb["init"], pb["min_b"], pb["max_b"],
                   pb["jump"], pb["ra"], pb["seed"], err=plain_state(pb).err)
    chain = make(st)
    st.data = pb["data0"]
    with np.errstate(divide="ignore"):
        st.var = 1.0 / pb["i0"]
    return st, chain


def same_chain(a, b, what, accepted=True):
    for k in ("params", "err", "dlog", "var"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg="%s %s" % (what, k))
    assert a.accepted == b.accepted or not accepted


def full_features(pb, which):
    D, H, W = pb["dims"]
    labels = (np.arange(H * W).reshape(H, W) // 11 + 1)
    ft = dict(lam=LAM, adapt=dict(target=0.25, window=2, last=4, gain=2.0, range=(1e-3, 1e3)),
              post=dict(first=1, every=1, cubes=True), hist=dict(pilot=2, span=4.0),
              regions=dict(labels=labels, K=int(labels.max()), spectra=True), refresh_every=3)
    if which == "R":
        ft.update(robust=dict(nu=4, every=2, start=1, accumulate_from=2), pred=True)
    else:
        ft.update(noise=dict(group=np.arange(D) // 4, every=2, start=1, shape=1., rate=1., spaxels=NO.holes(H, W)))
    return CO.features_of(**ft)


def test_neutral_is_the_oracles_sweep_bit_for_bit():
    pb = problem()
    st, _ = chain_state(pb, lambda s: None)
    co = CO.Composed(pb, CO.features_of())
    assert np.isinf(co.st.var).sum() >= SHAPE[0] + 2 and not np.isnan(co.st.err).any()
    for s in range(1, SWEEPS + 1):
        O.mh_sweep(st, s)
        co.sweep(s)
        same_chain(co.st, st, "sweep %d" % s)
        np.testing.assert_array_equal(co.chain[s], st.params)
    assert 0 < st.accepted == int(co.acc.sum())


def test_robust_alone_is_robust_chain_bit_for_bit():
    pb = problem()
    kw = dict(nu=4, every=2, start=1, accumulate_from=2)
    st, chain = chain_state(pb, lambda s: RB.RobustChain(s, **kw))
    co = CO.Composed(pb, CO.features_of(robust=kw))
    for s in range(1, SWEEPS + 1):
        chain.sweep(s)
        co.sweep(s)
        same_chain(co.st, st, "sweep %d" % s)
    assert chain.count == co.robust.count == 1                    # draws after 1 and 3, the mean from 2 on
    np.testing.assert_array_equal(co.robust.mean, chain.mean)
    np.testing.assert_array_equal(co.robust.weights, chain.weights)
    with np.errstate(divide="ignore"):
        np.testing.assert_array_equal(1.0 / co.ivar, st.var)


def test_noise_alone_is_noise_chain_bit_for_bit():
    pb = problem()
    D, H, W = pb["dims"]
    kw = dict(group=np.arange(D) // 4, every=2, start=1, shape=1., rate=1., spaxels=NO.holes(H, W))
    st, chain = chain_state(pb, lambda s: NO.NoiseChain(s, **kw))
    co = CO.Composed(pb, CO.features_of(noise=kw))
    for s in range(1, SWEEPS + 1):
        chain.sweep(s)
        co.sweep(s)
        same_chain(co.st, st, "sweep %d" % s)
    assert chain.sweeps == co.noise.sweeps == [1, 3]
    np.testing.assert_array_equal(co.noise.scale(), chain.scale())
    np.testing.assert_array_equal(co.noise.tau_g, chain.tau_g)


def test_prior_alone_is_the_priors_sweep_bit_for_bit():
    pb = problem()
    st, _ = chain_state(pb, lambda s: None)
    co = CO.Composed(pb, CO.features_of(lam=LAM))
    for s in range(1, SWEEPS + 1):
        prior_oracle.mh_sweep(st, s, np.array(LAM))
        co.sweep(s)
        same_chain(co.st, st, "sweep %d" % s)
    plain = CO.Composed(pb, CO.features_of())
    plain.sweep(1)
    assert not np.array_equal(plain.chain[1], co.chain[1])          # (and the prior does matter)


def test_a_fixed_scale_map_is_test_gpu_adapts_sweep():
    """window = 0: the amplitudes of tests/test_gpu_adapt.py: oracle_sweep, the counters its counts."""
    pb = problem()
    H, W = pb["dims"][1:]
    scale = 10. ** np.random.default_rng(2).uniform(-1., 1., size=(H, W))
    st, _ = chain_state(pb, lambda s: None)
    state = CO.fresh_state(pb, CO.features_of())
    state["scale"] = scale
    ft = CO.features_of(adapt=dict(target=0.25, window=0, last=0, gain=2.0, range=(1e-3, 1e3)))
    co = CO.Composed(pb, ft, state)
    counts = np.zeros((H, W), dtype=np.int64)
    for s in (1, 2):
        for (y, x) in O.colour_order(st.mask, *st.fsf.shape):
            st.amp = np.array([0., 0.1 * scale[y, x], 0.1 * scale[y, x]])
            counts[y, x] += bool(O.mh_update(st, y, x, s))
        co.sweep(s)
        same_chain(co.st, st, "sweep %d" % s)
    np.testing.assert_array_equal(co.acc, counts)
    np.testing.assert_array_equal(co.scale, scale)
    assert (co.n_win, co.k) == (2, 0)


@pytest.mark.parametrize("which", ["R", "N"])
def test_everything_armed_continues_from_its_own_state(which):
    """Six sweeps in one object, and in six objects each made from the state of the one before: the same
    bits.  On the way every event of the order happens: adapt steps (after 2 and 4, none after 6), a
    refresh with a draw (3) and without (6), the histograms' freeze (2) and binned samples (3 ..)."""
    pb = problem()
    ft = full_features(pb, which)
    whole = CO.Composed(pb, ft)
    state, rows = None, []
    for s in range(1, 7):
        whole.sweep(s)
        part = CO.Composed(pb, ft, state)
        part.sweep(s)
        state = part.state()
        rows += part.rows
        same_chain(part.st, whole.st, "sweep %d" % s, accepted=False)       # (a state's count starts at 0)
        np.testing.assert_array_equal(part.counts, whole.counts)
    assert (whole.k, whole.n_win) == (2, 2) and whole.post["n"] == 6
    assert not np.array_equal(whole.scale, np.ones(whole.scale.shape))
    live = pb["mask"] == 1
    total = whole.hist["bins"].sum(axis=-1, dtype=np.int64) + whole.hist["tails"].sum(axis=-1, dtype=np.int64)
    assert (total[live] == 4).all() and (total[~live] == 0).all()
    np.testing.assert_array_equal(np.stack(rows), np.stack(whole.rows))
    mine, theirs = whole.state(), state
    for k in ("scale", "acc", "ivar"):
        np.testing.assert_array_equal(mine[k], theirs[k], err_msg=k)
    for k in ("map", "clean", "conv"):
        for a, b in zip(mine["post"][k], theirs["post"][k]):
            np.testing.assert_array_equal(a, b, err_msg=k)
    for k in ("bins", "tails", "range"):
        np.testing.assert_array_equal(mine["hist"][k], theirs["hist"][k], err_msg=k)
    for a, b in zip(mine["regions"]["spec"], theirs["regions"]["spec"]):
        np.testing.assert_array_equal(a, b)
    if which == "R":
        for a, b in zip(mine["pred"], theirs["pred"]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(mine["robust"]["mean"], theirs["robust"]["mean"])
        assert mine["robust"]["count"] == theirs["robust"]["count"] == 2          # draws 1, 3, 5; the mean from 2
    else:
        np.testing.assert_array_equal(mine["tau_g"], theirs["tau_g"])
        assert whole.noise.sweeps == [1, 3, 5]


@pytest.mark.parametrize("which", ["R", "N"])
def test_the_devices_arrays_in_the_oracles_place_change_nothing_when_they_are_its_own(which):
    pb = problem()
    ft = full_features(pb, which)
    a, b = CO.Composed(pb, ft), CO.Composed(pb, ft)
    for s in range(1, 4):
        a.sweep(s)
        b.updates(s)
        b.end_of_sweep(s, device=dict(params=a.st.params.copy(), err=a.st.err.copy()))
        same_chain(b.st, a.st, "sweep %d" % s)
        np.testing.assert_array_equal(a.ivar, b.ivar)
    if which == "R":
        for x, y in zip(a.state()["pred"], b.state()["pred"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("which", ["R", "N"])
def test_a_draw_before_the_refresh_shows_in_the_weights(which):
    """Sweep 3 is followed by a refresh and a draw.  From a state whose carried residual is a known way
    off the parameters' own (as tests/test_gpu_composed.py seeds the device), the draw taken before the
    refresh gives other weights, far beyond the 1e-12 the device is compared at; and even from the
    rounding creep of two sweeps alone it gives other bits."""
    pb = problem()
    ft = full_features(pb, which)
    for bump in (1e-3, 0.):
        ran = CO.Composed(pb, ft)
        ran.sweep(1)
        ran.sweep(2)
        state = ran.state()
        state["err"] = state["err"] + bump * np.max(np.abs(state["err"])) * \
            np.random.default_rng(3).uniform(-1., 1., size=state["err"].shape)
        right, wrong = CO.Composed(pb, ft, state), CO.Composed(pb, ft, state, draw_before_refresh=True)
        right.sweep(3)
        wrong.sweep(3)
        np.testing.assert_array_equal(right.st.params, wrong.st.params)
        np.testing.assert_array_equal(right.st.err, wrong.st.err)                 # (both end on the refreshed one)
        live = pb["i0"] != 0.
        rel = np.max(np.abs(wrong.ivar[live] / right.ivar[live] - 1.))
        print(which, "bump", bump, "weights: max rel change", rel)
        assert not np.array_equal(right.ivar, wrong.ivar)
        if bump:
            assert rel > 1e-6
