"""The accepted-move counter ("the ends of a launch"): a decision adds its
verdict to its own spaxel's entry of a map on the device, and the map is totalled into the
context's counter wherever the host reads the count -- at the end of mh_sweeps, per chain of
mh_sweeps_batch, in mh_accepted.  Every kernel family decides through the same code, so every
one of them must report the count it always did.  The reference here is independent of the
counter: an accepted proposal moves (c, w) of its spaxel (a Cauchy jump is never exactly zero),
a rejected one leaves them, so the count of a sweep equals the number of spaxels whose (c, w)
differ from the state before it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, H, W = 16, 22, 26
PARTS = [(0, (0, 12, 0, W)), (1, (12, H, 0, W))]


def inputs(uniform=False, depth=D):
    from oracle import deconv3d_oracle as O
    rng = np.random.default_rng(4321 + depth)
    fsf = rng.random((5, 5)) + 0.1
    fsf /= fsf.sum()
    lsf = O.gaussian_lsf_vector(depth, 0.9088)
    mask = np.ones((H, W))
    mask[rng.integers(0, H, 30), rng.integers(0, W, 30)] = 0
    mask[0, :] = mask[:, -1] = 0
    data = rng.normal(0., 1., (depth, H, W)) + 3.0 * np.exp(-0.5 * ((np.arange(depth) - depth / 2.) / 1.5) ** 2)[:, None, None]
    var = None if uniform else (0.5 + rng.random((depth, H, W))) ** 2
    max_b = np.array([data.max() / fsf.max(), depth - 1., float(depth)])
    init = max_b * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.3)
    return dict(depth=depth, fsf=fsf, lsf=lsf, mask=mask, data=data, var=var, max_b=max_b, init=init)


def engine(inp, options=None, seed=11, parts=None):
    from deconv3d_amd import _lib
    eng = _lib.Engine((inp["depth"], H, W), inp["fsf"].shape, options=options or {})
    eng.set_taps(inp["fsf"], inp["lsf"])
    if inp["var"] is None:
        eng.set_data(inp["data"], None, var_scalar=0.7, mask=inp["mask"])
    else:
        eng.set_data(inp["data"], inp["var"], mask=inp["mask"])
    if parts:
        eng.set_parts([r for _, r in parts], [ph for ph, _ in parts])
    eng.set_params(inp["init"])
    eng.mh_config(np.zeros(3), inp["max_b"], 0.1, float(inp["max_b"][0] ** 2), seed=seed, refresh_every=0)
    return eng


def moved(before, after, mask):
    """Unmasked spaxels whose (c, w) changed."""
    ch = (before[..., 1] != after[..., 1]) | (before[..., 2] != after[..., 2])
    assert not ch[mask != 1].any()
    return int(ch.sum())


@pytest.fixture(scope="module")
def reference():
    """Three sweeps of the default family, one at a time: the count of each and the states."""
    inp = inputs()
    counts, states = [], [inp["init"]]
    with engine(inp) as eng:
        for s in (1, 2, 3):
            counts.append(eng.mh_sweeps(1, s))
            states.append(eng.get_params())
    return inp, counts, states


def test_count_is_the_number_of_spaxels_that_moved(reference):
    inp, counts, states = reference
    for k, n in enumerate(counts):
        assert n == moved(states[k], states[k + 1], inp["mask"])
    assert 0 < counts[0] < int(inp["mask"].sum())     # both verdicts occur


FAMILIES = [{"mh_small": 0}, {"mh_small": 0, "mh_layers": 2}, {"mh_small": 0, "mh_layers": 3},
            {"mh_layers": 2}, {"mh_defer": 0}, {"mh_defer": 2}, {"mh_props": 0}, {"mh_zigzag": 0, "mh_small": 0},
            {"mh_nt_ivar": 1, "mh_small": 0, "mh_layers": 2}]


@pytest.mark.parametrize("options", FAMILIES, ids=lambda o: ",".join("%s=%d" % kv for kv in sorted(o.items())))
def test_every_family_reports_the_same_count(reference, options):
    inp, counts, states = reference
    with engine(inp, options) as eng:
        if "mh_zigzag" in options:   # another walk order: the sums round differently, the chain is another
            n = eng.mh_sweeps(1, 1)
            assert n == moved(inp["init"], eng.get_params(), inp["mask"])
            return
        assert eng.mh_sweeps(3, 1) == sum(counts)
        np.testing.assert_array_equal(eng.get_params(), states[3])


@pytest.mark.parametrize("kind", ["uniform variance", "320 channels", "600 channels", "two parts"])
def test_count_of_the_other_forms(kind):
    """Uniform variance, the 512-thread form, the z-blocked form with its deciding kernel, and a
    two-part context: the count against the spaxels that moved."""
    inp = inputs(uniform=kind == "uniform variance", depth={"320 channels": 320, "600 channels": 600}.get(kind, D))
    with engine(inp, {"mh_small": 0, "mh_layers": 2}, parts=PARTS if kind == "two parts" else None) as eng:
        n = eng.mh_sweeps(1, 1)
        assert n == moved(inp["init"], eng.get_params(), inp["mask"]) and n > 0


def test_count_starts_over_with_every_call_and_stays_readable(reference):
    inp, counts, _ = reference
    with engine(inp) as eng:
        assert eng.mh_sweeps(2, 1) == counts[0] + counts[1]
        assert eng.mh_accepted() == counts[0] + counts[1]
        assert eng.mh_accepted() == counts[0] + counts[1]      # reading it changes nothing
        assert eng.mh_sweeps(1, 3) == counts[2]                # a call reports its own sweeps
        assert eng.mh_accepted(reset=True) == counts[2]
        assert eng.mh_accepted() == 0
        assert eng.mh_sweeps(0, 4) == 0


def test_phase_stepping_accumulates_until_reset():
    """d3d_mh_phase does not zero the counter: it accumulates over the phases and the sweeps,
    whether or not the host reads it in between, and equals what mh_sweeps reports."""
    inp = inputs()
    with engine(inp, parts=PARTS) as eng:
        want = [eng.mh_sweeps(1, 1), eng.mh_sweeps(1, 2)]
        final = eng.get_params()
    with engine(inp, parts=PARTS) as eng:
        eng.mh_accepted(reset=True)
        seen, before = [], inp["init"]
        for s in (1, 2):
            for ph in (0, 1):
                eng.mh_phase(ph, s)
                seen.append(eng.mh_accepted())
            after = eng.get_params()
            assert seen[-1] - (seen[-3] if s == 2 else 0) == moved(before, after, inp["mask"])
            before = after
        assert seen == sorted(seen) and seen[1] == want[0] and seen[3] == want[0] + want[1]
        np.testing.assert_array_equal(before, final)
    with engine(inp, parts=PARTS) as eng:                      # ... and without reading in between
        for s in (1, 2):
            for ph in (0, 1):
                eng.mh_phase(ph, s)
        assert eng.mh_accepted() == want[0] + want[1]


@pytest.mark.parametrize("options", [{}, {"mh_small": 0}], ids=["small form", "k_mh_ws"])
def test_batched_chains_count_per_chain(options):
    from deconv3d_amd import _lib
    inp = inputs()
    seeds = (11, 12, 13)
    alone = []
    for sd in seeds:
        with engine(inp, options, seed=sd) as eng:
            alone.append((eng.mh_sweeps(2, 1), eng.get_params()))
    assert len({n for n, _ in alone}) > 1                      # the chains differ
    engs = [engine(inp, options, seed=sd) for sd in seeds]
    try:
        got = _lib.mh_sweeps_batch(engs, 2, 1)
        assert got == [n for n, _ in alone]
        for e, (n, p) in zip(engs, alone):
            np.testing.assert_array_equal(e.get_params(), p)
            assert e.mh_accepted() == n
    finally:
        for e in engs:
            e.close()
