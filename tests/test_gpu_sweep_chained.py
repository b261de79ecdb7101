"""
Lattice-row strips chained from colour row to colour row (option mh_strip_order = 2, DESIGN.md section 3,
deconv3d_amd/csrc/d3d_strip_order.h): one fork per sweep, the strips of consecutive colour rows ordered
by events, one join at the sweep's end.  Same workgroup, same window, same arithmetic: the chained
chain is the unsplit chain (mh_strips = 1) BIT FOR BIT -- parameters, log ratios, accepted count and
the carried residual as 64-bit patterns -- and so is the joined one (mh_strip_order = 1).  Every run is
3 sweeps in ONE call, so that the wrap of the colour rows is crossed between two chained sweeps, then 2
more in a second call, which finds the layers the first left pending.

The problems are those of tests/test_gpu_sweep_strips.py (the smallest that reach each kernel form: see
there), plus its masked cube with one whole colour row masked.  `mh_strips_on` and `mh_strip_order_on`
are asserted for every run.

Test option mh_strip_lag = s + 1 puts a delay kernel of at most 200 us in front of strip s at every
colour row.  With every event in place the chain does not change whichever strip is late; a missing
edge lets the late strip's neighbour run into what it has not finished.

What follows a sweep -- a snapshot of a streamed chain, a from-scratch residual -- runs on the context's
stream behind the sweep-end join: compared with the unsplit run's, bit for bit.
"""
import functools

import numpy as np
import pytest

from tests import test_gpu_sweep_strips as SS

pytestmark = pytest.mark.gpu

FIRST, SECOND = 3, 2     # sweeps of the two calls
JOINED, CHAINED = 1, 2


@functools.lru_cache(maxsize=None)
def problem(name):
    if name != "masked_row":
        return SS.problem(name)
    # the masked 30 x 30 cube of 5 x 5 taps with colour row 1 -- the cube rows 1, 6, 11, ... -- fully masked
    p = dict(SS.problem("masked"))
    mask = p["mask"].copy()
    mask[1::5, :] = 0
    p["mask"] = mask
    return p


def run(name, strips, order=0, lag=0):
    """The state after FIRST sweeps in one call and after SECOND more in another (streamed: with the arrays)."""
    p = problem(name)
    p = dict(p, options=dict(p["options"], mh_strip_order=order, mh_strip_lag=lag))
    with SS.engine(p, strips) as eng:
        assert eng.get_option("mh_strips_on") == (strips if strips > 1 else 0)
        assert eng.get_option("mh_strip_order_on") == (order if strips > 1 else 0)
        out = ()
        for first, n in ((1, FIRST), (1 + FIRST, SECOND)):
            extra = ()
            if p["streamed"]:
                H, W = p["dims"][1:]
                ch, dl = np.zeros((first + n, H, W, 3)), np.zeros((first + n, H, W))
                acc = eng.mh_sweeps(n, first, keep_one_in=1, chain=ch, dlog=dl)
                extra = (ch[first:], dl[first:])
            else:
                acc = eng.mh_sweeps(n, first)
            out += SS.state(eng, acc, extra)
        return out


@functools.lru_cache(maxsize=None)
def unsplit(name):
    out = run(name, 1)
    for a in out:
        a.setflags(write=False)
    assert np.isfinite(out[0]).all() and out[2][0] > 0   # a chain that moves
    return out


# fill, the 512-thread form, zfill (z-blocked), a fully masked colour row, the smoothness prior, the
# non-temporal policy, one and three pending layers
PROBLEMS = ["c16", "c258", "zb_full", "masked_row", "prior", "c16_nt", "c16_one_layer", "c16_three_layers"]


@pytest.mark.parametrize("strips", [2, 3, 4])
@pytest.mark.parametrize("name", PROBLEMS)
def test_chained_chain_is_the_unsplit_and_the_joined_chain_bit_for_bit(name, strips):
    chained = run(name, strips, CHAINED)
    SS.assert_same_bits(chained, unsplit(name))
    SS.assert_same_bits(run(name, strips, JOINED), chained)


@pytest.mark.parametrize("strips", [2, 3, 4])
@pytest.mark.parametrize("name", ["c16", "zb_full"])
def test_a_late_strip_does_not_change_the_chain(name, strips):
    for lag in range(1, strips + 1):
        SS.assert_same_bits(run(name, strips, CHAINED, lag), unsplit(name))


@pytest.mark.parametrize("name", ["streamed", "refresh"])
def test_what_follows_a_sweep_sees_the_joined_strips(name):
    """keep_one_in = 1: every sweep's snapshot; refresh_every = 2: a from-scratch residual mid-run."""
    SS.assert_same_bits(run(name, 3, CHAINED), unsplit(name))
    SS.assert_same_bits(run(name, 3, CHAINED, lag=1), unsplit(name))
