"""
Lattice-row strips of a colour row (option mh_strips): the strips of a colour
row run the colour's kernel on ranges of its work list, on streams of their own between one fork
and one join per colour row.  The same workgroup does the same arithmetic on the same window, so a
chain run in 2, 3 or 4 strips is the unsplit chain (mh_strips = 1) BIT FOR BIT -- parameters, log
ratios, accepted count and the carried residual, compared as 64-bit patterns -- and two equal runs
of the 3-strip chain are equal: a race between strips shows up as a difference there.

Each problem is the smallest that still has what can go wrong (see PROBLEMS).  Unless a problem
says otherwise mh_layers = 2 and mh_small = 0 are forced, so that the small cubes take the k_mh_ws
variants the strips apply to, and `mh_strips_on` is asserted.  The unsplit reference of a problem is
computed once and shared.
"""
import functools

import numpy as np
import pytest

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O

pytestmark = pytest.mark.gpu

SWEEPS = 3
FORCE = {"mh_layers": 2, "mh_small": 0}


def gaussian_taps(fh, fw, sigma=1.1):
    y = np.exp(-0.5 * ((np.arange(fh) - (fh - 1) / 2.0) / sigma) ** 2)
    x = np.exp(-0.5 * ((np.arange(fw) - (fw - 1) / 2.0) / (1.2 * sigma)) ** 2)
    t = np.outer(y, x)
    return t / t.sum()


def masked_30x30(rng):
    """30 % masked at random; cube rows 0 .. 4 -- lattice row 0 of EVERY colour row of a 5 x 5 FSF --
    fully masked: with four strips strip 0 (the virtual row above the cube and lattice row 0) holds
    only virtual positions; colour (2, 3) fully masked: colour row 2 has an inactive colour."""
    mask = (rng.random((30, 30)) >= 0.3).astype(np.float64)
    mask[0:5, :] = 0
    mask[2::5, 3::5] = 0
    return mask


@functools.lru_cache(maxsize=None)
def problem(name):
    """dims, taps, data, variance (cube or scalar), mask, start, options, and what else is on."""
    base = {"options": dict(FORCE), "prior": None, "refresh_every": 0, "streamed": False, "var_scalar": None}
    seed = {"c16": 1, "c16_default_small": 1, "odd": 2, "masked": 3, "masked_uniform": 3, "masked_nt": 3,
            "zb": 4, "prior": 5, "refresh": 5, "streamed": 5, "too_few_rows": 6}[name]
    rng = np.random.default_rng(9000 + seed)
    if name in ("c16", "c16_default_small"):
        # 23 x 23 = 529 windows per colour: fills the chip (>= 512 workgroups) without forcing
        D, H, W, fh, fw = 16, 69, 69, 3, 3
        if name == "c16_default_small":
            base["options"] = {"mh_layers": 2}
    elif name == "odd":
        # odd depth (a padding channel), FSF not square, H and W no multiples of the period,
        # virtual rows outside the cube
        D, H, W, fh, fw = 15, 40, 45, 3, 7
    elif name.startswith("masked"):
        D, H, W, fh, fw = 128, 30, 30, 5, 5
        if name == "masked_uniform":
            base["var_scalar"] = 0.09
        if name == "masked_nt":
            base["options"]["mh_nt_ivar"] = 1  # write-through stores, non-temporal 1/variance
    elif name == "zb":
        D, H, W, fh, fw = 640, 12, 12, 3, 3    # the z-blocked form + k_mh_zdecide
    elif name in ("prior", "refresh", "streamed"):
        D, H, W, fh, fw = 128, 30, 30, 5, 5
        if name == "prior":
            base["prior"] = [4.0, 0.5, 2.0]
        if name == "refresh":
            base["refresh_every"] = 2           # a from-scratch residual mid-run
        if name == "streamed":
            base["streamed"] = True
    elif name == "too_few_rows":
        D, H, W, fh, fw = 128, 12, 30, 5, 5    # lattice rows -1 .. 2: four strips would hold one each
    else:
        raise KeyError(name)
    fsf = gaussian_taps(fh, fw)
    lsf = O.muse_like_lsf(D)
    truth = np.dstack((1.0 + 9.0 * rng.random((H, W)), D * (0.2 + 0.6 * rng.random((H, W))),
                       0.6 + 2.0 * rng.random((H, W))))
    if name.startswith("masked"):
        mask = masked_30x30(rng)
    else:
        mask = np.ones((H, W))
        mask[H // 3, W // 2] = mask[H - 1, 0] = 0
    data = rng.normal(0.0, 0.3, size=(D, H, W)) + truth[..., 0][None] * 0.05
    var = 0.09 * (0.5 + rng.random((D, H, W)))
    init = truth * (0.8 + 0.4 * rng.random((H, W, 3)))
    base.update(dims=(D, H, W), fsf=fsf, lsf=lsf, data=data, var=var, mask=mask, init=init,
                mn=np.array([0.0, 0.0, 0.3]), mx=np.array([30.0, D - 1.0, 6.0]))
    return base


def engine(p, strips, seed=77):
    eng = _lib.Engine(p["dims"], p["fsf"].shape, options=dict(p["options"], mh_strips=strips))
    eng.set_taps(p["fsf"], p["lsf"])
    if p["var_scalar"] is not None:
        eng.set_data(p["data"], None, var_scalar=p["var_scalar"], mask=p["mask"])
    else:
        eng.set_data(p["data"], p["var"], mask=p["mask"])
    eng.set_params(p["init"])
    eng.mh_config(p["mn"], p["mx"], 0.1, 900.0, seed=seed, refresh_every=p["refresh_every"])
    if p["prior"] is not None:
        eng.prior_begin(p["prior"])
    return eng


def state(eng, acc, extra=()):
    return (eng.get_params(), eng.get_dlog(), np.array([acc], dtype=np.int64),
            eng.download_slot(_lib.SLOT_ERR)) + tuple(extra)


def chain(name, strips, expect_on=None):
    """SWEEPS sweeps from first_sweep = 1; the state afterwards (and the streamed arrays)."""
    p = problem(name)
    with engine(p, strips) as eng:
        if expect_on is None:
            expect_on = strips if strips > 1 else 0
        assert eng.get_option("mh_strips_on") == expect_on
        extra = ()
        if p["streamed"]:
            H, W = p["dims"][1:]
            ch, dl = np.zeros((SWEEPS + 1, H, W, 3)), np.zeros((SWEEPS + 1, H, W))
            acc = eng.mh_sweeps(SWEEPS, 1, keep_one_in=1, chain=ch, dlog=dl)
            extra = (ch, dl)
        else:
            acc = eng.mh_sweeps(SWEEPS, 1)
        return state(eng, acc, extra)


@functools.lru_cache(maxsize=None)
def unsplit(name):
    out = chain(name, 1)
    for a in out:
        a.setflags(write=False)
    assert np.isfinite(out[0]).all() and out[2][0] > 0   # a chain that moves
    return out


def assert_same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint64 if g.itemsize == 8 else np.uint8),
                                      np.ascontiguousarray(w).view(np.uint64 if w.itemsize == 8 else np.uint8))


PROBLEMS = ["c16", "c16_default_small", "odd", "masked", "masked_uniform", "masked_nt", "prior", "refresh",
            "streamed"]


@pytest.mark.parametrize("strips", [2, 3, 4])
@pytest.mark.parametrize("name", PROBLEMS)
def test_stripped_chain_is_the_unsplit_chain_bit_for_bit(name, strips):
    assert_same_bits(chain(name, strips), unsplit(name))


@pytest.mark.parametrize("name", PROBLEMS + ["zb"])
def test_two_equal_stripped_runs_are_equal(name):
    """Two runs in one process: a race between strips is a difference between equal runs."""
    strips = 2 if name == "zb" else 3
    first = chain(name, strips)
    assert_same_bits(chain(name, strips), first)
    assert_same_bits(first, unsplit(name))


def test_z_blocked_form_in_two_strips():
    """640 channels: k_mh_ws<..., ZBK> on (window, block) workgroups + k_mh_zdecide, every strip its
    share of the blocks' wave sums."""
    p = problem("zb")
    with engine(p, 2) as eng:
        assert eng.get_option("mh_zblocks") == 1 and eng.get_option("lsf_fits") == 1
    assert_same_bits(chain("zb", 2), unsplit("zb"))


def test_unforced_strips_need_a_chip_filling_launch():
    """Automatic (mh_strips = 0): never on a latency-bound problem, whatever the build's default is."""
    with engine(problem("masked"), 0) as eng:
        assert eng.get_option("mh_strips_on") == 0


def test_too_few_lattice_rows_fall_back_to_whole_launches():
    """5 x 5 taps on 12 rows: lattice rows -1 .. 2.  Four strips would hold one row each: refused
    (mh_strips_on == 0), the chain is the unsplit one; two strips of two rows run."""
    assert_same_bits(chain("too_few_rows", 4, expect_on=0), unsplit("too_few_rows"))
    assert_same_bits(chain("too_few_rows", 2), unsplit("too_few_rows"))


def test_untouched_paths_read_the_strip_major_lists():
    """After a stripped run: one colour class through d3d_mh_colour (k_mh on the REAL spaxels of the
    list) and a d3d_mh_sweeps_batch of two contexts (the whole list in one launch) equal the
    unsplit contexts'."""
    p = problem("masked")
    outs = {}
    for strips in (1, 3):
        engs = [engine(p, strips, seed=77 + r) for r in range(2)]
        try:
            accs = [e.mh_sweeps(SWEEPS, 1) for e in engs]
            assert engs[0].get_option("mh_strips_on") == (strips if strips > 1 else 0)
            for col in (0, 7, 13, 24):      # (13 = colour (2, 3): fully masked, nothing to do)
                engs[0].mh_colour(col, SWEEPS + 1)
            after_colour = state(engs[0], accs[0])
            engs[0].mh_phase(0, SWEEPS + 1)     # stepping by phase: whole colour launches
            after_colour += state(engs[0], accs[0])
            accs = _lib.mh_sweeps_batch(engs, 2, first_sweep=SWEEPS + 2)
            outs[strips] = after_colour + state(engs[0], accs[0]) + state(engs[1], accs[1])
        finally:
            for e in engs:
                e.close()
    assert_same_bits(outs[3], outs[1])
