"""
Convolution in the reference layout (d3d_convolve = d3d_stage_upload / _convolve / _download):
k_spectral_z and k_spatial_z<FS> (csrc/d3d_kernels.h) against the oracle at every FSF size, at
widths of one, two and three 64-column tiles (a second tile reads its halo from the left
neighbour), with every strip height; the route they replace (option zmajor = 0: transpose, slot
kernels, transpose back) and the taps that fall back to it; the ping-pong between the two staging
buffers.  The read-only option stage_path says which route a call took: STAGE_ZMAJOR and
STAGE_TRANSPOSE are asserted here.
"""
import functools

import numpy as np
import pytest

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O

pytestmark = pytest.mark.gpu

H = 9
FS_ALL = (3, 5, 7, 9, 11, 13, 15)
WIDTHS = (1, 63, 64, 65, 70, 129)


def lsf_of(D, kind):
    return {"muse": O.muse_like_lsf, "wide": lambda d: O.gaussian_lsf_vector(d, 3.0), "none": lambda d: None}[kind](D)


@functools.lru_cache(maxsize=4)
def cube_and_reference(D, W, fs, lsf_kind):
    """A normal-random cube and the oracle's convolution of it (shared, read-only)."""
    rng = np.random.default_rng(D * 7919 + W * 31 + fs)
    fsf = O.moffat_cropped(fs, 3.0, 2.5)
    assert np.array_equal(fsf, fsf[::-1]) and np.array_equal(fsf, fsf[:, ::-1])
    cube = rng.normal(size=(D, H, W))
    want = oracle(cube, fsf, lsf_of(D, lsf_kind))
    cube.setflags(write=False)
    want.setflags(write=False)
    return cube, fsf, want


def oracle(cube, fsf, lsf):
    return O.convolve_cube(cube, fsf, lsf) if lsf is not None else O.spatial_convolve(cube, fsf)


def convolve(cube, fsf, lsf, staged=False, **options):
    """(result, stage_path) of d3d_convolve, or of the three staged calls it is made of."""
    with _lib.Engine(cube.shape, fsf.shape, options=options) as eng:
        eng.set_taps(fsf, lsf)
        if staged:
            eng.stage_upload(cube)
            eng.stage_convolve()
            out = eng.stage_download()
        else:
            out = eng.convolve(cube)
        return out, eng.get_option("stage_path")


def assert_oracle(got, want):
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


# the full FS x W product without an LSF at 6 channels; with the MUSE-like LSF at 32 channels the
# corners of it that have a second and a third column tile
CASES = [(6, W, fs, "none") for fs in FS_ALL for W in WIDTHS] + \
        [(32, W, fs, "muse") for fs in (3, 11, 15) for W in (65, 129)]


@pytest.mark.parametrize("D,W,fs,lsf_kind", CASES)
def test_reference_layout_kernels_against_the_oracle_and_the_transposing_route(D, W, fs, lsf_kind):
    cube, fsf, want = cube_and_reference(D, W, fs, lsf_kind)
    lsf = lsf_of(D, lsf_kind)
    got, path = convolve(cube, fsf, lsf)
    assert path == _lib.STAGE_ZMAJOR
    assert_oracle(got, want)
    staged, path = convolve(cube, fsf, lsf, staged=True)
    assert path == _lib.STAGE_ZMAJOR
    np.testing.assert_array_equal(staged, got)           # d3d_convolve IS the three staged calls
    slots, path = convolve(cube, fsf, lsf, zmajor=0)
    assert path == _lib.STAGE_TRANSPOSE
    assert_oracle(slots, want)
    assert np.max(np.abs(slots - got)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("D,W,fs,lsf_kind", [(6, 70, 7, "none"), (32, 65, 11, "muse"), (6, 129, 15, "none")])
def test_strip_height_of_the_reference_layout_kernel_keeps_the_bits(D, W, fs, lsf_kind):
    """k_spatial_z always marches down: an output row meets its input rows top to bottom whatever
    the strip height (1, 3, all 9 rows, more rows than the cube has), so the bits stay."""
    cube, fsf, want = cube_and_reference(D, W, fs, lsf_kind)
    lsf = lsf_of(D, lsf_kind)
    default, _ = convolve(cube, fsf, lsf)
    for hy in (1, 3, 9, 50):
        got, path = convolve(cube, fsf, lsf, zmajor_hy=hy)
        assert path == _lib.STAGE_ZMAJOR
        assert_oracle(got, want)
        np.testing.assert_array_equal(got, default, err_msg="zmajor_hy = %d" % hy)


def fsf_x_only(fs, rng):
    a = rng.random((fs, fs // 2 + 1))
    f = np.hstack([a, a[:, -2::-1]])
    return f / f.sum()


@pytest.mark.parametrize("what", ["y_only", "none", "non-square", "depth 30", "wide lsf"])
def test_taps_the_reference_layout_kernels_do_not_take_fall_back(what):
    """An FSF without both mirror symmetries, a non-square FSF, an LSF at a depth that is no power
    of two and an LSF wider than +-8 channels: the transposing route, by stage_path and to the
    oracle."""
    rng = np.random.default_rng(5)
    D, W, lsf_kind = 32, 65, "muse"
    fsf = O.moffat_cropped(7, 3.0, 2.5)
    if what == "y_only":
        fsf = np.ascontiguousarray(fsf_x_only(7, rng).T)
        assert np.array_equal(fsf, fsf[::-1]) and not np.array_equal(fsf, fsf[:, ::-1])
    elif what == "none":
        fsf = rng.random((7, 7))
        fsf /= fsf.sum()
    elif what == "non-square":
        fsf = np.ascontiguousarray(O.moffat_cropped(7, 3.0, 2.5)[2:5])      # 3 x 7, xy-symmetric
        assert np.array_equal(fsf, fsf[::-1]) and np.array_equal(fsf, fsf[:, ::-1])
    elif what == "depth 30":
        D = 30
    else:
        D, lsf_kind = 64, "wide"
    lsf = lsf_of(D, lsf_kind)
    cube = rng.normal(size=(D, H, W))
    with _lib.Engine(cube.shape, fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        got = eng.convolve(cube)
        assert eng.get_option("stage_path") == _lib.STAGE_TRANSPOSE
        if what == "wide lsf":
            assert eng.get_option("lsf_fits") == 0
    assert_oracle(got, oracle(cube, fsf, lsf))


@pytest.mark.parametrize("D,lsf_kind", [(32, "muse"), (6, "none")])
@pytest.mark.parametrize("zmajor", [1, 0])
def test_two_staged_convolutions_after_one_upload(D, lsf_kind, zmajor):
    """d3d_stage_convolve works in place on the staging buffer: with an LSF the spatial pass lands
    there by itself (stage -> stage2 -> stage), without one it is copied back from stage2.  A
    second call convolves the first one's result."""
    cube, fsf, once = cube_and_reference(D, 65, 11, lsf_kind)
    lsf = lsf_of(D, lsf_kind)
    twice = oracle(once, fsf, lsf)
    with _lib.Engine(cube.shape, fsf.shape, options={"zmajor": zmajor}) as eng:
        eng.set_taps(fsf, lsf)
        eng.stage_upload(cube)
        eng.stage_convolve()
        eng.stage_convolve()
        got = eng.stage_download()
        assert eng.get_option("stage_path") == (_lib.STAGE_ZMAJOR if zmajor else _lib.STAGE_TRANSPOSE)
        assert_oracle(got, twice)
        assert_oracle(eng.stage_download(), twice)       # a download leaves the buffer alone
