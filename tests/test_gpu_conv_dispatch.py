"""
Every kernel family the convolution dispatcher (csrc/d3d_spatial.hip) can pick, not only the ones
the default options reach: each run is checked against the oracle (O.convolve_cube /
O.spatial_convolve / O.forward_full, 1e-12 of the largest reference value), against the other
device paths of the same sum (1e-13 where the order of the sum differs, bit for bit where it
does not) and -- through the read-only options spatial_path / spectral_path -- against the
kernel family the dispatcher is expected to take, so that a rule that silently falls through to
another kernel fails here.

Every case convolves a normal-random cube slot to slot (d3d_convolve_slots) and runs the forward
model and the residual (the ``data - sim`` epilogue) with two masked spaxels.

Shapes: W = 2 FS + 2 gives x strips at the left border, at the right border and in the interior
and is no multiple of the 3 or 4 columns of a strip; H = 13 at 5 rows per strip gives strips of
5, 5 and 3 rows, the odd one marching upward in the xy-symmetric kernel; 128 channels are one
wavefront per strip (the UNI instantiations), 30 channels 17 strips per workgroup with idle
lanes, 2 and 200 channels the extremes of the 256-thread kernels.

Where each family code is asserted:

| code                         | test                                                          |
|------------------------------|---------------------------------------------------------------|
| SPATIAL_CONV_ROWS            | test_one_pass_kernel_codes                                    |
| SPATIAL_CONV_ROWS_ZB         | test_one_pass_kernel_codes                                    |
| SPATIAL_CONV_ROWS_LSF        | test_one_pass_kernel_codes                                    |
| SPATIAL_MARCH_XY             | test_march_kernel_of_every_symmetry_class, test_spatial_mode  |
| SPATIAL_MARCH_X              | test_march_kernel_of_every_symmetry_class, test_spatial_mode  |
| SPATIAL_MARCH                | test_march_kernel_of_every_symmetry_class, test_spatial_mode  |
| SPATIAL_SEP                  | test_outer_product_fsf_without_symmetry                       |
| SPATIAL_SEP_LSF              | test_outer_product_fsf_without_symmetry                       |
| SPATIAL_TILE + 256           | test_spatial_mode, test_stand_alone_spectral_pass             |
| SPATIAL_TILE + 512, + 1024   | test_spatial_nt_runs_the_wide_tile_kernels                    |
| SPATIAL_GENERIC              | test_generic_and_deep_kernels                                 |
| SPATIAL_DEEP                 | test_generic_and_deep_kernels                                 |
| SPECTRAL_BLOCKS              | test_stand_alone_spectral_pass                                |
| SPECTRAL_DENSE               | test_stand_alone_spectral_pass                                |
| SPECTRAL_TAPS                | test_stand_alone_spectral_pass                                |
| SPECTRAL_DEEP                | test_generic_and_deep_kernels                                 |
| STAGE_ZMAJOR, STAGE_TRANSPOSE| tests/test_gpu_zmajor.py                                      |

(SPATIAL_MARCH_EXPERIMENT and SPECTRAL_SHFL exist only in a `make EXPERIMENTS=1` build.)
"""
import functools
import itertools

import numpy as np
import pytest

from deconv3d_amd import _lib
from oracle import deconv3d_oracle as O

pytestmark = pytest.mark.gpu

H13, HY = 13, 5
FS_ALL = (3, 5, 7, 9, 11, 13, 15)
FS_D = [(fs, D) for fs in FS_ALL for D in (128, 30)] + [(11, 2), (11, 200)]


def fsf_of(kind, fs):
    """An FSF of exactly the given symmetry class (checked bit for bit below)."""
    rng = np.random.default_rng(500 + fs)
    if kind == "xy":
        f = O.moffat_cropped(fs, 3.0, 2.5)
    elif kind in ("x_only", "y_only"):
        a = rng.random((fs, fs // 2 + 1))
        f = np.hstack([a, a[:, -2::-1]])
        f = f / f.sum()
        if kind == "y_only":
            f = f.T
    elif kind == "none":
        f = rng.random((fs, fs))
        f = f / f.sum()
    elif kind == "sep_asym":
        u = 1.0 + np.arange(fs)
        v = 3.0 + 0.5 * np.arange(fs)[::-1]
        f = np.outer(u / u.sum(), v / v.sum())
    else:
        raise KeyError(kind)
    f = np.ascontiguousarray(f)
    symx, symy = np.array_equal(f, f[:, ::-1]), np.array_equal(f, f[::-1])
    assert f.shape == (fs, fs)
    assert (symx, symy) == {"xy": (True, True), "x_only": (True, False), "y_only": (False, True),
                            "none": (False, False), "sep_asym": (False, False)}[kind]
    return f


class FSF(object):
    """A hashable FSF image (problem() is cached by its arguments)."""

    def __init__(self, image):
        self.image = np.ascontiguousarray(image)

    def __hash__(self):
        return hash(self.image.tobytes())

    def __eq__(self, other):
        return isinstance(other, FSF) and np.array_equal(self.image, other.image)


@functools.lru_cache(maxsize=4)
def problem(kind, fs, D, H=H13, W=None, lsf_kind="muse"):
    """Inputs and the oracle's answers, computed once and shared (read-only)."""
    W = 2 * fs + 2 if W is None else W
    rng = np.random.default_rng(fs * 100003 + D * 101 + H * 7 + W)
    fsf = fsf_of(kind, fs) if isinstance(kind, str) else kind.image   # (an FSF given as such)
    lsf = O.muse_like_lsf(D) if lsf_kind == "muse" else None
    cube = rng.normal(size=(D, H, W))
    params = np.dstack((1 + 9 * rng.random((H, W)), D * (0.2 + 0.6 * rng.random((H, W))),
                        0.8 + 3 * rng.random((H, W))))
    mask = np.ones((H, W))
    mask[min(3, H - 1), min(5, W - 1)] = mask[H - 1, 0] = 0
    data = rng.normal(size=(D, H, W))
    conv = O.convolve_cube(cube, fsf, lsf) if lsf is not None else O.spatial_convolve(cube, fsf)
    sim = O.forward_full((D, H, W), params, mask, fsf, lsf)
    p = dict(shape=(D, H, W), fsf=fsf, lsf=lsf, cube=cube, params=params, mask=mask, data=data,
             conv=conv, sim=sim, err=data - sim)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def run(p, **options):
    """Slot-to-slot convolution, forward model and residual of a problem on a fresh context:
    the three cubes and the paths the dispatcher took."""
    opts = {"conv_rows": 0, "march_hy": HY}
    opts.update(options)
    with _lib.Engine(p["shape"], p["fsf"].shape, options=opts) as eng:
        eng.set_taps(p["fsf"], p["lsf"])
        eng.upload_slot(_lib.SLOT_TMP0, p["cube"])
        eng.convolve_slots(_lib.SLOT_TMP0, _lib.SLOT_SIM)
        out = dict(conv=eng.download_slot(_lib.SLOT_SIM))
        paths = [eng.get_option("spatial_path")]
        out["spectral_path"] = eng.get_option("spectral_path")
        eng.set_data(p["data"], mask=p["mask"])
        eng.set_params(p["params"])
        out["sim"] = eng.forward()
        paths.append(eng.get_option("spatial_path"))
        out["err"] = eng.residual()
        paths.append(eng.get_option("spatial_path"))
    assert paths[0] == paths[1] == paths[2], paths       # one dispatch rule for the three calls
    out["spatial_path"] = paths[0]
    return out


CUBES = ("conv", "sim", "err")


def assert_oracle(p, r):
    for k in CUBES:
        assert np.max(np.abs(r[k] - p[k])) <= 1e-12 * np.max(np.abs(p[k])), k


def assert_close(p, a, b):
    for k in CUBES:
        assert np.max(np.abs(a[k] - b[k])) <= 1e-13 * np.max(np.abs(p[k])), k


def assert_same_bits(a, b):
    for k in CUBES:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("fs,D", FS_D)
@pytest.mark.parametrize("kind,path", [("xy", _lib.SPATIAL_MARCH_XY), ("x_only", _lib.SPATIAL_MARCH_X),
                                       ("y_only", _lib.SPATIAL_MARCH), ("none", _lib.SPATIAL_MARCH)])
def test_march_kernel_of_every_symmetry_class(kind, path, fs, D):
    """launch_march_fs picks k_spatial_march<SYMX, SYMY> from fsf_symx / fsf_symy alone: an FSF
    mirrored in x only runs the x-symmetric kernel, one mirrored in y only (or not at all) the
    kernel without symmetry."""
    p = problem(kind, fs, D)
    r = run(p)
    assert r["spatial_path"] == path
    assert_oracle(p, r)


@pytest.mark.parametrize("fs,D", FS_D)
@pytest.mark.parametrize("variant", ["sep", "sep_lsf", "2d"])
def test_outer_product_fsf_without_symmetry(variant, fs, D):
    """u v^T of two different ramps: the separable march (with the LSF in the same pass where the
    depth allows it: a power of two within a wavefront), and the 2-D march without symmetry when
    the outer product is not to be used (spatial_sep = 0); the three agree to rounding."""
    p = problem("sep_asym", fs, D)
    options, path = {"sep": ({"sep_fuse": 0}, _lib.SPATIAL_SEP),
                     "sep_lsf": ({}, _lib.SPATIAL_SEP_LSF if D == 128 else _lib.SPATIAL_SEP),
                     "2d": ({"spatial_sep": 0}, _lib.SPATIAL_MARCH)}[variant]
    r = run(p, **options)
    assert r["spatial_path"] == path
    assert_oracle(p, r)


@pytest.mark.parametrize("D", [128, 30])
@pytest.mark.parametrize("fs", [7, 11])
@pytest.mark.parametrize("kind", ["xy", "x_only"])
def test_spatial_mode(kind, fs, D):
    """spatial_mode 0 tile kernel, 1 march without symmetry, 2 march with the symmetries the FSF
    has, 3 march with the x symmetry only (also for an FSF that has both)."""
    p = problem(kind, fs, D)
    want = {0: _lib.SPATIAL_TILE + 256, 1: _lib.SPATIAL_MARCH,
            2: _lib.SPATIAL_MARCH_XY if kind == "xy" else _lib.SPATIAL_MARCH_X, 3: _lib.SPATIAL_MARCH_X}
    runs = {}
    for mode in (0, 1, 2, 3):
        runs[mode] = run(p, spatial_mode=mode)
        assert runs[mode]["spatial_path"] == want[mode], mode
        assert_oracle(p, runs[mode])
    for a, b in itertools.combinations((0, 1, 2, 3), 2):
        assert_close(p, runs[a], runs[b])


@pytest.mark.parametrize("kind,fs,options,path", [
    ("xy", 11, {}, _lib.SPATIAL_MARCH_XY),
    ("sep_asym", 7, {"sep_fuse": 0}, _lib.SPATIAL_SEP),
    ("sep_asym", 7, {}, _lib.SPATIAL_SEP_LSF)])
def test_scheduling_options_keep_the_bits_where_they_keep_the_order(kind, fs, options, path):
    """xcd_remap, alt_dir, stagger and march_hy at 128 channels.

    An output row's value is the sum of its tap rows' contributions in the order the march meets
    the input rows.  xcd_remap only renumbers the workgroups and stagger only delays them: the
    bits stay.  A strip walks down, so with alt_dir = 0 every output row meets its input rows
    top to bottom whatever march_hy is: the bits stay.  alt_dir = 1 walks odd strips of the
    xy-symmetric kernel upward (k_spatial_march: dir = -1), reversing the order of those rows'
    sums: equal to rounding only -- unless the cube is ONE strip (march_hy >= H), which has no
    odd strip.  k_spatial_sep and k_spatial_sep_lsf never read alt_dir: all bits stay."""
    p = problem(kind, fs, 128)

    def go(**more):
        opts = dict(options)
        opts.update(more)
        r = run(p, **opts)
        assert r["spatial_path"] == path
        assert_oracle(p, r)
        return r

    default = go()                                       # xcd_remap 1, alt_dir 1, stagger 0, 5 rows
    down = go(alt_dir=0)
    for xcd, alt, stagger in itertools.product((0, 1), (0, 1), (0, 3)):
        assert_same_bits(go(xcd_remap=xcd, alt_dir=alt, stagger=stagger), default if alt else down)
    for hy in (1, 5, 13, 40):                            # 40: one strip taller than the cube
        assert_same_bits(go(march_hy=hy, alt_dir=0), down)
    for hy in (13, 40):
        assert_same_bits(go(march_hy=hy), down)          # one strip: nothing walks upward
    assert_close(p, go(march_hy=1), down)
    assert_close(p, default, down)
    if path != _lib.SPATIAL_MARCH_XY:
        assert_same_bits(default, down)
        assert_same_bits(go(march_hy=1), down)


# workgroups of the march launch at 128 channels (4 strips each), FS = 11 (3 columns per strip),
# 5 rows per strip: nb = ceil(ceil(W / 3) * ceil(H / 5) / 4)
REMAP_FOOTPRINTS = [
    (5, 8),      # 3 x 1 strips: nb = 1
    (13, 24),    # 8 x 3 strips: nb = 6, fewer workgroups than XCDs
    (40, 24),    # 8 x 8 strips: nb = 16, a multiple of 8
    (23, 26),    # 9 x 5 = 45 strips: nb = 12 = 8 + 4, the last workgroup holds one strip
]


@pytest.mark.parametrize("H,W", REMAP_FOOTPRINTS)
@pytest.mark.parametrize("kind,options,path", [
    ("xy", {}, _lib.SPATIAL_MARCH_XY),
    ("x_only", {}, _lib.SPATIAL_MARCH_X),
    ("sep_asym", {"sep_fuse": 0}, _lib.SPATIAL_SEP),
    ("sep_asym", {}, _lib.SPATIAL_SEP_LSF)])
def test_xcd_remap_is_a_bijection_at_every_grid_size(kind, options, path, H, W):
    """The remap of workgroups to strips is index arithmetic of its own in every march kernel: one
    that drops or repeats a strip leaves rows of the output unwritten (zero) or written twice --
    either fails the oracle -- and the remapped launch gives the bits of the plain one."""
    p = problem(kind, 11, 128, H, W)
    runs = []
    for remap in (1, 0):
        runs.append(run(p, xcd_remap=remap, **options))
        assert runs[-1]["spatial_path"] == path
        assert_oracle(p, runs[-1])
    assert_same_bits(runs[0], runs[1])


@pytest.mark.parametrize("D,kind,fs,W,nt,path", [
    (128, "none", 5, 12, 512, _lib.SPATIAL_TILE + 512),
    (128, "none", 5, 12, 1024, _lib.SPATIAL_TILE + 1024),
    (30, "none", 5, 12, 512, _lib.SPATIAL_TILE + 512),
    (30, "none", 5, 12, 1024, _lib.SPATIAL_TILE + 1024),
    (520, "x_only", 11, 24, 0, _lib.SPATIAL_TILE + 512)])    # the march is built for 256 threads
def test_spatial_nt_runs_the_wide_tile_kernels(D, kind, fs, W, nt, path):
    """k_spatial<512> and k_spatial<1024>, which the defaults reach only beyond 512 channels; at
    520 channels the x-symmetric FSF has no march kernel and takes the tile kernel."""
    p = problem(kind, fs, D, H13, W)
    r = run(p, spatial_nt=nt)
    assert r["spatial_path"] == path
    assert_oracle(p, r)
    if nt:
        r256 = run(p, spatial_mode=0)
        assert r256["spatial_path"] == _lib.SPATIAL_TILE + 256
        assert_same_bits(r, r256)        # a thread's sum does not depend on the workgroup's size


@pytest.mark.parametrize("D,options,path", [
    (64, {}, _lib.SPECTRAL_DENSE), (128, {}, _lib.SPECTRAL_DENSE),
    (64, {"spectral_dense": 0}, _lib.SPECTRAL_BLOCKS), (128, {"spectral_dense": 0}, _lib.SPECTRAL_BLOCKS),
    (64, {"spectral_dense": 0, "spectral_blocks": 0}, _lib.SPECTRAL_TAPS),
    (128, {"spectral_dense": 0, "spectral_blocks": 0}, _lib.SPECTRAL_TAPS),
    (100, {}, _lib.SPECTRAL_BLOCKS), (255, {}, _lib.SPECTRAL_BLOCKS),
    (100, {"spectral_blocks": 0}, _lib.SPECTRAL_TAPS), (255, {"spectral_blocks": 0}, _lib.SPECTRAL_TAPS)])
def test_stand_alone_spectral_pass(D, options, path):
    """The MUSE-like LSF with a 1 x 1 FSF (no spatial kernel applies the LSF itself): the dense
    one-wavefront kernel, the 128-channel blocks and the tap list, each against the oracle and
    against the default."""
    p = problem(FSF(np.ones((1, 1))), 1, D, 7, 9)
    r = run(p, **options)
    assert r["spectral_path"] == path
    assert r["spatial_path"] == _lib.SPATIAL_TILE + 256
    assert_oracle(p, r)
    assert_close(p, r, run(p))


@pytest.mark.parametrize("lsf_kind", ["muse", "none"])
@pytest.mark.parametrize("D,fs,hw,path", [
    (128, 7, (13, 16), _lib.SPATIAL_CONV_ROWS), (128, 11, (13, 24), _lib.SPATIAL_CONV_ROWS),
    (200, 11, (13, 24), _lib.SPATIAL_CONV_ROWS_ZB), (30, 9, (13, 20), _lib.SPATIAL_CONV_ROWS_ZB)])
def test_one_pass_kernel_codes(D, fs, hw, path, lsf_kind):
    """conv_rows = 1 (the default) on the xy-symmetric FSF: k_conv_rows with the LSF epilogue at
    128 channels, FSF only without an LSF, in z-blocks at every other depth (the LSF then has a
    pass of its own)."""
    p = problem("xy", fs, D, hw[0], hw[1], lsf_kind)
    r = run(p, conv_rows=1)
    assert r["spatial_path"] == (_lib.SPATIAL_CONV_ROWS_LSF if (D == 128 and lsf_kind == "muse") else path)
    assert_oracle(p, r)
    assert_close(p, r, run(p))                           # the march kernels


@pytest.mark.parametrize("what", ["generic", "deep", "deep tap list"])
def test_generic_and_deep_kernels(what):
    """k_spatial_generic (an FSF wider than 15 columns) and, beyond 1024 channels, k_spatial_deep
    with the LSF by k_spectral_blocks or, where that is off, by k_spectral_deep."""
    if what == "generic":
        rng = np.random.default_rng(17)
        f = rng.random((5, 17))
        p = problem(FSF(f / f.sum()), 17, 8, 9, 21)
        want = (_lib.SPATIAL_GENERIC, _lib.SPECTRAL_TAPS)
        options = {}
    else:
        p = problem(FSF(fsf_of("none", 3)), 3, 1030, 5, 6)
        options = {"spectral_blocks": 0} if what == "deep tap list" else {}
        want = (_lib.SPATIAL_DEEP, _lib.SPECTRAL_DEEP if options else _lib.SPECTRAL_BLOCKS)
    r = run(p, **options)
    assert (r["spatial_path"], r["spectral_path"]) == want
    assert_oracle(p, r)
