"""
The forms of the taps (deconv3d_amd/csrc/d3d_taps.h, host-only: what d3d_set_taps uploads and which
kernels it admits) without a device: tests/taps_dump.cpp, a stand-alone program with its own main, is
compiled with the host compiler, -fsanitize=address,undefined and -Werror and run as a child process;
doubles cross in C's hexadecimal form, exactly.  What the result must be is restated here from the rules:

  * FSF: mirror symmetries bit for bit; an outer product u v^T (u = centre column / centre tap, v = centre
    row) where every tap is within 8 ulp of the largest magnitude; the quadrant tables by distance from
    the centre of a square FSF with both symmetries; the rows per strip of the march kernels -- the HY in
    12 .. 20 with the fewest rounds x steps, the largest among equals;
  * LSF: the closed form of the reference's padded FFT convolution, out[k] = sum_t lsf[t] ext[(k + s_t) mod N],
    s_t = N/2 - h - t, checked against the oracle's FFT pipeline on delta spectra; the cut -- thr >= 0: taps
    up to thr * max dropped; thr < 0: the smallest taps dropped while the magnitude dropped stays within
    |thr| * sum, equal taps all or none; the dense form where every tap lies within +-LSF_RL channels and
    N >= 4 LSF_RL, admitted at any depth (dense_any) or only with N == D (dense_ok).
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import deconv3d_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deconv3d_amd", "csrc")
EPS = 2.0 ** -52
RL = 8  # the reach of the dense LSF form (taps within +-8 channels)


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no host C++ compiler (c++, g++, clang++) on PATH")


def mirrored(f, x=False, y=False):
    """f with the asked mirror symmetries made exact, bit for bit."""
    f = f.copy()
    if x:
        f[:, f.shape[1] - f.shape[1] // 2:] = f[:, :f.shape[1] // 2][:, ::-1]
    if y:
        f[f.shape[0] - f.shape[0] // 2:, :] = f[:f.shape[0] // 2, :][::-1, :]
    return f


def gauss2d(fh, fw, sy, sx, oy=0.0, ox=0.0):
    y, x = np.mgrid[0:fh, 0:fw].astype(np.float64)
    return np.exp(-0.5 * (((y - (fh - 1) / 2 - oy) / sy) ** 2 + ((x - (fw - 1) / 2 - ox) / sx) ** 2))


def fsf_cases():
    u5 = np.array([0.25, 0.5, 1.0, 0.5, 0.25])
    v5 = np.array([0.125, 0.5, 1.0, 0.5, 0.125])
    outer = np.outer(u5, v5)  # every product exact
    p4, p16 = outer.copy(), outer.copy()
    p4[0, 1] += 4 * EPS       # the largest tap is 1: 4 and 16 ulp of it, off the centre row and column
    p16[0, 1] += 16 * EPS
    zero_centre = mirrored(gauss2d(5, 5, 1.0, 1.0), True, True)
    zero_centre[2, 2] = 0.0
    fs = {
        "sym11": mirrored(gauss2d(11, 11, 1.7, 1.7), True, True),
        "sym3": mirrored(gauss2d(3, 3, 0.8, 0.8), True, True),
        "sym5x3": mirrored(gauss2d(5, 3, 1.1, 0.7), True, True),
        "one": np.array([[0.75]]),
        "xonly": mirrored(gauss2d(11, 11, 1.7, 1.7, oy=0.3), x=True),
        "yonly": mirrored(gauss2d(11, 11, 1.7, 1.7, ox=0.3), y=True),
        "rotated": O.gaussian_fsf_image(4.0, pa=30.0, ba=0.5),
        "moffat": mirrored(O.moffat_fsf_image((11, 11), 2.5, fwhm_px=3.0), True, True),
        "outer": outer, "outer4": p4, "outer16": p16, "zero_centre": zero_centre,
    }
    cases = []
    for name, f in fs.items():
        cases.append(dict(name=name, fsf=f, spatial_sep=1))
    cases.append(dict(name="outer_nosep", fsf=outer, spatial_sep=0))
    for (H, W) in ((300, 300), (64, 64), (12, 500)):
        for opt in (0, 17):
            for HL, grid, f in ((128, 1024, "sym11"), (64, 1024, "sym3"), (32, 1024, "sym11"), (16, 0, "sym5x3"),
                                (64, 16, "sym11")):
                cases.append(dict(name="march", fsf=fs[f], H=H, W=W, HL=HL, flow_grid=grid, march_hy_opt=opt))
    return cases


def lsf_cases():
    rng = np.random.RandomState(7)
    cases = []
    for D in (7, 8, 64, 100):
        skew = rng.rand(D) + 0.1
        for name, lsf in (("gauss", O.gaussian_lsf_vector(D, 0.9)), ("skew", skew / skew.sum())):
            cases.append(dict(name="%s%d" % (name, D), D=D, lsf=lsf, thr=0.0, delta=True))
    g128 = O.gaussian_lsf_vector(128, 1.02)
    cases.append(dict(name="thr0", D=128, lsf=g128, thr=0.0))
    cases.append(dict(name="thr1e-20", D=128, lsf=g128, thr=1e-20))
    for sigma in (0.5, 0.82, 1.02, 1.2):
        cases.append(dict(name="bound%g" % sigma, D=128, lsf=O.gaussian_lsf_vector(128, sigma), thr=-1e-16, sigma=sigma))
    # combs of equal taps under the bound 1e-3 * sum: the equal ones go together or not at all
    for name, small in (("comb4", [4e-4] * 4), ("comb2", [4e-4] * 2), ("comb4_1", [4e-4] * 4 + [1e-5]),
                        ("comb_neg", [4e-4, -4e-4, 4e-4, 1e-5, -1e-5])):
        lsf = np.zeros(64)
        lsf[32] = 1.0
        lsf[20:20 + len(small)] = small
        cases.append(dict(name=name, D=64, lsf=lsf, thr=-1e-3))
    cases.append(dict(name="zero", D=64, lsf=np.zeros(64), thr=0.0))
    cases.append(dict(name="zero_bound", D=64, lsf=np.zeros(64), thr=-1e-16))
    # the dense form: N == D, N != D, N < 4 RL; mirror-symmetric or not; the spectrum within a wavefront or not
    near = np.zeros(64)
    near[31:34] = (0.2, 0.5, 0.3)
    for D, lsf in ((64, O.gaussian_lsf_vector(64, 0.9)), (64, near), (100, O.gaussian_lsf_vector(100, 0.9)),
                   (8, O.gaussian_lsf_vector(8, 0.9)), (128, O.gaussian_lsf_vector(128, 3.0))):
        for HL in (64, 128, 48, 16):
            cases.append(dict(name="dense%d" % D, D=D, lsf=lsf, thr=-1e-16, HL=HL))
    return cases


def case_text(c):
    f = np.asarray(c["fsf"], dtype=np.float64)
    lsf = c.get("lsf")
    words = [f.shape[0], f.shape[1], c["D"], c["N"], c["H"], c["W"], c["HL"], c["flow_grid"], RL, float(c["thr"]).hex(),
             c["spatial_sep"], c["march_hy_opt"], 0 if lsf is None else 1]
    words += [float(v).hex() for v in f.ravel()]
    if lsf is not None:
        words += [float(v).hex() for v in lsf]
    return " ".join(str(w) for w in words) + "\n"


@pytest.fixture(scope="module")
def analysed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("taps") / "taps_dump")
    build = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                            os.path.join(ROOT, "tests", "taps_dump.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    cases = fsf_cases() + lsf_cases()
    for c in cases:
        c.setdefault("fsf", mirrored(gauss2d(3, 3, 0.8, 0.8), True, True))
        c.setdefault("D", 64)
        c["N"] = O.padded_length(c["D"])  # the reference's power of two
        for k, v in (("H", 64), ("W", 64), ("HL", 64), ("flow_grid", 1024), ("thr", 0.0), ("spatial_sep", 1),
                     ("march_hy_opt", 0)):
            c.setdefault(k, v)
    run = subprocess.run([exe], input="".join(case_text(c) for c in cases), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = [ln.split() for ln in run.stdout.strip().split("\n")]
    assert len(lines) == 7 * len(cases)
    for k, c in enumerate(cases):
        head, rows = lines[7 * k], lines[7 * k + 1:7 * k + 7]
        assert head[0] == "case" and [r[0] for r in rows] == ["uv", "quad", "quad_sep", "shift", "weight", "dense"]
        r = dict(zip("symx symy sep symt march_hy lsf_empty dense_any dense_ok dense_sym fusable".split(), map(int, head[1:])))
        for row in rows:
            r[row[0]] = [int(v) for v in row[1:]] if row[0] == "shift" else [float.fromhex(v) for v in row[1:]]
        c["got"] = r
    return {"fsf": [c for c in cases if "lsf" not in c], "lsf": [c for c in cases if "lsf" in c]}


def same_bits(got, want):
    want = np.asarray(want, dtype=np.float64).ravel()
    return len(got) == len(want) and np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), want.view(np.uint64))


def restate_fsf(c):
    f = np.asarray(c["fsf"], dtype=np.float64)
    fh, fw = f.shape
    cy, cx = (fh - 1) // 2, (fw - 1) // 2
    w = {}
    w["symx"] = bool(np.array_equal(f, f[:, ::-1]))
    w["symy"] = bool(np.array_equal(f, f[::-1, :]))
    cc, amax = f[cy, cx], np.max(np.abs(f))
    u, v = (f[:, cx] / cc, f[cy, :]) if cc != 0.0 else (None, None)
    w["sep"] = bool(cc != 0.0 and amax > 0.0 and np.all(np.abs(f - np.outer(u, v)) <= 8.0 * EPS * amax) and
                    c["spatial_sep"] != 0)
    w["uv"] = np.concatenate([u, v]) if w["sep"] else []
    w["quad"], w["quad_sep"], w["symt"] = [], [], False
    if w["symx"] and w["symy"] and fh == fw:
        q = f[:cy + 1, :cx + 1][::-1, ::-1]  # by distance from the centre
        w["quad"], w["symt"] = q, bool(np.array_equal(q, q.T))
        if w["sep"] and cy >= 1:  # (a 1 x 1 table has no second row)
            qs = np.zeros_like(q)
            qs[0], qs[1] = v[:cx + 1][::-1], u[:cy + 1][::-1]
            w["quad_sep"] = qs
    TX = 3 if fw >= 9 else 4
    slots = 2 * (c["flow_grid"] if c["flow_grid"] > 0 else 1024)
    per_wave = 1 if c["HL"] >= 64 else 64 // c["HL"]
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    cost = {hy: ceil(ceil(ceil(c["W"], TX) * ceil(c["H"], hy), per_wave), slots) * (hy + fh - 1) for hy in range(12, 21)}
    w["march_hy"] = c["march_hy_opt"] if c["march_hy_opt"] >= 1 else max(hy for hy in cost if cost[hy] == min(cost.values()))
    return w


def test_fsf_forms(analysed):
    by_name = {}
    for c in analysed["fsf"]:
        g, w = c["got"], restate_fsf(c)
        by_name[c["name"]] = g
        for k in ("symx", "symy", "sep", "symt", "march_hy"):
            assert g[k] == w[k], (c["name"], k, g[k], w[k])
        for k in ("uv", "quad", "quad_sep"):
            assert same_bits(g[k], w[k]), (c["name"], k)
        assert g["shift"] == [] and g["weight"] == [] and not g["lsf_empty"] and not g["dense_any"]
    flags = lambda n: tuple(by_name[n][k] for k in ("symx", "symy", "sep", "symt"))  # noqa: E731
    # what the cases are there for (x, y, outer product, transpose)
    assert flags("sym11") == (1, 1, 1, 1) and flags("sym3") == (1, 1, 1, 1) and flags("one") == (1, 1, 1, 1)
    assert flags("sym5x3")[:2] == (1, 1) and by_name["sym5x3"]["quad"] == []
    assert flags("moffat") == (1, 1, 0, 1)  # radial, no outer product
    assert flags("xonly")[:2] == (1, 0) and flags("yonly")[:2] == (0, 1)
    assert flags("rotated") == (0, 0, 0, 0)
    assert flags("outer") == (1, 1, 1, 0) and len(by_name["outer"]["quad_sep"]) == 9
    assert by_name["outer4"]["sep"] == 1 and by_name["outer16"]["sep"] == 0  # the bound is 8 ulp of the largest tap
    assert by_name["zero_centre"]["sep"] == 0 and by_name["outer_nosep"]["sep"] == 0
    marches = [c["got"]["march_hy"] for c in analysed["fsf"] if c["name"] == "march" and c["march_hy_opt"] == 0]
    assert len(set(marches)) > 2  # the cost rule is exercised: not one answer everywhere
    # 300 rows, 11 x 11, a spectrum of two wavefronts: 15 rows per strip (20 strips of 25 steps, all resident)
    assert [c["got"]["march_hy"] for c in analysed["fsf"]
            if c["name"] == "march" and (c["H"], c["HL"], c["march_hy_opt"]) == (300, 128, 0)] == [15]


def restate_cut(lsf, thr):
    mag = np.abs(lsf)
    if thr >= 0.0:
        return thr * mag.max()
    bound = -thr * math.fsum(mag)
    ok = [m for m in np.unique(mag) if math.fsum(mag[mag <= m]) <= bound]  # equal taps: all or none
    return max(ok) if ok else 0.0


def restate_lsf(c):
    lsf, D, N = np.asarray(c["lsf"], dtype=np.float64), c["D"], c["N"]
    h = O.padding_offset(D)
    keep = np.nonzero(np.abs(lsf) > restate_cut(lsf, c["thr"]))[0]
    w = {"shift": [int((N // 2 - h - t) % N) for t in keep], "weight": lsf[keep]}
    w["lsf_empty"] = len(keep) == 0
    signed = [s - N if s > N // 2 else s for s in w["shift"]]
    fits = len(keep) > 0 and N >= 4 * RL and all(-RL <= s <= RL for s in signed)
    dense = np.zeros(2 * RL + 1)
    if fits:
        for s, wt in zip(signed, w["weight"]):
            dense[s + RL] += wt
    w["dense"] = dense
    w["dense_any"] = fits
    w["dense_ok"] = fits and N == D
    w["dense_sym"] = fits and bool(np.array_equal(dense, dense[::-1]))
    w["fusable"] = w["dense_ok"] and c["HL"] <= 64 and 64 % c["HL"] == 0
    return w


def test_lsf_forms(analysed):
    by_name = {}
    for c in analysed["lsf"]:
        g, w = c["got"], restate_lsf(c)
        by_name.setdefault(c["name"], g)
        assert g["shift"] == w["shift"], c["name"]
        assert same_bits(g["weight"], w["weight"]) and same_bits(g["dense"], w["dense"]), c["name"]
        for k in ("lsf_empty", "dense_any", "dense_ok", "dense_sym", "fusable"):
            assert g[k] == int(w[k]), (c["name"], c["HL"], k)
        if c.get("delta"):
            # the tap list is the reference's convolution: every delta spectrum through the oracle's FFT pipeline.
            # Three transforms of length N in fp64: a few eps log2(N) of the largest output, sum|lsf| at most
            D, N = c["D"], c["N"]
            tol = 16 * EPS * math.log2(N) * np.abs(c["lsf"]).sum()
            k = np.arange(D)
            for j in range(D):
                line = np.zeros(D)
                line[j] = 1.0
                ext = np.zeros(N)
                ext[:D] = line
                out = np.zeros(D)
                for s, wt in zip(g["shift"], g["weight"]):
                    out += wt * ext[(k + s) % N]
                assert np.max(np.abs(out - O.convolve_1d_fft(line, c["lsf"]))) <= tol, (c["name"], j)
    n_taps = lambda n: len(by_name[n]["shift"])  # noqa: E731
    # thr = 0 keeps every non-zero tap; 1e-20 of the largest keeps a Gaussian's tail out to 9.6 sigma: 1.02 channels fall off +-8
    g128 = O.gaussian_lsf_vector(128, 1.02)
    assert n_taps("thr0") == int(np.count_nonzero(g128)) and n_taps("thr1e-20") == int(np.sum(g128 > 1e-20 * g128.max()))
    assert n_taps("thr1e-20") < n_taps("thr0") and not by_name["thr1e-20"]["dense_any"]
    # the error bound 1e-16: the taps beyond +-8 channels of a Gaussian of sigma 1.02 sum to 2 exp(-81 / (2 sigma^2)) /
    # (sigma sqrt(2 pi)) = 1e-17 and go; of sigma 1.2 to 5e-13 and stay.  MUSE's 0.82 .. 1.02 channels fit.
    assert [by_name["bound%g" % s]["dense_any"] for s in (0.5, 0.82, 1.02, 1.2)] == [1, 1, 1, 0]
    # four equal taps of which only two fit the bound all stay; two that fit go; a smaller one goes alone
    assert n_taps("comb4") == 5 and n_taps("comb2") == 1 and n_taps("comb4_1") == 5 and n_taps("comb_neg") == 4
    assert by_name["zero"]["lsf_empty"] == 1 and by_name["zero_bound"]["lsf_empty"] == 1
    seen = set((c["got"]["dense_any"], c["got"]["dense_ok"], c["got"]["dense_sym"], c["got"]["fusable"])
               for c in analysed["lsf"] if c["name"].startswith("dense"))
    assert seen == {(0, 0, 0, 0), (1, 0, 1, 0), (1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 0, 0), (1, 1, 0, 1)}, seen
