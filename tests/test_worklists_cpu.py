"""
The work lists of the MH sweep and the launch forms of every part (deconv3d_amd/csrc/d3d_worklists.h,
host-only: what build_colour_lists uploads) without a device: tests/worklists_dump.cpp, a stand-alone
program with its own main, is compiled with the host compiler, -fsanitize=address,undefined and -Werror
and run as a child process on a few hundred cases; it prints every part, list and decision as text.
What they must be is restated here from the rules, not from the header:

  * colour class of a spaxel: ((y + gy0) mod fh, (x + gx0) mod fw); a part's real entries of a colour are
    its unmasked spaxels of that class, each once; every unmasked owned spaxel is real exactly once;
  * the windows (fh x fw around every entry, real or virtual) of one (part, colour) cover every cell of the
    part's domain -- the part grown by the FSF's half widths, clipped to the cube -- exactly once, and
    none misses the domain;
  * order: real before virtual, each ascending in (y, x); both reversed where zig-zag is on, the colour's
    ordinal among the part's active colours is odd and the launch's workgroups (windows x 256-channel
    blocks of the z-blocked kernels) exceed flow_grid;
  * strips: strip-major by d3d_strips::plan's ranges (the program prints the plans; tests/test_strips_cpu.py
    proves them), within a strip real before virtual, within those the unsplit order; soff / sreal match;
  * layers, wide, small, strips and the strips' order against the thresholds flow_grid / 2, / 4 and
    > flow_grid, which the cases cross from both sides (asserted at the end).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deconv3d_amd", "csrc")

STRIPS_AUTO = 2       # the automatic strip count ...
STRIP_ORDER_AUTO = 2  # ... and order (chained)
MAX_LAYERS = 3

FIELDS = ("H W Dp fh fw gy0 gx0 oy0 oy1 ox0 ox1 tiled flow_grid ws_max_dp mh_zb deep mh_defer mh_layers_cfg "
          "mh_layers_forced mh_zigzag mh_wide mh_small mh_props strips_opt strip_order_opt chain_opt flow pair "
          "uniform").split()


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no host C++ compiler (c++, g++, clang++) on PATH")


def make_cases():
    rng = np.random.RandomState(20261021)
    shapes = [(5, 5), (7, 9), (12, 12), (13, 40), (40, 17), (24, 24), (8, 33), (30, 30)]
    fsfs = [(1, 1), (3, 3), (5, 3), (3, 5), (11, 11)]
    cases = []
    for n in range(320):
        pick = lambda seq: seq[rng.randint(len(seq))]  # noqa: E731
        c = {}
        c["H"], c["W"] = shapes[n % len(shapes)]
        c["fh"], c["fw"] = fsfs[(n // len(shapes)) % len(fsfs)]
        H, W, fh, fw = c["H"], c["W"], c["fh"], c["fw"]
        plain = n % 2 == 0  # one context, the whole cube: where strips may run
        c["Dp"] = pick([64, 128, 160, 256, 512] if plain else [64, 128, 128, 128, 160, 256, 512])
        c["ws_max_dp"] = pick([512, 512, 256])
        c["mh_zb"] = int(c["Dp"] == 512 and rng.rand() < 0.6)
        c["deep"] = int(rng.rand() < 0.05)
        c["mh_defer"] = 1 if (plain and rng.rand() < 0.85) else pick([0, 1, 1, 1, 2])
        c["mh_layers_cfg"] = pick([1, 2, 3])
        c["mh_layers_forced"] = int(rng.rand() < 0.3)
        c["mh_zigzag"] = int(rng.rand() < 0.8)
        c["mh_wide"] = int(rng.rand() < 0.8)
        c["mh_small"] = pick([0, 1, 1, 2])
        c["mh_props"] = int(rng.rand() < 0.8)
        c["strips_opt"] = pick([0, 0, 1, 2, 3, 4])
        c["strip_order_opt"] = pick([0, 1, 2])
        c["chain_opt"], c["flow"], c["pair"] = [int(rng.rand() < 0.04) for _ in range(3)]
        c["uniform"] = int(rng.rand() < 0.2)
        c["flow_grid"] = pick([16, 16, 16, 1024] if plain else [16, 16, 1024])
        c["tiled"] = int(not plain and rng.rand() < 0.6)
        if c["tiled"]:
            c["gy0"], c["gx0"] = pick([0, 1, fh + 2]), pick([0, 1, fw + 2])
            c["oy0"], c["ox0"] = rng.randint(0, 3), rng.randint(0, 3)
            c["oy1"], c["ox1"] = H - rng.randint(0, 3), W - rng.randint(0, 3)
        else:
            c["gy0"] = c["gx0"] = c["oy0"] = c["ox0"] = 0
            c["oy1"], c["ox1"] = H, W
        oy0, oy1, ox0, ox1 = c["oy0"], c["oy1"], c["ox0"], c["ox1"]
        my, mx = (oy0 + oy1) // 2, (ox0 + ox1) // 2
        kind = 0 if plain else pick([0, 1, 2, 4, 5])
        c["parts"] = {
            0: [],
            1: [(oy0, oy1, ox0, ox1, 0)],  # one part rectangle: counts as cut up for the lists
            2: [(oy0, my, ox0, ox1, 0), (my, oy1, ox0, ox1, 1)],
            4: [(oy0, my, ox0, mx, 0), (oy0, my, mx, ox1, 1), (my, oy1, ox0, mx, 1), (my, oy1, mx, ox1, 0)],
            5: [(oy0, my, ox0, ox1, 0), (my, my, ox0, ox1, 0), (my, oy1, ox0, ox1, 1)],  # the middle one empty
        }[kind]
        mk = pick(["none", "none", "random", "random", "row", "colour", "all"])
        mask = np.ones((H, W), dtype=np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        if mk == "random":
            mask[rng.rand(H, W) < 0.3] = 0
        elif mk == "row":     # every colour of one colour row without a spaxel
            mask[(yy + c["gy0"]) % fh == rng.randint(fh)] = 0
        elif mk == "colour":  # one colour class without a spaxel
            mask[((yy + c["gy0"]) % fh == rng.randint(fh)) & ((xx + c["gx0"]) % fw == rng.randint(fw))] = 0
        elif mk == "all":
            mask[:] = 0
        c["mask_kind"] = mk
        c["mask"] = mask
        cases.append(c)
    return cases


def case_text(c):
    lines = [" ".join(str(c[k]) for k in FIELDS),
             " ".join([str(len(c["parts"]))] + [str(v) for p in c["parts"] for v in p]),
             " ".join(str(v) for v in c["mask"].ravel())]
    return "\n".join(lines) + "\n"


def parse(out, n_cases):
    lines = [ln.split() for ln in out.strip().split("\n")]
    at = 0
    res = []
    for _ in range(n_cases):
        head = lines[at]
        assert head[0] == "case", head
        r = dict(zip(("rc", "n_phases", "n_parts", "n_list", "small_usable", "partitioned"), map(int, head[1:])))
        assert lines[at + 1][0] == "colour_real"
        r["colour_real"] = [int(v) for v in lines[at + 1][1:]]
        r["plans"] = {}
        for k, S in enumerate((2, 3, 4)):
            ln = lines[at + 2 + k]
            assert ln[0] == "plan"
            r["plans"][S] = [int(v) for v in ln[2:]] if int(ln[1]) else None
        at += 5
        r["parts"] = []
        names = ("y0 y1 x0 x1 dy0 dy1 dx0 dx1 phase layers wide small strips K last_col order_S order_M "
                 "uses_tables").split()
        for _p in range(r["n_parts"]):
            assert lines[at][0] == "part"
            p = dict(zip(names, map(int, lines[at][1:])))
            for k, key in enumerate(("off", "real", "soff", "sreal")):
                assert lines[at + 1 + k][0] == key
                p[key] = [int(v) for v in lines[at + 1 + k][1:]]
            r["parts"].append(p)
            at += 5
        assert lines[at][0] == "list"
        r["list"] = np.array([int(v) for v in lines[at][1:]], dtype=np.int64).reshape(-1, 4)
        assert len(r["list"]) == r["n_list"]
        at += 1
        res.append(r)
    assert at == len(lines)
    return res


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("worklists") / "worklists_dump")
    build = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                            os.path.join(ROOT, "tests", "worklists_dump.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    cases = make_cases()
    run = subprocess.run([exe], input="".join(case_text(c) for c in cases), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stderr
    return cases, parse(run.stdout, len(cases))


def strip_of(first, row):
    for s in range(len(first) - 1):
        if first[s] <= row < first[s + 1]:
            return s
    return -1


def check_case(c, r, seen):
    H, W, Dp, fh, fw = c["H"], c["W"], c["Dp"], c["fh"], c["fw"]
    fhh, fhw, ncol = (fh - 1) // 2, (fw - 1) // 2, fh * fw
    grid = c["flow_grid"]
    mask = c["mask"]
    assert r["rc"] == 0
    rects = c["parts"] or [(c["oy0"], c["oy1"], c["ox0"], c["ox1"], 0)]
    assert r["n_parts"] == len(rects)
    assert r["n_phases"] == max(p[4] for p in rects) + 1
    partitioned = bool(c["tiled"] or c["parts"])
    assert r["partitioned"] == int(partitioned)
    zmul = (Dp + 255) // 256 if c["mh_zb"] else 1
    small_usable = bool(c["mh_small"] and c["mh_props"] and c["mh_defer"] == 1 and not c["mh_zb"] and not c["deep"] and
                        Dp <= 256 and fh <= 31 and fw <= 31 and H * W * Dp * 8 < 2 ** 32)
    assert r["small_usable"] == int(small_usable)
    real_count = np.zeros((H, W), dtype=np.int64)  # times every spaxel is real, over all parts and colours
    colour_real = np.zeros(ncol, dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    gcol = ((yy + c["gy0"]) % fh) * fw + (xx + c["gx0"]) % fw  # the global colour class of every spaxel
    at = 0
    for (y0, y1, x0, x1, phase), p in zip(rects, r["parts"]):
        assert (p["y0"], p["y1"], p["x0"], p["x1"], p["phase"]) == (y0, y1, x0, x1, phase)
        dom = (max(y0 - fhh, 0), min(y1 + fhh, H), max(x0 - fhw, 0), min(x1 + fhw, W))
        assert (p["dy0"], p["dy1"], p["dx0"], p["dx1"]) == dom
        empty = y1 <= y0 or x1 <= x0
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y1, x0:x1] = True
        assert len(p["off"]) == ncol + 1 and len(p["real"]) == ncol and p["off"][0] == at
        most, ordinal, unsplit, active = 0, 0, [], []
        for col in range(ncol):
            lo, hi = p["off"][col], p["off"][col + 1]
            ent = r["list"][lo:hi]
            assert hi >= lo and np.all(ent[:, 3] == 0)
            want_real = sorted(zip(*np.nonzero(inside & (mask != 0) & (gcol == col))))
            got_real = [(int(y), int(x)) for y, x, k, _ in ent if k == 1]
            assert sorted(got_real) == [(int(y), int(x)) for y, x in want_real]  # each once: no duplicates either
            assert p["real"][col] == len(want_real)
            for y, x in got_real:
                real_count[y, x] += 1
            colour_real[col] += len(want_real)
            if empty:
                assert hi == lo
                unsplit.append([])
                continue
            # every entry belongs to the class; the windows tile the domain
            assert np.all((ent[:, 0] + c["gy0"]) % fh == col // fw) and np.all((ent[:, 1] + c["gx0"]) % fw == col % fw)
            cover = np.zeros((dom[1] - dom[0], dom[3] - dom[2]), dtype=np.int64)
            for y, x, _k, _ in ent:
                a0, a1 = max(y - fhh, dom[0]), min(y - fhh + fh, dom[1])
                b0, b1 = max(x - fhw, dom[2]), min(x - fhw + fw, dom[3])
                assert a1 > a0 and b1 > b0, "a window misses the domain"
                cover[a0 - dom[0]:a1 - dom[0], b0 - dom[2]:b1 - dom[2]] += 1
            assert np.all(cover == 1)
            # the order before any split into strips
            n_all = hi - lo
            virt = sorted((int(y), int(x)) for y, x, k, _ in ent if k == 0)
            reals = [(int(y), int(x)) for y, x in want_real]
            if reals:
                rev = bool(c["mh_zigzag"]) and ordinal % 2 == 1 and n_all * zmul > grid
                seen["rev" if rev else "fwd"] += 1
                if ordinal % 2 == 1 and c["mh_zigzag"]:
                    seen["rev_above" if n_all * zmul > grid else "rev_below"] += 1
                if rev:
                    reals, virt = reals[::-1], virt[::-1]
                ordinal += 1
                active.append(col)
            unsplit.append([(y, x, 1) for y, x in reals] + [(y, x, 0) for y, x in virt])
            most = max(most, n_all)
        at = p["off"][ncol]
        # the decisions
        most_wgs = most * zmul
        layers = 1 if (not c["mh_layers_forced"] and most_wgs < grid // 2) else c["mh_layers_cfg"]
        wide = bool(layers == 1 and c["mh_wide"] and partitioned and Dp == 128 and 0 < most <= grid // 4 and
                    c["mh_defer"] == 1)
        small = layers == 1 and most_wgs < grid // 2
        uses_tables = small_usable and small  # (a default build: no chip-filling form of k_mh_small)
        assert (p["layers"], p["wide"], p["small"], p["uses_tables"]) == (layers, int(wide), int(small), int(uses_tables))
        want = c["strips_opt"] if c["strips_opt"] >= 2 else (
            STRIPS_AUTO if (c["strips_opt"] == 0 and most_wgs >= grid // 2 and not c["uniform"]) else 1)
        plan = r["plans"].get(want)
        strips = want if (want >= 2 and not empty and not partitioned and c["mh_defer"] == 1 and
                          (Dp <= c["ws_max_dp"] or c["mh_zb"]) and not uses_tables and not c["chain_opt"] and
                          not c["flow"] and not c["pair"] and plan is not None) else 1
        assert p["strips"] == strips
        assert p["K"] == len(active) and p["last_col"] == (active[-1] if active else -1)
        seen["layers1" if layers == 1 else "layersN"] += 1
        seen["wide" if wide else "narrow"] += 1
        seen["small" if small else "large"] += 1
        seen["below_half" if most_wgs < grid // 2 else "above_half"] += 1
        if partitioned and Dp == 128 and layers == 1 and c["mh_wide"] and c["mh_defer"] == 1 and most > 0:
            seen["below_quarter" if most <= grid // 4 else "above_quarter"] += 1
        if strips == 1:
            assert p["soff"] == [] and p["sreal"] == [] and (p["order_S"], p["order_M"]) == (0, 0)
            for col in range(ncol):
                got = [tuple(int(v) for v in e[:3]) for e in r["list"][p["off"][col]:p["off"][col + 1]]]
                assert got == unsplit[col]
            seen["whole"] += 1
            continue
        seen["strips%d" % strips] += 1
        assert len(plan) == strips + 1
        soff, sreal = [], []
        for col in range(ncol):
            ly = (col // fw - c["gy0"]) % fh
            rows = {}
            for e in unsplit[col]:
                assert (e[0] - ly) % fh == 0
                s = strip_of(plan, (e[0] - ly) // fh)
                assert s >= 0, "a lattice row outside the plan"
                rows.setdefault(s, []).append(e)
            want_list, so = [], [0]
            for s in range(strips):  # within a strip the unsplit order: its real entries come first already
                es = [e for e in rows.get(s, []) if e[2] == 1] + [e for e in rows.get(s, []) if e[2] == 0]
                want_list += es
                so.append(len(want_list))
                sreal.append(sum(e[2] for e in es))
            soff += so
            got = [tuple(int(v) for v in e[:3]) for e in r["list"][p["off"][col]:p["off"][col + 1]]]
            assert got == want_list
        assert p["soff"] == soff and p["sreal"] == sreal
        # chained where asked (automatic: chained) and every active colour row holds `layers` colours at least
        chained = (c["strip_order_opt"] or STRIP_ORDER_AUTO) == 2 and 1 <= layers <= MAX_LAYERS and bool(active) and all(
            sum(1 for a in active if a // fw == row) >= layers for row in set(a // fw for a in active))
        assert (p["order_S"], p["order_M"]) == ((strips, layers) if chained else (0, 0))
        seen["chained" if chained else "joined"] += 1
        if (c["strip_order_opt"] or STRIP_ORDER_AUTO) == 2 and not chained:
            seen["chain_refused"] += 1
    assert at == r["n_list"]
    owned = np.zeros((H, W), dtype=bool)
    for y0, y1, x0, x1, _ in rects:
        owned[y0:y1, x0:x1] = True
    assert np.array_equal(real_count, (owned & (mask != 0)).astype(np.int64))
    assert r["colour_real"] == [int(v) for v in colour_real]


def test_lists_and_decisions(dumped):
    cases, results = dumped
    from collections import Counter
    seen = Counter()
    for k, (c, r) in enumerate(zip(cases, results)):
        try:
            check_case(c, r, seen)
        except AssertionError as e:
            raise AssertionError("case %d %s parts=%s mask=%s: %s" % (
                k, {f: c[f] for f in FIELDS}, c["parts"], c["mask_kind"], e))
    # the generator covers what it must, and every decision falls on both sides of its threshold
    for key in ("rev", "fwd", "rev_above", "rev_below", "layers1", "layersN", "wide", "narrow", "small", "large",
                "below_half", "above_half", "below_quarter", "above_quarter", "whole", "strips2", "strips3", "strips4",
                "chained", "joined", "chain_refused"):
        assert seen[key] > 0, (key, dict(seen))
    for key, values in (("Dp", (64, 128, 160, 256, 512)), ("flow_grid", (16, 1024)), ("strips_opt", (0, 1, 2, 3, 4)),
                        ("strip_order_opt", (0, 1, 2)), ("mask_kind", ("none", "random", "row", "colour", "all")),
                        ("gy0", (0, 1)), ("gx0", (0, 1))):
        assert set(values) <= set(c[key] for c in cases), key
    assert any(c["fh"] > c["H"] for c in cases) and any(c["gy0"] == c["fh"] + 2 for c in cases)
    assert set(len(c["parts"]) for c in cases) >= {0, 1, 2, 3, 4}
    assert any(c["mh_zb"] and c["Dp"] == 512 for c in cases)
