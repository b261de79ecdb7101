"""Lattice-row strips of a colour row (option mh_strips): same-box A/B and the
overlap of the strips' kernels, for profiles/sweep_strips_ab.txt.

  python tools/mh_strips.py ab [--lib NAME=PATH ...] [--strips 1,2,3,4] [--order 1,2] [--rounds 4] [-- bench args]
      bench.py in child processes, alternating between the libraries (DECONV3D_HIP_LIB; the tree's
      library is "tree"), the strip counts (D3D_MH_STRIPS, the default of new contexts) and, with
      --order, how the strips of consecutive colour rows are ordered (D3D_MH_STRIP_ORDER: 1 joined,
      2 chained; a column NAME/STRIPS/oORDER each) inside one job, `rounds` times over; prints every ms_per_step, medians, spreads and the project's
      rule against the first column (every run faster, median gain >= 5 x the larger spread).
      With --dump DIR every column also runs `--steps 5 --warmup 1 --dump-outputs` once and the
      outputs are compared with the first column's as 64-bit patterns.
      --key PATH: another figure of bench.py's record than ms_per_step, e.g.
      extras.uniform_variance.avg_launch_us (with `-- --full --no-cpu`).

  python tools/mh_strips.py overlap TRACE.csv [--colours 121] [--colour-rows 11]
      a rocprofv3 --kernel-trace CSV of the plain bench command: per sweep kernel launch the
      duration, and over the timed part how much of the wall time has 0, 1, 2, ... k_mh_ws kernels
      in flight; the gap at a join (last end of a colour row to the next start) against the gap
      between two launches of one stream; the time with nothing in flight per colour row and per
      sweep (a sweep: --colours launches of the busiest stream, in --colour-rows rows).
"""
import argparse
import csv
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def bench(lib, strips, args, timeout=900, order=None):
    env = dict(os.environ)
    env.pop("DECONV3D_HIP_LIB", None)
    env.pop("D3D_MH_STRIPS", None)
    env.pop("D3D_MH_STRIP_ORDER", None)
    if lib:
        env["DECONV3D_HIP_LIB"] = lib
    if strips is not None:
        env["D3D_MH_STRIPS"] = str(strips)
    if order is not None:
        env["D3D_MH_STRIP_ORDER"] = str(order)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, timeout=timeout,
                         stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def dig(rec, path):
    for k in path.split("."):
        rec = rec[k]
    return float(rec)


def ab(a, bench_args):
    libs = [("tree", None)] + [tuple(s.split("=", 1)) for s in a.lib]
    cols = []
    for name, path in libs:
        if name != "tree" and name in a.plain:
            cols.append((name, path, None, None))  # a library from before the option: no strip counts
        else:
            for s in a.strips:
                if a.order and s > 1:
                    cols += [("%s/%d/o%d" % (name, s, o), path, s, o) for o in a.order]
                else:
                    cols.append(("%s/%d" % (name, s), path, s, None))
    cols.sort(key=lambda c: c[0] not in a.first)  # the reference column first
    if a.dump:
        ref = None
        for name, path, s, o in cols:
            d = os.path.join(a.dump, name.replace("/", "_"))
            bench(path, s, ["--gpus", "1", "--steps", "5", "--warmup", "1", "--dump-outputs", d], order=o)
            got = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}
            if ref is None:
                ref = got
                print("outputs of %s: %s" % (name, ", ".join(sorted(got))), flush=True)
                continue
            same = sorted(got) == sorted(ref) and all(
                got[f].shape == ref[f].shape and np.array_equal(got[f].view(np.uint64), ref[f].view(np.uint64))
                for f in ref)
            print("outputs of %-12s %s" % (name, "bit-identical" if same else "DIFFER"), flush=True)
    runs = {c[0]: [] for c in cols}
    args = bench_args or ["--gpus", "1", "--steps", "20", "--warmup", "3"]
    for r in range(a.rounds):
        for name, path, s, o in cols:
            runs[name].append(dig(bench(path, s, args, order=o), a.key))
        print("round %d  " % (r + 1) + "  ".join("%s %.4f" % (n, runs[n][-1]) for n, _, _, _ in cols), flush=True)
    print("\n%s of `bench.py %s`" % (a.key, " ".join(args)))
    print("  run     " + "".join("%-12s" % n for n, _, _, _ in cols))
    for r in range(a.rounds):
        print("  %-8d" % (r + 1) + "".join("%-12.4f" % runs[n][r] for n, _, _, _ in cols))
    med = {n: float(np.median(v)) for n, v in runs.items()}
    spread = {n: (max(v) - min(v)) / med[n] for n, v in runs.items()}
    print("  median  " + "".join("%-12.4f" % med[n] for n, _, _, _ in cols))
    print("  spread  " + "".join("%-12s" % ("%.2f %%" % (100 * spread[n])) for n, _, _, _ in cols))
    base = cols[0][0]
    for n, _, _, _ in cols[1:]:
        gain = 1.0 - med[n] / med[base]
        every = max(runs[n]) < min(runs[base])
        noise = max(spread[n], spread[base])
        print("  %-12s against %s: %+.2f %%, %s, %.1f x the larger spread -> %s"
              % (n, base, -100 * gain, "every run faster" if every else "NOT every run faster",
                 gain / noise if noise > 0 else float("inf"),
                 "passes" if every and gain >= 5 * noise else "does not pass"))


def overlap(path, colours=121, colour_rows=11):
    rows = []
    with open(path) as fh:
        for rec in csv.DictReader(fh):
            rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec["Kernel_Name"],
                         rec.get("Stream_Id", rec.get("Queue_Id", "0"))))
    rows.sort()
    ws = [r for r in rows if "k_mh_ws" in r[2]]
    if not ws:
        raise SystemExit("no k_mh_ws launches in %s" % path)
    # the timed part: the last run of sweep kernels that no other kernel interrupts for long --
    # simply the second half of the launches (warm-up and set-up come first)
    ws = ws[len(ws) // 2:]
    t0, t1 = ws[0][0], max(r[1] for r in ws)
    ev = sorted([(r[0], 1) for r in ws] + [(r[1], -1) for r in ws])
    depth, last, hist = 0, t0, {}
    for t, d in ev:
        hist[depth] = hist.get(depth, 0) + (t - last)
        last = t
        depth += d
    wall = float(t1 - t0)
    dur = np.array([r[1] - r[0] for r in ws]) / 1e3
    print("%s: %d k_mh_ws launches over %.3f ms, %.2f us of wall time per launch, kernel duration "
          "median %.2f us (min %.2f, max %.2f)" % (os.path.basename(path), len(ws), wall / 1e6,
                                                   wall / 1e3 / len(ws), np.median(dur), dur.min(), dur.max()))
    for k in sorted(hist):
        print("  %d kernels in flight: %5.1f %% of the wall time" % (k, 100.0 * hist[k] / wall))
    # a sweep is `colours` launches of the busiest stream (strip 0 launches every colour)
    per_stream = {}
    for r in ws:
        per_stream[r[3]] = per_stream.get(r[3], 0) + 1
    sweeps = max(per_stream.values()) / float(colours)
    idle = hist.get(0, 0) / 1e3
    print("  %.1f sweeps: %.1f us with nothing in flight per colour row, %.1f us per sweep; %.1f us of wall time per sweep"
          % (sweeps, idle / (sweeps * colour_rows), idle / sweeps, wall / 1e3 / sweeps))
    # gaps with nothing in flight, by length: the longest ones are the joins
    gaps, depth, last = [], 0, t0
    for t, d in ev:
        if depth == 0 and t > last:
            gaps.append((t - last) / 1e3)
        last = t
        depth += d
    if gaps:
        g = np.sort(np.array(gaps))
        print("  %d gaps with nothing in flight: median %.2f us, 90th percentile %.2f us, total %.1f %% of the wall"
              % (len(g), np.median(g), g[int(0.9 * (len(g) - 1))], 100.0 * g.sum() * 1e3 / wall))
    # the stretches between two such gaps are the colour rows: per row how long after the fork (the end of
    # the last whole launch on the first stream) an auxiliary stream's first kernel starts, and how far
    # apart the streams' last kernels end
    rows_, cur, depth = [], [], 0
    for r in ws:
        if cur and r[0] > max(q[1] for q in cur):
            rows_.append(cur)
            cur = []
        cur.append(r)
    rows_.append(cur)
    lag, apart, span, n_whole = [], [], [], []
    for seg in rows_:
        streams = sorted({q[3] for q in seg})
        if len(streams) < 2:
            continue
        main = seg[0][3]
        first_aux = min(q[0] for q in seg if q[3] != main)
        whole = [q for q in seg if q[3] == main and q[1] <= first_aux]
        if whole:
            lag.append((first_aux - max(q[1] for q in whole)) / 1e3)
        n_whole.append(len(whole))
        ends = [max(q[1] for q in seg if q[3] == s) for s in streams]
        apart.append((max(ends) - min(ends)) / 1e3)
        span.append((max(ends) - seg[0][0]) / 1e3)
    if span:
        print("  %d colour rows in strips: %.1f us each (median), %.1f whole launches before the fork; first kernel of "
              "an auxiliary stream %.2f us after the fork (median); the streams' last kernels end %.2f us apart "
              "(median, 90th percentile %.2f)"
              % (len(span), np.median(span), np.mean(n_whole), np.median(lag) if lag else float("nan"),
                 np.median(apart), np.sort(apart)[int(0.9 * (len(apart) - 1))]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("ab")
    p.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    p.add_argument("--plain", action="append", default=[], metavar="NAME",
                   help="a library without the option (the parent's): one column, no strip counts")
    p.add_argument("--first", action="append", default=[], metavar="COLUMN", help="the reference column")
    p.add_argument("--strips", type=lambda s: [int(v) for v in s.split(",")], default=[1, 2, 3, 4])
    p.add_argument("--order", type=lambda s: [int(v) for v in s.split(",")], default=[],
                   help="orders of the strips of consecutive colour rows (1 joined, 2 chained): a column each")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--key", default="ms_per_step")
    p.add_argument("--dump", default=None, metavar="DIR")
    p.add_argument("bench_args", nargs=argparse.REMAINDER)
    q = sub.add_parser("overlap")
    q.add_argument("trace")
    q.add_argument("--colours", type=int, default=121, help="active colours of a sweep (11 x 11 taps: 121)")
    q.add_argument("--colour-rows", type=int, default=11, help="colour rows of a sweep")
    a = ap.parse_args()
    if a.cmd == "overlap":
        return overlap(a.trace, a.colours, a.colour_rows)
    rest = a.bench_args[1:] if a.bench_args[:1] == ["--"] else a.bench_args
    if not a.first:
        a.first = [a.plain[0]] if a.plain else ["tree/1"]
    ab(a, rest)


if __name__ == "__main__":
    main()
