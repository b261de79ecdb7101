"""Cost of the posterior histograms kept on the device (d3d_hist_*, k_hist_accum) on one GPU:

    python tools/hist_time.py [parent=<libdeconv3d_hip.so of the parent commit>] [shape=D,H,W]

At 300x300x128 (the bench's config 3: Moffat 11x11, 17-tap LSF), us per d3d_post_accumulate -- one
accumulated sample: the forward model into SLOT_SIM, k_post_accum and, with histograms on, k_hist_accum
on the same stream --
  * with the parent commit's library (given parent=; built by tools/build_variant.sh from a checkout of
    that commit), timed twice: the spread between the two is what "equal" can mean on this box;
  * with this library, histograms off, twice;
  * with this library, histograms on and the pilot passed;
and the same three with the map's moments alone (d3d_post_begin(0): no forward model, k_post_accum
touches the map only), where the histograms' launch is not hidden behind 72 bytes per voxel.  The
difference on - off is what the added launch costs per sample.  Then one d3d_hist_quantiles call
(k_hist_quantiles and its three downloads, wall clock) and the device memory the counters take.

HIP events on the context's stream after a warm-up; every figure is the median of 7 batches of 20
(tools/posterior_time.py's method).  Each row is a process of its own (DECONV3D_HIP_LIB selects the
library).  profiles/hist_time.txt."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
D, H, W = (int(v) for v in args.get("shape", "128,300,300").split(","))


def engine():
    import bench as B
    from deconv3d_amd import _lib
    fsf, lsf = B.build_taps(D, 11)
    eng = _lib.Engine((D, H, W), fsf.shape)
    eng.set_taps(fsf, lsf)
    data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
    eng.set_data(data, var)
    eng.set_params(init)
    eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
    return eng, truth, init


def median_ms(eng, call, per_batch=20, batches=7, warm=3):
    for _ in range(warm):
        call()
    eng.sync()
    out = []
    for _ in range(batches):
        eng.timer_start()
        for _ in range(per_batch):
            call()
        out.append(eng.timer_stop() / per_batch)
    return float(np.median(out))


def row(what, hist):
    """us per accumulated sample; what: d3d_post_begin's argument; hist < 0: the parent's library."""
    from deconv3d_amd import _lib
    if hist < 0:      # the parent commit's library has no d3d_hist_*
        _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if s not in _lib.HIST_PROTOTYPES]
        _lib.HIST_PROTOTYPES.clear()
    eng, truth, init = engine()
    with eng:
        eng.post_begin(what)
        if hist > 0:
            eng.hist_begin(2, 6.0)
            for p in (init, truth):          # a pilot with a spread, so that the samples fall inside the ranges
                eng.set_params(p)
                eng.post_accumulate()
            eng.set_params(0.5 * (init + truth))
        us = median_ms(eng, eng.post_accumulate) * 1e3
        print("%.2f" % us, flush=True)
        if hist > 0 and what == 0:
            assert eng.hist_count() > 0
            bins, tails, _ = eng.hist_get()
            inside = float(bins.sum()) / max(float(bins.sum()) + float(tails.sum()), 1.)
            eng.hist_quantiles([0.16, 0.5, 0.84])
            t0 = time.perf_counter()
            eng.hist_quantiles([0.16, 0.5, 0.84])
            ms = (time.perf_counter() - t0) * 1e3
            print("  (%.0f %% of the counted samples inside the ranges; d3d_hist_quantiles of 3 quantiles, mode and "
                  "outside with their downloads: %.2f ms; counters %.1f MB)"
                  % (100. * inside, ms, H * W * 1120 / 1e6), file=sys.stderr, flush=True)


def child(what, hist, lib=None):
    env = dict(os.environ)
    if lib:
        env["DECONV3D_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "mode=row", "what=%d" % what, "hist=%d" % hist,
                          "shape=%d,%d,%d" % (D, H, W)], env=env, check=True, stdout=subprocess.PIPE, text=True,
                         timeout=600)
    return float(out.stdout.strip().splitlines()[-1])


if args.get("mode") == "row":
    row(int(args["what"]), int(args["hist"]))
else:
    for what, label in ((3, "both cubes' moments"), (0, "the map's moments alone")):
        rows = []
        if args.get("parent"):
            rows += [("parent commit's library", -1, args["parent"]), ("parent commit's library, again", -1, args["parent"])]
        rows += [("histograms off", 0, None), ("histograms off, again", 0, None), ("histograms on", 1, None)]
        for name, hist, lib in rows:
            print("%dx%dx%d %-24s %-32s %9.2f us per accumulated sample"
                  % (W, H, D, label, name, child(what, hist, lib)), flush=True)
