# coding=utf-8
"""
Cost of the smoothness prior (d3d_prior_begin) at the flagship shape, 300x300x128:
ms per sweep with and without the prior -- HIP events around 20 sweeps, median of 5 runs after a
warm-up --, and the time of one d3d_prior_energy call (two kernels and a 32-byte copy).

    python tools/prior_time.py [--shape 128 300 300] [--sweeps 20] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench as B                      # noqa: E402
from deconv3d_amd import _lib          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 300, 300], metavar=("D", "H", "W"))
    ap.add_argument("--fsf", type=int, default=11)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    D, H, W = args.shape
    fsf, lsf = B.build_taps(D, args.fsf)
    out = dict(shape=[D, H, W], sweeps=args.sweeps, runs=args.runs)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
        eng.set_data(data, var)
        eng.set_params(init)
        eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
        eng.residual(fetch=False)
        first = 1
        for name, lam in (("off", None), ("on", [1.0, 1.0, 1.0]), ("off_again", None)):
            if lam is None:
                eng.prior_end()
            else:
                eng.prior_begin(lam)
            eng.mh_sweeps(args.sweeps, first)          # warm-up
            first += args.sweeps
            ms = []
            for _ in range(args.runs):
                eng.timer_start()
                eng.mh_sweeps(args.sweeps, first)
                ms.append(eng.timer_stop() / args.sweeps)
                first += args.sweeps
            out["ms_per_sweep_" + name] = float(np.median(ms))
            out["ms_per_sweep_%s_all" % name] = [round(float(v), 4) for v in ms]
        eng.prior_energy()                             # warm-up (allocates the partials)
        calls = []
        for _ in range(20):
            eng.sync()
            t0 = time.perf_counter()
            eng.prior_energy()
            calls.append((time.perf_counter() - t0) * 1e3)
        out["prior_energy_call_ms"] = float(np.median(calls))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
