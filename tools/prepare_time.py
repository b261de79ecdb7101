"""Cost of preparing a raw cube (d3d_running_median, d3d_channel_stats, d3d_prepare): device time
of the running-median kernel and of the channel median / MAD kernel at 300x300x128 (the bench's
config 3) and 64x64x64, by the HIP events the calls record around them.
    python tools/prepare_time.py [DxHxW[:window] ...]
One line per shape: microseconds (medians of 5), the rate of window comparisons of the running
median ((2 h + 1)^2 per voxel, two compares each), and the whole d3d_prepare call with its
rejection pass, allocations and copies, beside the 4.9 ms of one MH sweep at 300x300x128.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deconv3d_amd import _lib  # noqa: E402

SWEEP_MS = 4.9                   # one MH sweep at 300x300x128

shapes = sys.argv[1:] or ["128x300x300:51", "64x64x64:51"]
for spec in shapes:
    spec, _, window = spec.partition(":")
    D, H, W = [int(v) for v in spec.lower().split("x")]
    h = int(window or 51) // 2
    rng = np.random.default_rng(777)
    # noise with a channel-dependent factor on a sloped continuum, a few NaN voxels
    cube = rng.normal(0., 1., (D, H, W)) * (1. + 2. * rng.random(D))[:, None, None]
    cube += 20. * rng.random((H, W))[None] + 0.05 * np.arange(float(D))[:, None, None]
    cube[rng.random(cube.shape) < 1e-4] = np.nan
    with _lib.Engine((D, H, W), (1, 1)) as eng:
        eng.running_median(cube, h)              # (warm-up: code objects, allocator)
        eng.channel_stats(cube)
        median, stats, both_m, both_s, wall = [], [], [], [], []
        for rep in range(5):
            eng.running_median(cube, h)
            median.append(eng.get_option("prep_median_ns") / 1e3)
            eng.channel_stats(cube)
            stats.append(eng.get_option("prep_stats_ns") / 1e3)
            t0 = time.perf_counter()
            sigma = eng.prepare(cube, h, 3.0)[3]
            wall.append(time.perf_counter() - t0)
            both_m.append(eng.get_option("prep_median_ns") / 1e3)
            both_s.append(eng.get_option("prep_stats_ns") / 1e3)
        he = min(h, max(D - 1, 1))
        pairs = float(D) * H * W * (2 * he + 1) ** 2
        us_m, us_s = float(np.median(median)), float(np.median(stats))
        print("%dx%dx%d, window %d: running median %.1f us (%.2f T window pairs/s; %.2f of a %.1f ms sweep), "
              "channel median/MAD %.1f us (%.2f of a sweep); d3d_prepare with reject=3: kernels %.1f + %.1f us "
              "(both passes), whole call %.1f ms with its allocations and copies; %d of %d channels have a sigma "
              "(medians of 5)" % (D, H, W, 2 * h + 1, us_m, pairs / (us_m * 1e-6) / 1e12, us_m / 1e3 / SWEEP_MS,
                                  SWEEP_MS, us_s, us_s / 1e3 / SWEEP_MS, float(np.median(both_m)),
                                  float(np.median(both_s)), 1e3 * float(np.median(wall)),
                                  int(np.isfinite(sigma).sum()), D), flush=True)
