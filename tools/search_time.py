"""Cost of the matched-filter line search (d3d_line_search): device time of the template bank's
build and of the search kernel at 300x300x128 (the bench's config 3) and 64x64x64, default grid
(8 widths x D centres), by the HIP events the call records around them.
    python tools/search_time.py [DxHxW ...]
One line per shape: microseconds, and the search kernel's share of the fp64 vector peak for its
4 n_cand D HW flops (N and Q: two multiply-adds per candidate, channel and spaxel), beside the
4.9 ms of one MH sweep at 300x300x128.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deconv3d_amd import _lib, search  # noqa: E402
import bench as B  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12       # MI355X, flop/s
SWEEP_MS = 4.9                   # one MH sweep at 300x300x128

shapes = sys.argv[1:] or ["128x300x300", "64x64x64"]
for spec in shapes:
    D, H, W = [int(v) for v in spec.lower().split("x")]
    fsf, lsf = B.build_taps(D, 11)
    centres, widths, _ = search.check_grid(None, None, D)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        data, var = B.synthetic_inputs(eng, D, H, W, fsf, 777)[:2]
        eng.set_data(data, var, mask=None)
        del data, var
        eng.line_search(centres, widths)          # (warm-up: code objects, allocator)
        bank, kern, wall = [], [], []
        for rep in range(5):
            t0 = time.perf_counter()
            best, _ = eng.line_search(centres, widths)
            wall.append(time.perf_counter() - t0)
            bank.append(eng.get_option("search_bank_ns") / 1e3)
            kern.append(eng.get_option("search_kernel_ns") / 1e3)
        n_cand = centres.size * widths.size
        flops = 4. * n_cand * D * H * W
        us = float(np.median(kern))
        print("%dx%dx%d, %d x %d candidates: bank %.1f us, search %.1f us (%.1f %% of the fp64 vector peak; "
              "%.2f of a %.1f ms sweep), whole call %.2f ms with its allocations and copies; %d of %d detected "
              "(medians of 5)" % (D, H, W, widths.size, centres.size, float(np.median(bank)), us,
                                  100. * flops / (us * 1e-6) / FP64_VECTOR_PEAK, us / 1e3 / SWEEP_MS, SWEEP_MS,
                                  1e3 * float(np.median(wall)), int((best >= 0).sum()), H * W), flush=True)
