"""Cost of the Student-t weights' redraw (d3d_robust_*, k_robust_step) on one GPU:

    python tools/robust_time.py [shapes=128,300,300:256,300,300] [nus=3,4]

At 300x300x128 (the bench's config 3: Moffat 11x11, 17-tap LSF) and 300x300x256, for nu = 3 and 4:
  * the step alone: us per d3d_robust_step with and without the running mean (40 and 24 bytes per
    voxel), HIP events around batches of calls -- each call ends with a stream synchronisation, so
    the figure holds the gap of one empty synchronisation, printed beside it;
  * beside the sweep: ms per sweep of d3d_mh_sweeps armed with a start never reached (no draw: the
    Gaussian chain on the per-voxel kernels) and with every = 1; the difference is what a draw costs
    in place -- the write-back of the pending layers, the kernel, the overlap the sweep loses;
  * the traffic floor: the bytes the kernel moves at 6.3 TB/s, and the ratio to it.
Then, at the first shape, nu = 1, 3, 4, 29, 30 without the mean: 29 against 3 adds seven Philox
blocks and no libm call, 4 against 3 adds one block, one log and one cos -- which of the two takes
the issue slots.

HIP events on the context's stream after a warm-up; every figure is the median of 7 batches
(tools/posterior_time.py's method).  profiles/robust_time.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.get("shapes", "128,300,300:256,300,300").split(":")]
NUS = [int(v) for v in args.get("nus", "3,4").split(",")]
NEVER = 10 ** 9
HBM_TBS = 6.3


def engine(D, H, W):
    import bench as B
    from deconv3d_amd import _lib
    fsf, lsf = B.build_taps(D, 11)
    eng = _lib.Engine((D, H, W), fsf.shape)
    eng.set_taps(fsf, lsf)
    data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
    eng.set_data(data, var)
    eng.set_params(init)
    eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
    eng.residual(fetch=False)
    return eng


def median_us(eng, call, per_batch, batches=7, warm=2):
    for _ in range(warm):
        call()
    eng.sync()
    out = []
    for _ in range(batches):
        eng.timer_start()
        for _ in range(per_batch):
            call()
        out.append(eng.timer_stop() * 1e3 / per_batch)
    return float(np.median(out))


def step_us(eng, nu, mean):
    eng.robust_begin(nu, 1, NEVER, 0 if mean else NEVER)
    return median_us(eng, lambda: eng.robust_step(1), 20)


def sweep_ms(eng, nu, every_one):
    eng.robust_begin(nu, 1, 0 if every_one else NEVER, 0)
    state = {"s": 1}

    def call():
        eng.mh_sweeps(5, state["s"])
        state["s"] += 5

    return median_us(eng, call, 2, batches=5, warm=1) / 5e3


for k, (D, H, W) in enumerate(SHAPES):
    with engine(D, H, W) as eng:
        voxels = float(D) * H * W
        gap = median_us(eng, eng.sync, 20)
        print("%dx%dx%d: an empty stream synchronisation between events %.1f us" % (W, H, D, gap), flush=True)
        for nu in NUS:
            for mean, nbytes in ((True, 40), (False, 24)):
                us = step_us(eng, nu, mean)
                floor = voxels * nbytes / (HBM_TBS * 1e6)
                print("%dx%dx%d nu %2d step alone, %s  %8.1f us   %5.0f MB at %d B/voxel, floor %6.1f us at %.1f TB/s, "
                      "ratio %.2f" % (W, H, D, nu, "with the mean" if mean else "no mean     ", us, voxels * nbytes / 1e6,
                                      nbytes, floor, HBM_TBS, us / floor), flush=True)
            off, on = sweep_ms(eng, nu, False), sweep_ms(eng, nu, True)
            print("%dx%dx%d nu %2d beside the sweep: %.4f ms per sweep without a draw, %.4f with every = 1, "
                  "difference %.1f us" % (W, H, D, nu, off, on, (on - off) * 1e3), flush=True)
        if k == 0:
            for nu in (1, 3, 4, 29, 30):
                m = (nu + 1) // 2
                blocks = (m + (2 if nu % 2 == 0 else 0) + 1) // 2
                print("%dx%dx%d nu %2d step alone, no mean: %8.1f us  (%d Philox blocks, %d log, %d cos per voxel)"
                      % (W, H, D, nu, step_us(eng, nu, False), blocks, 1 + (nu % 2 == 0), int(nu % 2 == 0)), flush=True)
        eng.robust_end()
