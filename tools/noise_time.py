"""Cost of the noise scales' redraw (d3d_noise_*: k_noise_sums, k_noise_draw, k_noise_apply) on one GPU:

    python tools/noise_time.py [shapes=128,300,300:256,300,300] [pers=channel,cube]

At 300x300x128 (the bench's config 3: Moffat 11x11, 17-tap LSF) and 300x300x256, per='channel' and 'cube':
  * the three kernels alone: us each by the option noise_timing (HIP events between the launches of
    d3d_noise_step, read back as noise_sums_ns / noise_draw_ns / noise_apply_ns), medians of 21 steps;
  * the step alone: us per d3d_noise_step, HIP events around batches of calls -- each call ends with a
    stream synchronisation, so the figure holds the gap of one empty synchronisation, printed beside it;
  * beside the sweep: ms per sweep of d3d_mh_sweeps armed with a start never reached (no draw: the chain
    on the per-voxel kernels) and with every = 1; the difference is what a draw costs in place -- the
    write-back of the pending layers, the three kernels, the overlap the sweep loses;
  * the traffic floor: 32 bytes per voxel (16 read by k_noise_sums, 16 read and written by
    k_noise_apply) at 6.3 TB/s, the stream rate DESIGN.md section 8l uses, and the ratio to it.

HIP events on the context's stream after a warm-up; every figure is a median (tools/robust_time.py's
method).  profiles/noise_time.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.get("shapes", "128,300,300:256,300,300").split(":")]
PERS = args.get("pers", "channel,cube").split(",")
NEVER = 10 ** 9
HBM_TBS = 6.3
KERNELS = ("sums", "draw", "apply")


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


def group_of(per, D):
    return np.arange(D) if per == "channel" else np.zeros(D, dtype=int)


def kernels_us(eng, per, D):
    eng.noise_begin(group_of(per, D), start=NEVER, capacity=64)
    eng.set_option("noise_timing", 1)
    rows = []
    for s in range(24):
        eng.noise_step(s)
        rows.append([eng.get_option("noise_%s_ns" % k) / 1e3 for k in KERNELS])
    eng.set_option("noise_timing", 0)
    return np.median(rows[3:], axis=0)


def step_us(eng, per, D):
    eng.noise_begin(group_of(per, D), start=NEVER, capacity=7 * 20 + 2)
    return median_us(eng, lambda: eng.noise_step(1), 20)


def sweep_ms(eng, per, D, every_one):
    eng.noise_begin(group_of(per, D), start=0 if every_one else NEVER, capacity=64)
    state = {"s": 1}

    def call():
        eng.mh_sweeps(5, state["s"])
        state["s"] += 5

    return median_us(eng, call, 2, batches=5, warm=1) / 5e3


for D, H, W in SHAPES:
    with engine(D, H, W) as eng:
        voxels = float(D) * H * W
        gap = median_us(eng, eng.sync, 20)
        floor = voxels * 32 / (HBM_TBS * 1e6)
        print("%dx%dx%d: an empty stream synchronisation between events %.1f us; %.0f MB at 32 B/voxel, floor %.1f us "
              "at %.1f TB/s" % (W, H, D, gap, voxels * 32 / 1e6, floor, HBM_TBS), flush=True)
        for per in PERS:
            k = kernels_us(eng, per, D)
            print("%dx%dx%d per=%-7s kernels alone: k_noise_sums %7.1f us, k_noise_draw %7.1f us, k_noise_apply %7.1f us, "
                  "together %7.1f us, ratio to the floor %.2f" % (W, H, D, per, k[0], k[1], k[2], k.sum(), k.sum() / floor),
                  flush=True)
            us = step_us(eng, per, D)
            print("%dx%dx%d per=%-7s step alone %7.1f us, ratio to the floor %.2f" % (W, H, D, per, us, us / floor),
                  flush=True)
            off, on = sweep_ms(eng, per, D, False), sweep_ms(eng, per, D, True)
            print("%dx%dx%d per=%-7s beside the sweep: %.4f ms per sweep without a draw, %.4f with every = 1, "
                  "difference %.1f us" % (W, H, D, per, off, on, (on - off) * 1e3), flush=True)
        eng.noise_end()
