"""Cost of one sample of the pointwise predictive accuracy (d3d_pred_*, k_pred_accum) on one GPU:

    python tools/predictive_time.py [shapes=128,300,300] [post_nt=0,1]

At 300x300x128 (the bench's config 3: Moffat 11x11, 17-tap LSF), per value of the option post_nt:
  * one d3d_post_accumulate with the moments of the parameter map alone (what = 0: a launch over
    H W spaxels, the floor of the call), then the same call with d3d_pred_begin armed -- the
    difference is k_pred_accum, 80 bytes per voxel (0.92 GB at this shape), printed with its
    traffic floor at 6.3 TB/s;
  * beside it one full posterior sample (what = 3: forward model into SLOT_SIM and k_post_accum, 72
    bytes per voxel) and that sample with the predictive accumulators;
  * beside the sweep: ms per sweep of d3d_mh_sweeps with the moments scheduled after every sweep,
    without and with the predictive accumulators -- the difference holds the write-back of the pending
    residual layers a predictive sample needs -- and with nothing scheduled (the 4.9 ms sweep).

HIP events on the context's stream after a warm-up; every figure is the median of 7 batches
(tools/posterior_time.py's method).  Writes profiles/predictive_time.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.get("shapes", "128,300,300").split(":")]
POST_NT = [int(v) for v in args.get("post_nt", "0,1").split(",")]
HBM_TBS = 6.3
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def engine(D, H, W, post_nt):
    import bench as B
    from deconv3d_amd import _lib
    fsf, lsf = B.build_taps(D, 11)
    eng = _lib.Engine((D, H, W), fsf.shape, options={"post_nt": post_nt})
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


def sample_us(eng, what, predictive):
    eng.post_begin(what)
    if predictive:
        eng.pred_begin()
    return median_us(eng, eng.post_accumulate, 20)


def sweep_ms(eng, scheduled, predictive):
    eng.post_begin(3)
    if predictive:
        eng.pred_begin()
    eng.post_schedule(0 if scheduled else 10 ** 9, 1)
    state = {"s": 1}

    def call():
        eng.mh_sweeps(5, state["s"])
        state["s"] += 5

    return median_us(eng, call, 2, batches=5, warm=1) / 5e3


for D, H, W in SHAPES:
    for post_nt in POST_NT:
        with engine(D, H, W, post_nt) as eng:
            tag = "%dx%dx%d post_nt %d" % (W, H, D, post_nt)
            voxels = float(D) * H * W
            floor = voxels * 80 / (HBM_TBS * 1e6)
            base, pred = sample_us(eng, 0, False), sample_us(eng, 0, True)
            say("%s map moments alone %8.1f us; with k_pred_accum %8.1f us; k_pred_accum %8.1f us   %.0f MB at 80 "
                "B/voxel, floor %.1f us at %.1f TB/s, ratio %.2f"
                % (tag, base, pred, pred - base, voxels * 80 / 1e6, floor, HBM_TBS, (pred - base) / floor))
            full, both = sample_us(eng, 3, False), sample_us(eng, 3, True)
            say("%s a posterior sample (forward model + k_post_accum, 72 B/voxel) %8.1f us; with k_pred_accum %8.1f us"
                % (tag, full, both))
            none, post, post_pred = sweep_ms(eng, False, False), sweep_ms(eng, True, False), sweep_ms(eng, True, True)
            say("%s beside the sweep: %.4f ms per sweep with nothing scheduled, %.4f with the moments after every "
                "sweep, %.4f with the predictive accumulators too (difference %.1f us)"
                % (tag, none, post, post_pred, (post_pred - post) * 1e3))
            eng.post_end()

out = os.path.join(ROOT, "profiles", "predictive_time.txt")
with open(out, "w") as f:
    f.write("# python tools/predictive_time.py %s\n" % " ".join(sys.argv[1:]))
    f.write("\n".join(LINES) + "\n")
print("wrote", out)
