"""Cost of the posterior moments kept on the device (d3d_post_*, k_post_accum) on one GPU:

    python tools/posterior_time.py [parent=<libdeconv3d_hip.so of the parent commit>] [sweeps=N]

1. k_post_accum at 300x300x128, 300x300x256 and 64^3, with plain and with non-temporal accesses
   (option post_nt): us per d3d_post_accumulate of both cubes minus us per d3d_forward (the
   accumulate call is the forward model into SLOT_SIM followed by the kernel, on one stream), and
   the kernel's 9 * 8 * Dp * H * W bytes over that time as a fraction of the 8 TB/s peak -- beside
   k_chi2_map's fraction (16 * Dp * H * W bytes) from the same process, the project's plain streaming
   kernel.
2. ms per sweep of the bench's config 3 (300x300x128, Moffat 11x11, 17-tap LSF) with the schedule off,
   every = 1 and every = 10 -- and, given parent=, with the parent commit's library (built by
   tools/build_variant.sh from a checkout of that commit), timed twice: the spread between those two
   is what "equal" can mean on this box.

HIP events on the context's stream after a warm-up; every figure is the median of 7 batches.  Each row
of part 2 is a process of its own (DECONV3D_HIP_LIB selects the library).  profiles/posterior_time.txt."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
n_sweeps = int(args.get("sweeps", 10))
PEAK = 8e12  # bytes / s


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
    return eng


def median_ms(eng, call, per_batch, batches=7, warm=3):
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


def kernels():
    for D, H, W in ((128, 300, 300), (256, 300, 300), (64, 64, 64)):
        with engine(D, H, W) as eng:
            Dp = D + (D & 1)
            eng.residual(fetch=False)
            chi = median_ms(eng, lambda: eng.chi2_map(fetch=False), 20) * 1e3
            fwd = median_ms(eng, lambda: eng.forward(fetch=False), 20) * 1e3
            print("%dx%dx%d k_chi2_map %8.1f us  %.2f of peak;  forward %8.1f us"
                  % (W, H, D, chi, 16. * Dp * H * W / (chi * 1e-6) / PEAK, fwd), flush=True)
            for nt in (0, 1):
                eng.set_option("post_nt", nt)
                eng.post_begin()
                acc = median_ms(eng, eng.post_accumulate, 20) * 1e3
                k = acc - fwd
                print("%dx%dx%d post_nt=%d accumulate %8.1f us, k_post_accum %8.1f us  %.2f of peak"
                      % (W, H, D, nt, acc, k, 72. * Dp * H * W / (k * 1e-6) / PEAK), flush=True)
                eng.post_end()


def sweeps(every):
    from deconv3d_amd import _lib
    if every < 0:      # the parent commit's library has no d3d_post_*
        _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if s not in _lib.POST_PROTOTYPES]
        _lib.POST_PROTOTYPES.clear()
    with engine(128, 300, 300) as eng:
        if every > 0:
            eng.post_begin()
            eng.post_schedule(1, every)
        first = [1]

        def call():
            eng.mh_sweeps(n_sweeps, first[0])
            first[0] += n_sweeps
        print("%.4f" % median_ms(eng, call, 1, warm=2), flush=True)


def child(every, lib=None):
    env = dict(os.environ)
    if lib:
        env["DECONV3D_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "mode=sweeps", "every=%d" % every,
                          "sweeps=%d" % n_sweeps], env=env, check=True, capture_output=True, text=True, timeout=600)
    return float(out.stdout.strip().splitlines()[-1]) / n_sweeps


if args.get("mode") == "sweeps":
    sweeps(int(args["every"]))
elif args.get("mode") == "kernels":
    kernels()
else:
    subprocess.run([sys.executable, os.path.abspath(__file__), "mode=kernels"], check=True, timeout=900)
    rows = []
    if args.get("parent"):
        rows += [("parent commit's library", -1, args["parent"]), ("parent commit's library, again", -1, args["parent"])]
    rows += [("schedule off", 0, None), ("every = 1", 1, None), ("every = 10", 10, None), ("schedule off, again", 0, None)]
    for label, every, lib in rows:
        print("sweep 300x300x128 %-32s %8.3f ms per sweep" % (label, child(every, lib)), flush=True)
