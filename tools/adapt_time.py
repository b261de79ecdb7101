"""Cost of the per-spaxel jump scales (d3d_adapt_*), off and on: MH sweep time of one context at
64x64x64 (k_mh_small, us per launch) and 300x300x128 (the bench's config 3, ms per sweep).
    python tools/adapt_time.py [DxHxW ...]
One line per shape and mode.  For the A/B against the parent commit build its library beside this
one (tools/build_variant.sh) and run this tool under DECONV3D_HIP_LIB=<that library>, interleaved
with runs of this build: a library without the entry points is timed with the feature off only.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deconv3d_amd import _lib  # noqa: E402

HAVE = hasattr(ctypes.CDLL(_lib.LIB_PATH), "d3d_adapt_begin")
if not HAVE:          # the parent commit's library: bind what it has
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if s not in _lib.ADAPT_PROTOTYPES]
    _lib.ADAPT_PROTOTYPES.clear()
import bench as B  # noqa: E402

shapes = sys.argv[1:] or ["64x64x64", "128x300x300"]
for spec in shapes:
    D, H, W = [int(v) for v in spec.lower().split("x")]
    fsf, lsf = B.build_taps(D, 11)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        data, var, truth, init, mn, mx = B.synthetic_inputs(eng, D, H, W, fsf, 777)
        eng.set_data(data, var, mask=None)
        del data, var
        n = 100 if D * H * W < (1 << 22) else 20
        for mode in (("off", "on") if HAVE else ("off",)):
            eng.set_params(init)
            eng.mh_config(mn, mx, 0.1, float(mx[0] ** 2), seed=777, refresh_every=0)
            if mode == "on":      # a window of 10: two steps of k_mh_adapt inside the timed sweeps
                eng.adapt_begin(0.25, 10, 1 << 30, 2.0, (1e-3, 1e3))
            eng.residual(fetch=False)
            eng.mh_sweeps(3, 1)
            eng.sync()
            best = []
            for rep in range(3):
                eng.timer_start()
                eng.mh_sweeps(n, 4 + rep * n)
                best.append(eng.timer_stop() / n)
            ms = sorted(best)[1]
            print("adapt=%s lib=%s %dx%dx%d: %.4f ms per sweep, %.3f us per launch (median of 3 x %d sweeps)"
                  % (mode, "this" if HAVE else "parent", D, H, W, ms, ms * 1e3 / 121, n), flush=True)
            if mode == "on":
                eng.adapt_end()
