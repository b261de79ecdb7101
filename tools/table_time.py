"""Cost of the tabulated line model (TabulatedLineModel, d3d_set_line_table) on one GPU:

    python tools/table_time.py [sweeps=N]

ms per MH-within-Gibbs sweep and us per Engine.forward() -- the forward model with its line
launch; the rows differ in that launch alone -- HIP-event timed on the context's stream, median
of 5 after a warm-up, at the bench's config-3 shape 300x300x128 (Moffat 11x11 FSF, 17-tap LSF) for
the single Gaussian (the MULTI = false kernels), the Gaussian as a table (n = 2049, support 8),
the Gaussian doublet and the same doublet as a table (the MULTI = true kernels, exp against table
read).  Prints one line per measurement (profiles/table_time.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
import deconv3d_amd as d3d  # noqa: E402
from deconv3d_amd import _lib  # noqa: E402

DOUBLET = ([0., 3.8], [1., 1.4])
U = np.linspace(-8., 8., 2049)
LINES = [("single Gaussian", d3d.SingleGaussianLineModel()),
         ("Gaussian table", d3d.TabulatedLineModel(np.exp(-U ** 2 / 2.), 8.)),
         ("doublet", d3d.GaussianMultipletLineModel(*DOUBLET)),
         ("doublet table", d3d.TabulatedLineModel(np.exp(-U ** 2 / 2.), 8., *DOUBLET))]
D, H, W = 128, 300, 300
REPEATS = 5
args = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
n_sweeps = int(args.get("sweeps", 10))


def engine(model):
    fsf, lsf = B.build_taps(D, 11)
    eng = _lib.Engine((D, H, W), fsf.shape)
    eng.set_taps(fsf, lsf)
    data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
    eng.set_data(data, var)
    if not isinstance(model, d3d.SingleGaussianLineModel):
        eng.set_line_shape(model.offsets, model.ratios)
    if isinstance(model, d3d.TabulatedLineModel):
        eng.set_line_table(model.table, model.support, model.table_integral)
    eng.set_params(init)
    eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
    return eng


for label, model in LINES:
    with engine(model) as eng:
        eng.mh_sweeps(2, 1)                  # warm-up (first launches, tables)
        eng.sync()
        times = []
        for r in range(REPEATS):
            eng.timer_start()
            eng.mh_sweeps(n_sweeps, 3 + r * n_sweeps)
            times.append(eng.timer_stop() / n_sweeps)
    print("sweep %dx%dx%d %-16s %9.3f ms per sweep (median of %d; min %.3f, max %.3f)"
          % (W, H, D, label, float(np.median(times)), REPEATS, min(times), max(times)), flush=True)

for label, model in LINES:
    with engine(model) as eng:
        for _ in range(3):
            eng.forward(fetch=False)
        eng.sync()
        times = []
        for r in range(REPEATS):
            eng.timer_start()
            for _ in range(20):
                eng.forward(fetch=False)
            times.append(eng.timer_stop() / 20 * 1e3)
    print("forward %dx%dx%d %-16s %9.1f us (median of %d; min %.1f, max %.1f)"
          % (W, H, D, label, float(np.median(times)), REPEATS, min(times), max(times)), flush=True)
