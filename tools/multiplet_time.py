"""Cost of the multiplet line model (GaussianMultipletLineModel, d3d_set_line_shape) on one GPU:

    python tools/multiplet_time.py [sweeps=N] [host=0]

ms per MH-within-Gibbs sweep, HIP-event timed on the context's stream, for the default context (the
single Gaussian), the multiplet with K = 1, 2 and 3, at the bench's config-3 shape 300x300x128
(Moffat 11x11 FSF, 17-tap LSF), 64^3, and a 600-channel cube (z-blocked sweep kernels); us per
Engine.forward() at 300x300x128; and one sweep of the HOST path (a GaussianMultipletLineModel
subclass that overrides modelize, evaluated by host_model.HostModelChain) with the K = 2 shape at
300x300x128.  Prints one line per measurement (profiles/multiplet_time.txt)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
import deconv3d_amd as d3d  # noqa: E402
from deconv3d_amd import _lib  # noqa: E402
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction  # noqa: E402

SHAPES = [("single Gaussian", None), ("K=1", ([0.], [1.])), ("K=2", ([0., 3.8], [1., 1.4])),
          ("K=3", ([0., -14.5, 15.2], [1., 0.34, 0.11]))]
CUBES = [(128, 300, 300), (64, 64, 64), (600, 96, 96)]
args = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
n_sweeps = int(args.get("sweeps", 10))


def engine(D, H, W, shape):
    fsf, lsf = B.build_taps(D, 11)
    eng = _lib.Engine((D, H, W), fsf.shape)
    eng.set_taps(fsf, lsf)
    data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
    eng.set_data(data, var)
    if shape is not None:
        eng.set_line_shape(*shape)
    eng.set_params(init)
    eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
    return eng, (fsf, lsf, data, var, init)


for D, H, W in CUBES:
    for label, shape in SHAPES:
        eng, _ = engine(D, H, W, shape)
        with eng:
            eng.mh_sweeps(2, 1)                  # warm-up (first launches, tables)
            eng.sync()
            eng.timer_start()
            eng.mh_sweeps(n_sweeps, 3)
            ms = eng.timer_stop() / n_sweeps
        print("sweep %dx%dx%d %-16s %9.3f ms per sweep" % (W, H, D, label, ms), flush=True)

for label, shape in SHAPES[1:]:
    eng, _ = engine(128, 300, 300, shape)
    with eng:
        for _ in range(3):
            eng.forward(fetch=False)
        eng.sync()
        eng.timer_start()
        for _ in range(20):
            eng.forward(fetch=False)
        us = eng.timer_stop() / 20 * 1e3
    print("forward 300x300x128 %-16s %9.1f us" % (label, us), flush=True)

if args.get("host", "1") != "0":
    class HostDoublet(d3d.GaussianMultipletLineModel):
        """The same curve through the host path (modelize overridden)."""

        def modelize(self, runner, x, parameters):
            return d3d.GaussianMultipletLineModel.modelize(self, runner, x, parameters)

    D, H, W = 128, 300, 300
    eng, (fsf, lsf, data, var, init) = engine(D, H, W, None)
    eng.close()
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    model = HostDoublet(*SHAPES[2][1])
    kw = dict(variance=var, model=model, initial_parameters=init, min_acceptance_rate=0., seed=1)
    t0 = time.perf_counter()
    d3d.Run(cube, inst, max_iterations=1, **kw)            # setup only
    t1 = time.perf_counter()
    d3d.Run(cube, inst, max_iterations=2, **kw)            # setup + one sweep
    t2 = time.perf_counter()
    print("host path 300x300x128 K=2 %9.1f ms per sweep (Run wall time minus its setup)"
          % (((t2 - t1) - (t1 - t0)) * 1e3), flush=True)
