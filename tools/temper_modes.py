"""Does replica exchange let the cold chain leave a wrong mode of c?  One bimodal synthetic case:

    python tools/temper_modes.py [sweeps=1000] [rungs=6] [beta_min=0.02] [off=10] [size=64]

The cube of examples/quickstart.py (64 channels, size x size spaxels, default MUSE instrument, noise 2 % of the peak), every
spaxel started at the truth with its centre `off` channels away: the line it should fit lies outside
the reach of a local step, and the neighbours -- started wrong alike -- explain part of its flux.  The
share of the bright spaxels (a > 3) whose mean c over the last quarter of the chain lies within one
channel of the truth, without tempering and with it (cold rung), at equal sweeps per rung; the swap
rates per pair and the rungs' mean energies.  Reported as measured: DESIGN.md section 8i.

    python tools/temper_modes.py --patch P [...]

adds the same ladder with the exchange of patches of P x P spaxels (Run(tempering=dict(..., patch=P)):
DESIGN.md section 8j); `--patch 1,2,4,10` runs one after the other."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deconv3d_amd import MUSE, Run, _lib  # noqa: E402

args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
if "--patch" in sys.argv:
    args["patch"] = sys.argv[sys.argv.index("--patch") + 1]
patches = [int(v) for v in args["patch"].split(",")] if args.get("patch") else []
sweeps, rungs = int(args.get("sweeps", 1000)), int(args.get("rungs", 6))
beta_min, off = float(args.get("beta_min", 0.02)), float(args.get("off", 10))
D = 64
H = W = int(args.get("size", 64))
rng = np.random.default_rng(7)
inst = MUSE()
y, x = np.indices((H, W))
r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
truth = np.dstack((12.0 * np.exp(-r2 / (2. * (H / 5.) ** 2)),
                   D / 2. + (D / 7.) * np.tanh((x - W / 2.) / (W / 7.)),
                   1.6 + 0.8 * np.exp(-r2 / (2. * (H / 8.) ** 2))))
probe = inst.build_cube(np.zeros((D, H, W)))
fsf, lsf = inst.fsf.as_image(probe), inst.lsf.as_vector(probe)
with _lib.Engine((D, H, W), fsf.shape) as eng:
    eng.set_taps(fsf, lsf)
    eng.set_params(truth)
    clean = eng.forward()
sigma = 0.02 * clean.max()
cube = inst.build_cube(clean + rng.normal(0., sigma, clean.shape))
start = truth.copy()
start[..., 1] += off
bright = truth[..., 0] > 3.0
kw = dict(variance=np.full(clean.shape, sigma ** 2), max_iterations=sweeps, min_acceptance_rate=0.,
          jump_amplitude=[0., 0.5, 0.2], gibbs_apriori_variance=100., seed=1, initial_parameters=start,
          sweeps_per_call=64)
for label, more in (("without tempering", {}),
                    ("tempering, %d rungs down to beta %g, swap_every 1" % (rungs, beta_min),
                     dict(tempering=dict(rungs=rungs, beta_min=beta_min)))) + tuple(
        ("tempering, %d rungs down to beta %g, patch %d" % (rungs, beta_min, p),
         dict(tempering=dict(rungs=rungs, beta_min=beta_min, patch=p))) for p in patches):
    t0 = time.perf_counter()
    run = Run(cube, inst, **dict(kw, **more))
    dt = time.perf_counter() - t0
    c = run.chain[3 * sweeps // 4:, ..., 1].mean(axis=0)
    share = float((np.abs(c - truth[..., 1])[bright] <= 1.).mean())
    print("%dx%dx%d %-52s %d sweeps per rung in %.1f s: %.1f %% of the %d bright spaxels within 1 channel of the true c "
          "(median |c - truth| %.2f)" % (W, H, D, label, sweeps, dt, 100. * share, bright.sum(),
                                        np.median(np.abs(c - truth[..., 1])[bright])), flush=True)
    if run.tempering is not None:
        print("    betas %s\n    swap rates %s\n    energy mean %s\n    energy std %s\n    labels %s" % (
            np.round(run.tempering.betas, 4), np.round(run.tempering.swap_rates, 3),
            np.round(run.tempering.energy_mean, 1), np.round(run.tempering.energy_std, 1), run.tempering.labels),
            flush=True)
        if run.tempering.patch is not None:
            print("    patch rates %s of %s proposed" % (np.round(run.tempering.patch_rates, 3),
                                                        run.tempering.patch_attempts), flush=True)
