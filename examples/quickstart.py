#!/usr/bin/env python
# coding=utf-8
"""
Quick start: deconvolve a synthetic MUSE-like cube on one MI355X.

    python examples/quickstart.py [iterations] [chains]

Builds a 64x64x64 cube of one Gaussian emission line per spaxel (a rotating
disc seen through the default MUSE instrument: Gaussian FSF, Gaussian LSF),
adds noise, runs the MH-within-Gibbs chain through the same `Run` call a user
of irap-omp/deconv3d would write (lib/run.py:95-109), and prints how well the
posterior means recover the line centres and widths.  With a FITS file:

    cube = Cube.from_fits('my_cube.fits')
    run = Run(cube, MUSE(fsf_fwhm=0.8841), mask=above_snr(cube, MUSE(fsf_fwhm=0.8841), 5.),
              initial_search=True, max_iterations=4000)
    run.save('my_run')
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deconv3d_amd import MUSE, Run, _lib, regions  # noqa: E402

iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
D = H = W = 64
rng = np.random.default_rng(7)
inst = MUSE()                                       # Gaussian FSF (1" seeing) + Gaussian LSF
y, x = np.indices((H, W))
r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
truth = np.dstack((12.0 * np.exp(-r2 / (2. * (H / 5.) ** 2)),             # amplitude
                   D / 2. + (D / 7.) * np.tanh((x - W / 2.) / (W / 7.)),   # centre: rotation curve
                   1.6 + 0.8 * np.exp(-r2 / (2. * (H / 8.) ** 2))))        # width

# the noiseless observation comes from the device forward model
probe = inst.build_cube(np.zeros((D, H, W)))
fsf, lsf = inst.fsf.as_image(probe), inst.lsf.as_vector(probe)
with _lib.Engine((D, H, W), fsf.shape) as eng:
    eng.set_taps(fsf, lsf)
    eng.set_params(truth)
    clean = eng.forward()
sigma = 0.02 * clean.max()
cube = inst.build_cube(clean + rng.normal(0., sigma, clean.shape))

t0 = time.perf_counter()
run = Run(cube, inst, variance=np.full(clean.shape, sigma ** 2), max_iterations=iterations,
          keep_one_in=10, min_acceptance_rate=0., jump_amplitude=[0., 0.5, 0.2],
          gibbs_apriori_variance=100., seed=1,   # amplitude prior, as tests/read_mat.py:109-119 sets one
          posterior_burn_in=max(1, iterations // 2),   # mean / std of the samples' cubes, kept on the device
          regions=regions.annuli((H, W), (H / 2., W / 2.), [0., 4., 8., 12., 16.]))   # ... and four rings' (F, C, S)
dt = time.perf_counter() - t0
burn = run.chain.shape[0] // 2
post = run.chain[burn:].mean(axis=0)                # posterior means over the second half
last = run.simulate_convolved(cube.data.shape, run.chain[-1])      # forward model of the last sample
model = run.convolved_cube.data                     # ... and of the extracted (mean) parameters
print("%d iterations of %d spaxels in %.1f s (%.2f M spaxel-updates/s including setup)" % (
    iterations, H * W, dt, iterations * H * W / dt / 1e6))
print("reduced chi2: last sample %.4f, extracted parameters %.4f; their convolved model vs the noiseless cube: "
      "rms %.2f %% of its peak" % (np.mean(((cube.data - last) / sigma) ** 2),
                                   np.mean(((cube.data - model) / sigma) ** 2),
                                   100. * np.sqrt(np.mean((model - clean) ** 2)) / clean.max()))
# The mean of the samples' convolved CUBES (run.posterior, accumulated on the device over the second
# half of the sweeps) beside the cube of the mean parameter MAP (run.convolved_cube)
post_cube = run.posterior.convolved_mean
print("reduced chi2: posterior mean cube %.4f (%d samples; median error bar %.3g) beside the cube of the mean map %.4f" % (
    np.mean(((cube.data - post_cube) / sigma) ** 2), run.posterior.count, np.median(run.posterior.convolved_std),
    np.mean(((cube.data - model) / sigma) ** 2)))
# Per-spaxel parameters are what a 13x13-pixel seeing leaves of them: neighbours trade
# flux, so single spaxels scatter far more than the convolved model does.
bright = truth[..., 0] > 3.0
print("bright spaxels (%d): median |centre - truth| = %.2f channels, |width - truth| = %.2f channels" % (
    bright.sum(), np.median(np.abs(post[..., 1] - truth[..., 1])[bright]),
    np.median(np.abs(post[..., 2] - truth[..., 2])[bright])))
# What IS determined is a set of spaxels: every ring's summed flux, flux-weighted centre and width per
# sample (run.posterior.regions, summed on the device in a fixed order) and their scatter over the samples.
rings = run.posterior.regions
ring_of = regions.annuli((H, W), (H / 2., W / 2.), [0., 4., 8., 12., 16.])
F_true = truth[..., 0] * truth[..., 2] * np.sqrt(2. * np.pi)
for k, label in enumerate(rings.ids):
    inside = ring_of == label
    print("ring %d (%4d spaxels): flux %9.2f +- %.2f (truth %9.2f), centre %.3f +- %.3f, width %.3f +- %.3f channels" % (
        label, rings.sizes[k], rings.flux_mean[k], rings.flux_std[k], F_true[inside].sum(),
        rings.centre_mean[k], rings.centre_std[k], rings.width_mean[k], rings.width_std[k]))


# ---- cosmic rays: robust=nu ------------------------------------------------------------------------
# +50 sigma on one voxel in a thousand.  robust=4 gives every voxel a Student-t error: the device redraws
# a weight per voxel between sweeps, and run.robust.weight_mean says which voxels the run stopped believing.
hits = rng.random(clean.shape) < 1e-3
hit_cube = inst.build_cube(cube.data + 50. * sigma * hits)
r = Run(hit_cube, inst, variance=np.full(clean.shape, sigma ** 2), max_iterations=min(iterations, 500),
        min_acceptance_rate=0., gibbs_apriori_variance=100., seed=1, robust=4)
print("robust=4: %d of %d hit voxels have a mean weight below 0.5 (and %d of the %d others)" % (
    r.robust.downweighted()[hits].sum(), hits.sum(), r.robust.downweighted()[~hits].sum(), (~hits).sum()))


# ---- per-spaxel jump scales: adapt_sweeps=N ----------------------------------------------------
# One jump amplitude for every spaxel is too wide for the bright ones and too narrow for the faint
# ones.  adapt_sweeps=N adapts a scale per spaxel on the device during the first N sweeps and freezes
# it; run.acceptance_map is the accepted share of the sweeps after the freeze.  With the scale range
# pinned at (1, 1) nothing adapts: the chain of a run without the keyword, counted alike.
short = dict(variance=np.full(clean.shape, sigma ** 2), max_iterations=min(iterations, 1000), keep_one_in=10,
             min_acceptance_rate=0., gibbs_apriori_variance=100., seed=1,
             adapt_sweeps=min(iterations, 1000) // 2, adapt_window=min(50, min(iterations, 1000) // 2))
for label, more in (("adapted", {}), ("one amplitude", dict(adapt_scale_range=(1., 1.)))):
    r = Run(cube, inst, **dict(short, **more))
    rate = r.acceptance_map[r.mask == 1]
    print("acceptance rate per spaxel after sweep %d, %s: 5th / 50th / 95th percentile %s "
          "(jump scales %s)" % (r.adapted_until, label, np.round(np.percentile(rate, [5, 50, 95]), 3),
                                np.round(np.percentile(r.jump_scale, [5, 50, 95]), 3)))


# ---- matched-filter line search: S/N map, mask and starting map --------------------------------
# A uniform start (the reference's, lib/run.py:310-314) leaves a spaxel tens of channels from its
# line.  line_search correlates every spectrum with the LSF-convolved line over a grid of centres and
# widths on the device; Run(initial_search=True) starts chain 0 from that map.
from deconv3d_amd import above_snr, line_search  # noqa: E402

var = np.full(clean.shape, sigma ** 2)
found = line_search(cube, inst, variance=var)
strong = found.snr >= 5.
print("line search: %d of %d spaxels at S/N >= 5 (above_snr agrees: %s); their centres lie within %.2f channels "
      "of the truth (median)" % (strong.sum(), H * W, bool(np.array_equal(above_snr(cube, inst, 5., variance=var), found.mask(5.))),
                                 np.median(np.abs(found.parameters[..., 1] - truth[..., 1])[strong])))
few = dict(variance=var, max_iterations=min(iterations, 200), min_acceptance_rate=0., gibbs_apriori_variance=100., seed=1)
for label, more in (("searched start", dict(initial_search=True)), ("uniform start", {})):
    r = Run(cube, inst, **dict(few, **more))
    print("%s: reduced chi2 of the last sample after %d sweeps %.3f" % (
        label, few["max_iterations"], np.mean(((cube.data - r.simulate_convolved(cube.data.shape, r.chain[-1])) / sigma) ** 2)))


# ---- a raw cube: continuum removal and channel noise --------------------------------------------
# An archive cube has stellar continuum under the line and a noise that changes with the channel
# (sky lines).  prepare_cube takes the running median of every spectrum as the continuum and
# 1.4826 MAD of every channel of the residual as its noise, both on the device; Run(prepare=True)
# and line_search(prepare=True) do it first and use the prepared cube and its variance.
from deconv3d_amd import prepare_cube  # noqa: E402

true_sigma = sigma * (1. + 2. * rng.random(D))                     # channel-dependent noise
continuum = (20. * sigma * rng.random((H, W))[None]
             + (rng.random((H, W))[None] - 0.5) * 0.5 * sigma * np.arange(float(D))[:, None, None])
raw = inst.build_cube(clean + rng.normal(0., 1., clean.shape) * true_sigma[:, None, None] + continuum)
sky = r2 > (H / 3.) ** 2
prep = prepare_cube(raw, continuum_window=31, reject=3.0, noise_mask=sky)
print("prepared cube: per-channel sigma / truth, median %.3f; continuum error %.2f sigma rms" % (
    np.median(prep.sigma / true_sigma),
    np.sqrt(np.mean(((prep.continuum - continuum) / true_sigma[:, None, None]) ** 2))))
for label, kw in (("raw cube, true variance", dict(variance=np.ones(clean.shape) * (true_sigma ** 2)[:, None, None])),
                  ("prepared", dict(prepare=dict(continuum_window=31, noise_mask=sky)))):
    f = line_search(raw, inst, **kw)
    ok = f.snr >= 5.
    print("line search on the %s: %d spaxels at S/N >= 5, %d of them within one channel of the truth" % (
        label, ok.sum(), (np.abs(f.parameters[..., 1] - truth[..., 1])[ok] <= 1.).sum()))
r = Run(raw, inst, prepare=dict(continuum_window=31, noise_mask=sky), initial_search=True, **{
    k: v for k, v in few.items() if k != "variance"})
print("Run(prepare=...): %d channels with a noise estimate; reduced chi2 of the last sample against the prepared "
      "cube %.3f" % (np.isfinite(r.prepared.sigma).sum(),
                     np.mean((r.cube.data - r.simulate_convolved(r.cube.data.shape, r.chain[-1])) ** 2 / r.variance_cube)))


# ---- several chains at once: chains=R ----------------------------------------------------------
# The reference's own science fixture (tests/input/data14forAntoine.mat: 24 x 30 spaxels x 21
# channels, settings of its tests/read_mat.py:94-121).  A colour launch of so small a cube holds
# two or three windows -- a single chain is a chain of launch latencies -- so R independent chains
# (seeds seed + r) advance TOGETHER, one launch per colour class for all of them, in about the
# time of one; run.chains[r] is bit for bit the chain of Run(..., seed=seed + r), the posterior
# means pool the chains and run.rhat says whether they agree.
from deconv3d_amd import above_percentile  # noqa: E402

chains = int(sys.argv[2]) if len(sys.argv) > 2 else 8
fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                       "ref_mat_fixture.npz")
g = np.load(fixture)
inst2 = MUSE(fsf_fwhm=0.8841, lsf_fwhm=0.)
cube2 = inst2.build_cube(g["data"])
kw = dict(variance=g["var"], gibbs_apriori_variance=5., mask=above_percentile(cube2, 60),
          max_iterations=min(iterations, 4000), keep_one_in=10, seed=7, min_acceptance_rate=0.)
one = Run(cube2, inst2, **kw)
many = Run(cube2, inst2, chains=chains, **kw)
live = many.mask == 1
print("reference fixture %s: 1 chain %.2f s of sweeps, %d chains %.2f s (%.1fx the samples per second); "
      "chain 0 identical: %s; R-hat of the live spaxels' (a, c, w): median %s, 95th percentile %s" % (
          "x".join(str(v) for v in g["data"].shape), one.mh_seconds, chains, many.mh_seconds,
          chains * one.mh_seconds / many.mh_seconds, bool(np.array_equal(one.chain, many.chains[0])),
          np.round(np.nanmedian(many.rhat[live], axis=0), 3), np.round(np.nanpercentile(many.rhat[live], 95, axis=0), 3)))
