# coding=utf-8
"""
``Run`` -- the MCMC deconvolution runner, drop-in for the reference's
``lib/run.py`` class ``Run`` (constructor kwargs :95-109, result attributes
:540-549, helper methods :553-708, 742-840).

The host control flow (validation, setup, stopping rule, chain bookkeeping) is
restated here; everything inside the reference's per-spaxel loop
(lib/run.py:367-519) and the forward models (:597-708, 999-1031) runs on the
GPU through ``libdeconv3d_hip.so``.  There is no CPU fallback.

Differences from the reference, all deliberate:
  * additive kwargs ``seed=`` (the reference is unseeded), ``device=``,
    ``refresh_every=`` (the reference hard-codes 1000, lib/run.py:525);
  * spaxels are scanned colour by colour ((y mod fh, x mod fw) classes, whose
    FSF windows are disjoint) instead of row-major -- the reference declares
    the scan order overridable (lib/run.py:553-560);
  * the (H,W,D,H,W) ``contributions`` array (lib/run.py:285-288) is never
    built: a spaxel's old contribution is recomputed from its parameters;
  * chain / likelihoods are NaN-initialised instead of uninitialised memory;
  * the user's mask is copied, not mutated; zero variances become 1e12 for
    ndarray input too; NaN voxels get zero weight in the Gibbs sums as well;
  * 1-D ``initial_parameters`` are broadcast as the docstring promises;
  * ``SingleGaussianLineModel`` and ``GaussianMultipletLineModel`` (and
    subclasses that only change names/bounds) are evaluated on the device; any
    other ``LineModel`` plugin is evaluated on
    the host per colour class (host_model.py) with the same device kernels for
    everything else -- correct, but python-speed.
"""
from __future__ import annotations

import logging
import math
import time
from collections import namedtuple
from os.path import splitext

import numpy as np

from . import _lib, adapt as _adapt, ensemble, noise as _noise, posterior as _posterior, prepare as _prepare, \
    regions as _regions, \
    predictive as _predictive, prior as _prior, robust as _robust, search as _search, tempering as _tempering
from .cube import Cube, read_fits
from .host_model import HostModelChain
from .instruments import Instrument
from .line_models import (LineModel, SingleGaussianLineModel, SINGLE_LINE_SHAPE,
                          device_line_shape, device_line_table, model_is_on_device)
from .math_utils import median_clip

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger('deconv3d')

CIRCLE_4TH = np.pi / 2.

# adapt.check_keywords' tuple, by name
_AdaptKeywords = namedtuple("_AdaptKeywords", "sweeps window target gain scale_range")


class _Acceptance:
    """The accepted proposals the stopping rule counts (lib/run.py:344-359), of the WHOLE chain:
    ``state`` is the ``resume_state=`` of an earlier segment, whose totals are the base this
    segment's counts add to.  Iteration 1 of a segment counts as accepted; that of a resumed
    segment is the resumed state itself, already counted in the state's totals."""

    def __init__(self, spaxels_count, n_chains, state=None):
        self.spaxels_count, self.n_chains = spaxels_count, n_chains
        self.accepted_count = spaxels_count * n_chains  # first iteration counts as accepted
        self.per_chain_accepted = [spaxels_count] * n_chains
        self._acc_base, self._it_base, self._acc_base_chain = 0, 0, [0] * n_chains
        if state is None:
            return
        files = getattr(state, "files", state)
        # totals over every earlier segment (older checkpoints hold one segment's)
        accepted = int(state["total_accepted"] if "total_accepted" in files else state["accepted_count"])
        iterations = int(state["total_iterations"] if "total_iterations" in files else state["iteration"])
        # (per chain: what the checkpoint recorded, else an even share of the total)
        if n_chains > 1 and "per_chain_accepted" in files:
            per_chain = [int(v) for v in state["per_chain_accepted"]]
        else:
            per_chain = [accepted // n_chains] * n_chains
        self._acc_base = accepted - spaxels_count * n_chains
        self._it_base = iterations - 1
        self._acc_base_chain = [a - spaxels_count for a in per_chain]

    def add(self, per_chain_acc):
        """The accepted counts, one per chain, of the sweeps a call made."""
        self.accepted_count += sum(per_chain_acc)
        self.per_chain_accepted = [a + b for a, b in zip(self.per_chain_accepted, per_chain_acc)]

    def running_rate(self, iteration):
        """The rate the stopping rule sees before the sweep after ``iteration`` (0 while nothing
        can be accepted: no unmasked spaxel)."""
        max_accepted_count = self.spaxels_count * self.n_chains * (iteration + self._it_base)
        if max_accepted_count > 0:
            return float(self.accepted_count + self._acc_base) / float(max_accepted_count)
        return 0.

    def final_rates(self, iteration):
        """``(pooled, [per chain])`` of a run that stopped at ``iteration``."""
        pooled = float(self.accepted_count + self._acc_base) / \
            float(max(self.spaxels_count * self.n_chains * (iteration + self._it_base), 1))
        if self.n_chains == 1:
            return pooled, [pooled]
        return pooled, [(a + b) / float(max(self.spaxels_count * (iteration + self._it_base), 1))
                        for a, b in zip(self.per_chain_accepted, self._acc_base_chain)]

    def state_record(self, iteration):
        """The entries of a checkpoint's state that a later segment is built from."""
        record = dict(accepted_count=self.accepted_count,
                      total_accepted=self.accepted_count + self._acc_base,
                      total_iterations=iteration + self._it_base)
        if self.n_chains > 1:
            record["per_chain_accepted"] = np.array(
                [a + b for a, b in zip(self.per_chain_accepted, self._acc_base_chain)], dtype=np.int64)
        return record


class Run:
    """
    Main runner of the deconvolution::

        cube = Cube.from_fits('my_fits.fits')
        inst = MUSE()
        run = Run(cube, inst, max_iterations=10000)
        run.plot_chain()

    Arguments are those of the reference (lib/run.py:51-109): ``cube``
    (FITS path or Cube), ``instrument``, ``mask``, ``variance``, ``model``,
    ``initial_parameters``, ``jump_amplitude``, ``gibbs_apriori_variance``,
    ``max_iterations``, ``keep_one_in``, ``write_every``,
    ``min_acceptance_rate``; plus ``seed``, ``device``, ``refresh_every``,
    ``sweeps_per_call``, ``checkpoint`` (file prefix written every
    ``write_every`` iterations) and ``resume_state`` (the ``<prefix>_state.npz``
    of a checkpoint: the sweep numbering -- hence the random-number streams -- and the
    accepted count of the stopping rule continue where the checkpointed run stopped; pass the
    checkpoint's ``<prefix>_parameters.npy`` as ``initial_parameters``), and
    ``chain_file`` (file prefix: chain and likelihoods live in memory-mapped
    ``<prefix>_chain.npy`` / ``<prefix>_likelihoods.npy`` instead of RAM, written as the
    device streams saved sweeps out -- a 300x300 chain of 50 000 sweeps is 108 GB), and
    ``chains`` (R >= 2 independent chains of the same cube, seeds ``seed + r``, advanced
    TOGETHER: a cube whose colour launches leave the chip idle -- the reference's own fixtures
    are 24x30x21 -- runs R chains in about the time of one, see `chains` below).

    With ``chains=R``: ``run.chains[r]`` / ``run.all_likelihoods[r]`` are chain r's arrays
    (``run.chain`` / ``run.likelihoods`` are chain 0's; chain r is bit for bit the chain of
    ``Run(..., seed=seed + r)``), ``extract_parameters`` pools the chains, ``run.rhat`` is the
    per-parameter Gelman-Rubin map, ``run.acceptance_rates`` the per-chain rates; the stopping
    rule looks at the pooled acceptance rate.  ``initial_parameters`` may be 4-D, one map per
    chain; a checkpoint holds all R chains (``<prefix>_parameters.npy`` is that 4-D array, chain
    r > 0's slots are ``<prefix>_c<r>_chain.npy``) and resumes R chains.  A custom
    (host-evaluated) line model advances its R chains one after the other.

    ``posterior_burn_in=B`` (default ``None``: off, nothing allocated or launched) keeps, on the
    device, running means and standard deviations of the SAMPLES' clean cube, convolved cube,
    parameters and integrated flux: every chain accumulates its state after the sweeps
    ``B, B + posterior_every, ...`` (with ``keep_one_in = 1`` exactly ``run.chain[B::every]``)
    without a cube crossing to the host.  ``run.posterior`` is a
    :class:`deconv3d_amd.posterior.PosteriorMoments` (``count``, ``clean_mean``, ``clean_std``,
    ``convolved_mean``, ``convolved_std``, ``parameters_mean``, ``parameters_std``, ``flux_mean``,
    ``flux_std``, ``clean_cube()``, ``convolved_cube()``, ``save(prefix)``), downloaded on first
    access; with ``chains=R`` it pools the chains and ``run.posteriors[r]`` is chain r's.  Where
    the FSF leaves single spaxels unidentified, ``posterior.convolved_mean`` fits the data
    while the cube of the mean map (``run.convolved_cube``, the reference's estimator, unchanged)
    does not.  A run that stops before sweep B has ``count == 0`` and NaN
    arrays.  A host-evaluated line model raises ``NotImplementedError``.  The accumulators are
    not part of a checkpoint: a ``resume_state=`` run starts fresh ones, scheduled in this
    segment's sweep numbering.  Costs four more cubes of device memory per chain.

    ``posterior_histograms=True`` (or ``dict(pilot=200, span=6.0)``; default ``None``: off, nothing
    allocated or launched, the chain is bit for bit what it is without the keyword; needs
    ``posterior_burn_in``) keeps, on the device, a 64-bin histogram of every unmasked spaxel's
    ``a``, ``c``, ``w`` and ``F`` beside the moments: the first ``pilot`` accumulated samples
    freeze each range at their mean +- ``span`` standard deviations, clipped to the model's
    bounds, and every later accumulated sample is binned, whatever ``keep_one_in`` is.
    ``run.posterior.histograms`` is a :class:`deconv3d_amd.posterior.PosteriorHistograms`
    (``count``, ``median``, ``interval(0.68)``, ``quantiles(qs)``, ``mode``, ``outside``,
    ``counts``, ``tails``, ``range``, ``save(prefix)``) whose maps are extracted on the device;
    ``outside`` is the share of the samples beyond the frozen range, where a mode the pilot never
    visited ends up.  With ``chains=R`` every chain keeps its own,
    ``run.posteriors[r].histograms``, and the pooled ``run.posterior.histograms`` is ``None``
    (the chains' ranges differ).  A run that cannot accumulate more than ``pilot`` samples logs a
    warning.  Not part of a checkpoint, like the moments.  Costs 1120 bytes per spaxel and chain.

    ``regions=`` (default ``None``: off, nothing allocated or launched, the chain is bit for bit
    what it is without the keyword; needs ``posterior_burn_in``) follows SETS of spaxels: an (H, W)
    integer label map (0: no region, any positive value names one;
    :func:`deconv3d_amd.regions.blocks` and :func:`deconv3d_amd.regions.annuli` build some) or
    ``dict(labels=, spectra=True)``.  For every accumulated sample the device sums, in a fixed
    order, each region's flux ``F = sum F_i``, flux-weighted centre ``C = sum F_i c_i / F`` and
    width ``S = sqrt(sum F_i (w_i^2 + (c_i - C)^2) / F)`` over its unmasked spaxels into a series,
    and (``spectra``) folds the region's summed clean spectrum into a mean and a standard deviation
    (d3d_region_*).  ``run.posterior.regions`` is a :class:`deconv3d_amd.regions.RegionPosterior`
    (``ids``, ``sizes``, ``count``, the series ``flux`` / ``centre`` / ``width`` (n, K), their
    ``*_mean`` / ``*_std``, ``quantiles(qs)``, ``flux_covariance()``, ``spectrum_mean``,
    ``spectrum_std``, ``save(prefix)``); ``run.posterior.save`` writes it too.  With ``chains=R``
    every chain keeps its own, ``run.posteriors[r].regions``, and the pooled one concatenates the
    series chain by chain and pools the spectra; ``tempering=`` follows rung 0 only.  A
    host-evaluated line model raises ``NotImplementedError``.  Not part of a checkpoint, like the
    moments.  Costs ``24 K`` bytes per accumulated sample and chain.

    ``adapt_sweeps=N`` (default ``None``: off, nothing allocated or launched, the chain is bit for
    bit what it is without the keyword) gives every spaxel its own multiplicative jump scale: the
    reference proposes all of them with the one ``jump_amplitude`` (lib/run.py:251-262, 570-579),
    too wide for a bright spaxel and too narrow for a faint one.  Every ``adapt_window`` sweeps of
    the first N each scale s moves, on the device, by
    ``s <- clip(s * exp(adapt_gain / sqrt(k) * (rate - adapt_target)), *adapt_scale_range)``, rate
    the spaxel's accepted share of the window and k the step's number; after the last full window
    at or before sweep N (``run.adapted_until``) the scales are frozen and the rest is an ordinary
    Markov chain.  ``run.jump_scale`` (H, W) holds the frozen scales, ``run.acceptance_map`` (H, W)
    the accepted share of the sweeps after the freeze (NaN where masked, or when none followed);
    with ``chains=R`` every chain adapts from its own counters, ``run.jump_scales[r]`` /
    ``run.acceptance_maps[r]``.  ``posterior_burn_in`` must not lie before N; N beyond 80 % of
    ``max_iterations`` logs a warning (``extract_parameters`` averages the last 20 %).  A
    checkpoint records the maps, and ``resume_state=`` continues them bit for bit (a state
    written with other ``adapt_*`` keywords is refused).  A host-evaluated line model raises
    ``NotImplementedError``.

    ``smoothness=`` (default ``None``: off, nothing allocated or launched, the chain is bit for bit
    what it is without the keyword) adds a pairwise Gaussian prior between 4-neighbours to the
    reference's flat one (lib/run.py:426-438, 491-496), ``-1/2 sum_<i,j> sum_k (theta_i,k -
    theta_j,k)^2 / sigma_k^2`` over the adjacent pairs of unmasked spaxels: a dict with any of
    ``a``, ``c``, ``w``, or a 3-sequence, of sigmas -- the expected difference between neighbouring
    spaxels in the parameter's own unit; ``None`` or ``inf``: none.  ``run.smoothness`` holds the
    three sigmas, ``run.roughness(parameters=None)`` the sums of squared neighbour differences
    ``(E_a, E_c, E_w, pairs)`` of a map.  With ``chains=R`` every chain has the same prior and its
    own parameters.  The checkpoint records the sigmas; ``resume_state=`` refuses a state written
    with others.  A host-evaluated line model raises ``NotImplementedError``, an FSF one spaxel
    wide ``ValueError`` (adjacent spaxels would share a colour class of the sweep).

    ``initial_search=True`` (or a dict of :func:`deconv3d_amd.search.line_search` keywords
    ``centres`` / ``widths`` plus ``jitter``; default ``None``: off, nothing allocated or launched,
    the chain is bit for bit what it is without the keyword) starts the chain from a matched-filter
    search of the cube instead of the reference's uniform draw (lib/run.py:310-314): chain 0 from
    the searched ``(a, c, w)`` map, chains r > 0 from copies whose ``(c, w)`` are jittered by the
    generator of ``seed + r`` (Gaussian, ``jitter = (0.5 channel, 10 %)``, clipped to the bounds) so
    that R-hat still sees dispersed starts; spaxels without a detection keep their uniform draw.
    ``run.search`` is the :class:`deconv3d_amd.search.LineSearch` (``snr``, ``parameters``,
    ``mask(threshold)``).  Refused with ``initial_parameters=`` or ``resume_state=``.

    ``prepare=True`` (or a dict of :func:`deconv3d_amd.prepare.prepare_cube` keywords
    ``continuum_window`` / ``reject`` / ``noise_mask`` / ``rescale``; default ``None``: off, nothing
    allocated or launched, the chain is bit for bit what it is without the keyword) runs
    ``prepare_cube`` on the raw cube first: the run then fits the continuum-free cube
    (``run.cube``) and, when ``variance=`` is None, uses the per-channel variance estimated from
    it instead of the one constant of lib/run.py:171-178; with ``rescale=True`` the given variance
    is rescaled channel by channel instead.  ``run.prepared`` is the
    :class:`deconv3d_amd.prepare.Prepared` (``continuum``, ``sigma``, ...).  ``initial_search=``
    sees the prepared cube.  The checkpoint records the settings; ``resume_state=`` runs the
    preparation again and refuses a state written with other settings.

    ``tempering=`` (default ``None``: off, nothing allocated or launched, the chain is bit for bit
    what it is without the keyword) runs parallel tempering: a dict with either ``betas=(1, ...)``
    (strictly decreasing inverse temperatures) or ``rungs=R`` plus ``beta_min=`` (the geometric
    ladder ``beta_min ** (r / (R - 1))``), and ``swap_every=1``.  Rung r is a chain of the same
    cube with the variance divided by ``betas[r]`` -- its MH ratio (lib/run.py:426-438) and the
    likelihood terms of its Gibbs draw (lib/run.py:491-496) scale by ``betas[r]``, the priors stay
    as they are -- seeded ``seed + r`` and started as chain r of ``chains=R`` is; after every
    sweep s with ``(s + sweep_origin) % swap_every == 0`` adjacent rungs exchange their states on
    the device with the Metropolis rule of replica exchange (d3d_temper_swap), so that the cold
    chain inherits the barrier crossings of the hot ones.  ``run.chain``, ``run.likelihoods``,
    ``run.parameters`` and the cubes come from rung 0 alone; ``run.chains[r]`` holds rung r's
    tempered samples, ``run.rhat`` is ``None`` (the rungs sample different distributions), and
    ``run.tempering`` is a :class:`deconv3d_amd.tempering.TemperingReport` (``betas``,
    ``swap_attempts``, ``swap_accepts``, ``swap_rates``, ``energy_mean``, ``energy_std``,
    ``labels``, ``rounds``, ``save(prefix)``).  ``adapt_sweeps`` and ``smoothness`` apply to every
    rung, ``posterior_burn_in`` / ``posterior_histograms`` to rung 0 only; the acceptance rate of
    the stopping rule is pooled over the rungs.  ``chains`` must be 1 (the rungs take the chains'
    place), a host-evaluated line model raises ``NotImplementedError``.  The checkpoint holds the
    R maps as for ``chains=R`` and records the ladder and ``swap_every``; ``resume_state=`` refuses
    a state written with others, the round numbering continues, counters and labels start afresh.
    ``patch=p`` in the dict (default ``None``: whole cubes) makes a round trade PATCHES instead:
    the unmasked spaxels of tiles of p x p spaxels, cut from an origin drawn per round, each
    decided by itself from an energy difference that lives in the tile dilated by the FSF
    (d3d_temper_set_patch), so that a coarse ladder swaps where whole cubes never would.  The
    report then counts ``patch_attempts`` / ``patch_accepts`` / ``patch_rates`` per pair, its
    ``labels`` is ``None``, and ``resume_state=`` refuses a state written with another patch size.

    ``robust=4`` (or ``dict(nu=4, every=1, start=0)``; default ``None``: off, nothing allocated or
    launched, the chain is bit for bit what it is without the keyword) replaces the reference's
    Gaussian error of known variance (lib/run.py:171-192, 407-426) by a Student-t error with ``nu``
    degrees of freedom (an integer from 1 to 30), so that single voxels tens of sigma off -- cosmic
    rays, sky-line residuals, bad columns -- stop pulling on every spaxel whose FSF window holds
    them.  Every voxel carries a latent weight: after each sweep s >= ``start`` with
    ``(s - start) % every == 0`` (the whole run's numbering) the device redraws the weights from
    ``Gamma((nu + 1)/2, rate (nu + r^2 / variance)/2)``, r the voxel's residual, and the sweeps run
    on ``variance / weight`` -- an exact Gibbs step (d3d_robust_*).  ``run.robust`` is a
    :class:`deconv3d_amd.robust.RobustReport` (``nu``, ``every``, ``start``, ``count``,
    ``weight_mean`` (D, H, W), ``weights``, ``downweighted(threshold)``, ``save(prefix)``); the mean
    takes the draws from ``posterior_burn_in`` on when that is given, else from ``start``.  With
    ``chains=R`` every chain draws its own, ``run.robusts[r]``, and ``run.robust`` pools the means by
    count.  ``run.likelihoods``, ``d3d_chi2_map`` and the window probe of such a run are those of the
    conditional Gaussian under the current weights.  ``initial_search=`` and ``prepare=`` run before
    the weights are armed and see the given variance.  Refused with ``tempering=`` (a rung's
    ``variance / beta`` is not a tempered Student-t); a host-evaluated line model raises
    ``NotImplementedError``.  The checkpoint records ``nu``, ``every`` and ``start``;
    ``resume_state=`` refuses a state written with others and re-makes the last due draw at or
    before the checkpointed sweep from the restored state; the weight mean starts afresh.  Costs
    two more cubes of device memory per chain.

    ``noise=True`` (or ``dict(per='channel'|'cube'|<D integer labels>, every=1, start=0, shape=0.,
    rate=0., spaxels='all'|'unmasked'|<(H, W) 0/1 map>)``; default ``None``: off, nothing allocated or
    launched, the chain is bit for bit what it is without the keyword) stops taking the variance as
    known (lib/run.py:171-200, 407-426): the variance of every voxel of a group ``g`` of channels is
    ``s_g`` times the given one, ``s_g ~ InvGamma(shape, rate)`` (0, 0: Jeffreys' ``1/s``), and after
    every sweep ``s >= start`` with ``(s - start) % every == 0`` (the whole run's numbering) the device
    redraws ``1/s_g ~ Gamma(shape + N_g/2, rate rate + Q_g/2)`` from the residual -- an exact Gibbs
    step (d3d_noise_*) -- and the sweeps run on the rescaled variance.  ``per`` names the groups
    (label -1: the channel is never rescaled), ``spaxels`` the spaxels whose voxels are counted.
    ``run.noise`` is a :class:`deconv3d_amd.noise.NoiseReport` (``scale`` (n, G), ``sweeps``,
    ``groups``, ``voxels``, ``count``; ``scale_mean``, ``scale_std``, ``quantiles(q)`` over the draws
    from ``posterior_burn_in`` on, or all; ``channel_scale`` (D,); ``variance(given)``;
    ``save(prefix)``).  With ``chains=R`` every chain draws its own, ``run.noises[r]``, and
    ``run.noise`` concatenates the series.  ``run.likelihoods`` and the chi2 map of such a run are those
    of the conditional Gaussian under the current scales.  ``initial_search=`` and ``prepare=`` run
    before arming, on the given variance.  A checkpoint records the keywords, ``resume_state=`` refuses
    a state written with others, and a resumed run re-makes the last due draw and starts a fresh
    series.  Refused: ``robust=`` and ``predictive=`` (their device code reads the base variance),
    ``tempering=``, host-evaluated line models.

    ``predictive=True`` (or ``dict()``, for future keys; default ``None``: off, nothing allocated or
    launched; needs ``posterior_burn_in``) keeps, on the device, the pointwise predictive density of
    every voxel over the samples of the posterior moments: ``lppd_v = log mean_s p(y_v | theta_s)``
    and the WAIC penalty ``p_v = var_s log p(y_v | theta_s)`` (d3d_pred_*), under the run's own
    likelihood -- Gaussian, or with ``robust=`` the Student-t marginal on the given variance.
    ``run.posterior.predictive`` is a :class:`deconv3d_amd.predictive.PredictiveAccuracy`
    (``count``; ``lppd_map``, ``p_waic_map``, ``elpd_map``, ``voxels``; ``lppd``, ``p_waic``,
    ``elpd``, ``waic``, ``se``; ``lppd_cube``, ``p_waic_cube``; ``compare(other)`` -> ``(delta_elpd,
    se_delta)``; ``save(prefix)``), ``None`` without the keyword.  The chain is bit for bit the chain
    without the keyword.  With ``chains=R`` every chain keeps its own,
    ``run.posteriors[r].predictive``, and the pooled one merges their accumulators exactly;
    ``tempering=`` follows rung 0.  Not part of a checkpoint: a resumed run starts afresh.  A
    host-evaluated line model raises ``NotImplementedError``.  Costs four more cubes of device
    memory per chain.
    """

    def __init__(
        self,
        cube,
        instrument=None,
        mask=None,
        variance=None,
        model=SingleGaussianLineModel,
        initial_parameters=None,
        jump_amplitude=0.1,
        gibbs_apriori_variance=None,
        max_iterations=100000,
        keep_one_in=1,
        write_every=10000,
        min_acceptance_rate=0.01,
        seed=12345,
        device=0,
        refresh_every=1000,
        sweeps_per_call=None,
        checkpoint=None,
        resume_state=None,
        chain_file=None,
        chains=1,
        posterior_burn_in=None,
        posterior_every=1,
        posterior_histograms=None,
        adapt_sweeps=None,
        adapt_window=50,
        adapt_target=0.25,
        adapt_gain=2.0,
        adapt_scale_range=(1e-3, 1e3),
        initial_search=None,
        prepare=None,
        smoothness=None,
        tempering=None,
        regions=None,
        robust=None,
        predictive=None,
        noise=None,
    ):
        prepare_cfg, search_cfg, posterior_burn_in, posterior_every, hist_cfg = self._check_keywords(
            prepare, initial_search, initial_parameters, resume_state, posterior_burn_in,
            posterior_every, posterior_histograms, adapt_sweeps, adapt_window, adapt_target,
            adapt_gain, adapt_scale_range, smoothness, tempering, keep_one_in, write_every,
            max_iterations, chains, regions, robust, predictive, noise)
        self._read_inputs(cube, prepare_cfg, mask, variance, device)
        self._read_instrument(instrument)
        self._read_model(model, jump_amplitude, gibbs_apriori_variance, seed, posterior_burn_in)
        self._allocate_chains(chain_file)
        start_rngs = self._starting_maps(initial_parameters)
        # a resumed run continues the checkpointed run's sweep numbering: sweep s of
        # this segment draws the random numbers of sweep s + origin
        self.sweep_origin, resumed, resumed_adapt = self._read_checkpoint(resume_state)
        self._acceptance = _Acceptance(int(np.sum(self.mask == 1)), self.n_chains, resumed)
        self._create_engines(device)
        self._searched_start(search_cfg, start_rngs)
        temper_group = self._arm(refresh_every, posterior_burn_in, posterior_every, hist_cfg,
                                 resumed_adapt, resume_state is not None)
        last_swap_round = self._loop(min_acceptance_rate, sweeps_per_call, checkpoint, temper_group)
        self._read_adaptation()
        self._outputs(temper_group, last_swap_round, posterior_burn_in, hist_cfg)

    # THE PHASES OF __init__, IN ITS ORDER ####################################

    def _check_keywords(self, prepare, initial_search, initial_parameters, resume_state,
                        posterior_burn_in, posterior_every, posterior_histograms, adapt_sweeps,
                        adapt_window, adapt_target, adapt_gain, adapt_scale_range, smoothness,
                        tempering, keep_one_in, write_every, max_iterations, chains, regions, robust=None,
                        predictive=None, noise=None):
        """The keywords' own checks.  Returns the checked ``prepare=`` and ``initial_search=``,
        the posterior schedule and the checked ``posterior_histograms=``."""
        # (before anything else: no device work yet)
        prepare_cfg = _prepare.check_keywords(prepare)
        search_cfg = _search.check_keywords(initial_search, initial_parameters, resume_state)
        if posterior_burn_in is not None:     # (before anything else: no device work yet)
            posterior_burn_in, posterior_every = _posterior.check_schedule(posterior_burn_in,
                                                                           posterior_every)
        hist_cfg = _posterior.check_histograms(posterior_histograms, posterior_burn_in)
        # (the map's shape is checked against the cube's in _read_inputs)
        self._regions_cfg = _regions.check_regions(regions, None, posterior_burn_in)
        self._predictive_cfg = _predictive.check_keyword(predictive, posterior_burn_in)
        adapt_cfg = None
        if adapt_sweeps is not None:
            adapt_cfg = _AdaptKeywords(*_adapt.check_keywords(adapt_sweeps, adapt_window, adapt_target,
                                                              adapt_gain, adapt_scale_range))
            if posterior_burn_in is not None and posterior_burn_in < adapt_cfg.sweeps:
                raise ValueError("posterior_burn_in=%d lies before adapt_sweeps=%d: the moments of a "
                                 "chain that is still adapting are not posterior moments"
                                 % (posterior_burn_in, adapt_cfg.sweeps))
        self._adapt_cfg = adapt_cfg
        self.smoothness = _prior.check_keywords(smoothness)
        temper_cfg = self.tempering_cfg = _tempering.check_keywords(tempering)
        self._robust_cfg = _robust.check_keywords(robust)
        _robust.check_run(self._robust_cfg, temper_cfg)
        # (shapes are checked against the cube's in _read_inputs)
        self._noise_cfg = _noise.check_keywords(noise)
        _noise.check_run(self._noise_cfg, temper_cfg, self._robust_cfg, self._predictive_cfg)
        # lib/run.py:112-114
        assert keep_one_in > 0, "keep_one_in= MUST be a positive integer"
        assert write_every > 0, "write_every= MUST be a positive integer"
        assert max_iterations > 0, "max_iterations= MUST be a positive integer"
        self.logger = logger
        self.keep_one_in = int(keep_one_in)
        self.max_iterations = int(max_iterations)
        self.write_every = int(write_every)
        n_chains = int(chains)
        assert n_chains >= 1, "chains= MUST be a positive integer"
        _tempering.check_run(temper_cfg, n_chains, False, None)
        if temper_cfg is not None:          # (the rungs take the chains' place: rung r is chain r)
            n_chains = len(temper_cfg["betas"])
        self.n_chains = n_chains
        if adapt_cfg is not None and adapt_cfg.sweeps > 0.8 * self.max_iterations:
            logger.warning("adapt_sweeps=%d is beyond 80 %% of max_iterations=%d: extract_parameters "
                           "averages the last 20 %% of the chain, part of which is still adapting"
                           % (adapt_cfg.sweeps, self.max_iterations))
        return prepare_cfg, search_cfg, posterior_burn_in, posterior_every, hist_cfg

    def _read_inputs(self, cube, prepare_cfg, mask, variance, device):
        """``run.cube`` (prepared, with ``prepare=``), ``run.mask``, ``run.variance_cube`` and
        ``run.error_cube``."""
        # ---- input cube (lib/run.py:119-143) --------------------------------
        if isinstance(cube, str):
            cube = Cube.from_fits(cube)
        if not isinstance(cube, Cube):
            raise TypeError("Provided cube is not a HyperspectralCube")
        if cube.is_empty():
            raise ValueError("Provided cube is empty")
        if self._regions_cfg is not None:
            _regions.check_shape(self._regions_cfg["labels"], cube.data.shape[1:])
        # ---- prepare=: the continuum-free cube and its per-channel variance take the place of
        # the raw cube and of a variance that was not given (or, rescale=True, of the given one)
        self.prepared = None
        if prepare_cfg is not None:
            given = variance if prepare_cfg["rescale"] else None
            if prepare_cfg["rescale"] and variance is None:
                raise ValueError("prepare=dict(rescale=True) needs the variance= cube it rescales")
            self.prepared = _prepare.prepare_cube(
                cube, prepare_cfg["continuum_window"], prepare_cfg["reject"], prepare_cfg["noise_mask"],
                variance=given, rescale=prepare_cfg["rescale"], device=device)
            cube = self.prepared.cube
            if variance is None or prepare_cfg["rescale"]:
                variance = self.prepared.variance
        self.cube = cube
        signal_max = np.nanmax(self.cube.data)
        assert signal_max > 1e-10, \
            "The input cube has data that is too small and will cause " \
            "numerical instability, infinite loops, or worse : bad science."
        cube_shape = cube.data.shape
        cube_depth, cube_height, cube_width = cube_shape

        # ---- mask (lib/run.py:151-165), copied instead of mutated -------------
        if mask is None:
            mask = np.ones((cube_height, cube_width))
        if isinstance(mask, str):
            mask, _ = read_fits(mask)
        mask = np.array(mask, dtype=np.float64)
        if mask.shape != (cube_height, cube_width):
            raise ValueError("Mask MUST have (%d, %d) shape, got %s."
                             % (cube_height, cube_width, str(mask.shape)))
        mask[np.isnan(np.sum(self.cube.data, 0))] = 0
        self.mask = mask
        if self._noise_cfg is not None:      # noise=: the groups and the counted spaxels of this cube
            self._noise_cfg = _noise.resolve(self._noise_cfg, cube_depth, mask)

        # ---- variance (lib/run.py:170-200) ---------------------------------
        if variance is not None:
            if isinstance(variance, str):
                variance = Cube.from_fits(variance)
            if isinstance(variance, Cube):
                if variance.data is None:
                    self.logger.warning("Provided variance cube is empty")
                variance_cube = variance.data
            elif isinstance(variance, np.ndarray):
                variance_cube = variance
            else:
                raise TypeError("Provided variance is not a Cube")
            variance_cube = np.where(variance_cube == 0.0, 1e12, variance_cube)
        else:
            sub_data = np.copy(cube.data[2:-2, 2:-4, 2:4])
            _, clip_sigma, _ = median_clip(sub_data, 2.5)
            if clip_sigma == 0:
                clip_sigma = 1e-20
            variance_cube = np.ones(cube_shape) * clip_sigma ** 2
        if variance_cube.shape != cube_shape:
            raise ValueError("Provided variance has not the correct shape."
                             "Expected %s, got %s" % (str(cube_shape), str(variance_cube.shape)))
        self.variance_cube = variance_cube
        self.error_cube = np.sqrt(self.variance_cube)

    def _read_instrument(self, instrument):
        """Instrument and taps (lib/run.py:202-224): ``run.instrument``, ``run.lsf``, ``run.fsf``."""
        cube_depth = self.cube.data.shape[0]
        if not isinstance(instrument, Instrument):
            raise TypeError("Provided instrument is not an Instrument")
        self.instrument = instrument
        lsf = self.instrument.lsf.as_vector(self.cube)
        self.lsf = None if lsf is None else np.asarray(lsf, dtype=np.float64)
        self.fsf = np.asarray(self.instrument.fsf.as_image(self.cube), dtype=np.float64)
        if self.fsf.ndim != 2 or self.fsf.shape[0] % 2 == 0 or self.fsf.shape[1] % 2 == 0:
            raise ValueError("FSF *must* be of odd dimensions")
        if self.lsf is not None and self.lsf.shape != (cube_depth,):
            raise ValueError("LSF must have the length of the cube's spectral axis (%d), got %s"
                             % (cube_depth, str(self.lsf.shape)))

    def _refuse_host_model(self, what, reason=None):
        """The refusal of a keyword or method that needs a line model the device evaluates."""
        sentence = "%s: the line model %s is evaluated on the host" % (what, type(self.model).__name__)
        raise NotImplementedError(sentence if reason is None else "%s; %s" % (sentence, reason))

    def _read_model(self, model, jump_amplitude, gibbs_apriori_variance, seed, posterior_burn_in):
        """Model (lib/run.py:226-265): ``run.model``, what the device needs of it, its bounds and
        the jump amplitudes; and the keywords a host-evaluated model cannot honour."""
        if isinstance(model, LineModel):
            self.model = model
        else:
            self.model = model()
            if not isinstance(self.model, LineModel):
                raise TypeError("Provided model is not a LineModel")
        # The HIP kernels evaluate SingleGaussianLineModel and GaussianMultipletLineModel
        # themselves (line_models.model_is_on_device: subclasses may change names/bounds but
        # not the curve or the Gibbs index); any other LineModel plugin is evaluated on the
        # host (host_model.HostModelChain): same device kernels for LSF, window statistics,
        # accept, Gibbs draw and residual, but python-speed proposals and modelize() calls.
        self._host_model = not model_is_on_device(self.model)
        # (before posterior_burn_in=, which regions= needs: the refusal names the keyword that asked)
        if self._regions_cfg is not None and self._host_model:
            self._refuse_host_model("regions=", "the device follows regions only for the models it "
                                    "evaluates itself")
        if self._predictive_cfg is not None and self._host_model:
            self._refuse_host_model("predictive=", "the device accumulates the predictive density only "
                                    "between the sweeps it runs itself")
        if posterior_burn_in is not None and self._host_model:
            self._refuse_host_model("posterior_burn_in=", "the device accumulates posterior moments "
                                    "only for the models it evaluates itself")
        _prior.check_fsf(self.smoothness, self.fsf.shape)
        if self.smoothness is not None and self._host_model:
            self._refuse_host_model("smoothness=", "the device knows the prior only for the "
                                    "(a, c, w) of the models it evaluates itself")
        _tempering.check_run(self.tempering_cfg, 1, self._host_model, type(self.model).__name__)
        if self._noise_cfg is not None and self._host_model:
            self._refuse_host_model("noise=", "the device redraws the scales only between the sweeps "
                                    "it runs itself")
        if self._robust_cfg is not None and self._host_model:
            self._refuse_host_model("robust=", "the device redraws the weights only between the sweeps "
                                    "it runs itself")
        if self._adapt_cfg is not None and self._host_model:
            self._refuse_host_model("adapt_sweeps=", "the device adapts jump scales only for the "
                                    "models it evaluates itself")
        # (offsets, ratios) of the device's unit line; None for a host-evaluated model
        self.line_shape = None if self._host_model else device_line_shape(self.model)
        # (table, support, flux_factor) of a tabulated line and the digest a checkpoint records
        self.line_table = None if self._host_model else device_line_table(self.model)
        self.line_table_digest = None if self.line_table is None else self.model.digest()
        min_boundaries = np.array(self.model.min_boundaries(self), dtype=np.float64)
        max_boundaries = np.array(self.model.max_boundaries(self), dtype=np.float64)
        names = self.model.parameters()
        self.logger.info("Min boundaries : %s" % dict(zip(names, min_boundaries)))
        self.logger.info("Max boundaries : %s" % dict(zip(names, max_boundaries)))
        if not (np.isfinite(min_boundaries).all() and np.isfinite(max_boundaries).all()):
            raise ValueError("Boundaries are not finite: min %s, max %s (NaN or infinite data?)"
                             % (min_boundaries, max_boundaries))
        if (min_boundaries > max_boundaries).any():
            raise ValueError("Boundaries are inconsistent: min > max.")
        parameters_count = len(names)
        jumping_amplitude = np.ones(parameters_count) * np.array(jump_amplitude)
        gpi = self.model.gibbs_parameter_index()
        if gpi is not None:                                   # lib/run.py:255-265
            jumping_amplitude[gpi] = 0
            if gibbs_apriori_variance is None:
                gibbs_apriori_variance = float(max_boundaries[gpi] ** 2)
        elif gibbs_apriori_variance is None:
            gibbs_apriori_variance = 1.0
        self.min_boundaries = min_boundaries
        self.max_boundaries = max_boundaries
        self.jumping_amplitude = jumping_amplitude
        self.gibbs_apriori_variance = gibbs_apriori_variance
        self.seed = int(seed)

    def _allocate_chains(self, chain_file):
        """Chain storage (lib/run.py:267-281), NaN instead of garbage: ``run.chains`` and
        ``run.all_likelihoods``, in memory or mapped to ``chain_file``'s."""
        # (one chain array per chain; chain r > 0 of a memory-mapped run lives in <prefix>_c<r>_*)
        cnt_iterations = int(math.ceil(self.max_iterations / float(self.keep_one_in)))
        self._chain_file = chain_file
        self._likelihoods_maps = []
        self.chains, self.all_likelihoods = [], []
        try:
            chain_shape = (cnt_iterations,) + self.mask.shape + (len(self.model.parameters()),)
            for r in range(self.n_chains):
                if chain_file is not None:
                    # pages are created as saved sweeps arrive; slots never written (early
                    # stop) are NaN-filled at the end like the in-memory chain
                    prefix = chain_file if r == 0 else "%s_c%d" % (chain_file, r)
                    ch = np.lib.format.open_memmap(
                        "%s_chain.npy" % prefix, mode="w+", dtype=np.float64, shape=chain_shape)
                    lk = np.lib.format.open_memmap(
                        "%s_likelihoods.npy" % prefix, mode="w+", dtype=np.float64,
                        shape=chain_shape[:3])
                    lk[0] = np.nan
                    self._likelihoods_maps.append(lk)
                else:
                    ch = np.full(chain_shape, np.nan)
                    lk = np.full(chain_shape[:3], np.nan)
                self.chains.append(ch)
                self.all_likelihoods.append(lk)
        except MemoryError:
            self.logger.error("Not enough RAM available for that many iterations. "
                              "Use a higher value in the keep_one_in= parameter.")
            raise
        self.chain = self.chains[0]
        self.likelihoods = self.all_likelihoods[0]

    def _starting_maps(self, initial_parameters):
        """Initial parameters (lib/run.py:293-314), slot 0 of every chain: the given map(s), or
        uniform draws within the bounds.  Returns the generators that drew (one per chain), which
        ``initial_search=`` goes on drawing from."""
        # (chain r draws its start from the generator of seed + r: it is the chain of
        # Run(..., seed=seed + r))
        cube_height, cube_width = self.mask.shape
        parameters_count = self.chain.shape[3]
        n_chains, start_rngs = self.n_chains, []
        if initial_parameters is not None:
            if isinstance(initial_parameters, str):
                initial_parameters = np.load(initial_parameters)
            initial_parameters = np.array(initial_parameters, dtype=np.float64)
            if initial_parameters.ndim == 1:
                if initial_parameters.shape[0] != parameters_count:
                    raise ValueError("1D initial params MUST have %d values, got %d."
                                     % (parameters_count, initial_parameters.shape[0]))
                initial_parameters = np.tile(initial_parameters, (cube_height, cube_width, 1))
            per_chain = initial_parameters.ndim == 4
            if per_chain and initial_parameters.shape[0] != n_chains:
                raise ValueError("4D initial params MUST hold one map per chain (%d), got %d."
                                 % (n_chains, initial_parameters.shape[0]))
            ip_shape = initial_parameters.shape[1:] if per_chain else initial_parameters.shape
            if ip_shape[0] != cube_height or ip_shape[1] != cube_width:
                raise ValueError("Initial params MUST have (%d, %d) shape, got (%d, %d)."
                                 % (cube_height, cube_width, ip_shape[0], ip_shape[1]))
            for r in range(n_chains):
                self.chains[r][0] = initial_parameters[r] if per_chain else initial_parameters
        else:
            for r in range(n_chains):
                start_rngs.append(np.random.default_rng(self.seed + r))
                draws = start_rngs[r].random((cube_height, cube_width, parameters_count))
                self.chains[r][0] = self.min_boundaries + \
                    (self.max_boundaries - self.min_boundaries) * draws
        return start_rngs

    def _create_engines(self, device):
        """Device context: ``run.engines``, one per chain, holding the taps, the data and the line."""
        temper_cfg = self.tempering_cfg
        self.engines = []
        for r in range(self.n_chains):
            eng = _lib.Engine(self.cube.data.shape, self.fsf.shape, device=device)
            self.engines.append(eng)
            eng.set_taps(self.fsf, self.lsf)
            # (tempering=: rung r samples L^beta_r x prior, the same model with the variance / beta_r)
            eng.set_data(self.cube.data, self.variance_cube if temper_cfg is None
                         else self.variance_cube / temper_cfg["betas"][r], mask=self.mask)
            if self.line_shape is not None:
                eng.set_line_shape(*self.line_shape)
            if self.line_table is not None:
                eng.set_line_table(*self.line_table)
        self.engine = self.engines[0]

    def _searched_start(self, search_cfg, start_rngs):
        """Searched start (initial_search=), ``run.search``: chain 0 from the matched-filter map, chains
        r > 0 from jittered copies; spaxels without a detection keep their uniform draw."""
        self.search = None
        if search_cfg is not None:
            self.search = _search.search_engine(self.engine, self.model, self, search_cfg["centres"],
                                                search_cfg["widths"], self.lsf)
            found = self.search.detected & (self.mask == 1)
            for r in range(self.n_chains):
                start = self.search.parameters if r == 0 else _search.jittered_start(
                    self.search.parameters, search_cfg["jitter"], start_rngs[r],
                    self.min_boundaries, self.max_boundaries)
                self.chains[r][0][found] = start[found]

    def _arm(self, refresh_every, posterior_burn_in, posterior_every, hist_cfg, resumed_adapt, resumed):
        """Everything the first sweep needs: the host chains, or the engines' parameters, sampler
        settings, accumulators and residual.  Returns the ``tempering=`` group, or None."""
        n_chains, temper_cfg, adapt_cfg = self.n_chains, self.tempering_cfg, self._adapt_cfg
        if self._host_model:
            self.logger.info("Line model %s is evaluated on the host (slower path)."
                             % type(self.model).__name__)
            # (chains=R: one host chain per engine, seeds seed + r, advanced one after the other)
            self._host_chains = [
                HostModelChain(self, self.engines[r], self.chains[r][0], self.min_boundaries,
                               self.max_boundaries, self.jumping_amplitude,
                               self.gibbs_apriori_variance, self.seed + r, refresh_every)
                for r in range(n_chains)]
            self._host_chain = self._host_chains[0]
        else:
            for r, eng in enumerate(self.engines):
                eng.set_params(self.chains[r][0])
                eng.mh_config(self.min_boundaries, self.max_boundaries, self.jumping_amplitude,
                              self.gibbs_apriori_variance, seed=self.seed + r,
                              refresh_every=refresh_every)
                if posterior_burn_in is not None and (temper_cfg is None or r == 0):
                    eng.post_begin()
                    eng.post_schedule(posterior_burn_in, posterior_every)
                    if hist_cfg is not None:
                        eng.hist_begin(hist_cfg["pilot"], hist_cfg["span"])
                    if self._regions_cfg is not None:
                        eng.region_begin(self._regions_cfg["labels"], len(self._regions_cfg["ids"]),
                                         len(range(posterior_burn_in, self.max_iterations, posterior_every)),
                                         self._regions_cfg["spectra"])
                if adapt_cfg is not None:
                    # (the last adapted sweep in the numbering of the whole run: a resumed
                    # segment counts from its sweep origin)
                    eng.adapt_begin(adapt_cfg.target, adapt_cfg.window, adapt_cfg.sweeps,
                                    adapt_cfg.gain, adapt_cfg.scale_range)
                    if resumed_adapt is not None:
                        eng.adapt_set(*resumed_adapt[r])
                if self.smoothness is not None:
                    eng.prior_begin(_prior.lam_of(self.smoothness))
                if self._robust_cfg is not None:
                    # (the run's numbering; a resumed segment's mean starts with its own sweeps)
                    cfg = self._robust_cfg
                    first = cfg["start"] if posterior_burn_in is None else posterior_burn_in + self.sweep_origin
                    eng.robust_begin(cfg["nu"], cfg["every"], cfg["start"],
                                     max(first, self.sweep_origin + 1) if resumed else first)
                if self._noise_cfg is not None:
                    # (after initial_search= and prepare= have seen the given variance; the run's numbering)
                    cfg = self._noise_cfg
                    eng.noise_begin(cfg["group"], cfg["G"], cfg["map"], cfg["shape"], cfg["rate"], cfg["every"],
                                    cfg["start"], _noise.capacity(cfg, self.max_iterations, self.sweep_origin))
                # (after robust=: the predictive density is the likelihood's in force; rung 0 only)
                if self._predictive_cfg is not None and (temper_cfg is None or r == 0):
                    eng.pred_begin()
        if resumed:
            for chain in self._host_chains if self._host_model else self.engines:
                chain.set_sweep_origin(self.sweep_origin)
        if hist_cfg is not None:
            reachable = len(range(posterior_burn_in, self.max_iterations, posterior_every))
            if reachable <= hist_cfg["pilot"]:
                self.logger.warning("posterior_histograms=: max_iterations=%d leaves %d accumulated sweeps, "
                                    "none beyond the pilot of %d; the histograms will hold no sample"
                                    % (self.max_iterations, reachable, hist_cfg["pilot"]))
            if n_chains > 1 and temper_cfg is None:
                self.logger.info("posterior_histograms=: every chain freezes its own ranges; "
                                 "run.posteriors[r].histograms are per chain and the pooled "
                                 "run.posterior.histograms is None")
        self.logger.info("Iteration #1")
        if not self._host_model:
            for eng in self.engines:
                eng.residual(fetch=False)              # lib/run.py:317-334
            # robust=, resumed: the weights the checkpointed run held were its last due draw
            last = _robust.last_due(self._robust_cfg, self.sweep_origin) \
                if resumed and self._robust_cfg is not None else None
            if last is not None:
                for eng in self.engines:
                    eng.robust_step(last)
            # noise=, resumed: likewise the scales
            last = _noise.last_due(self._noise_cfg, self.sweep_origin) \
                if resumed and self._noise_cfg is not None else None
            if last is not None:
                for eng in self.engines:
                    eng.noise_step(last)
        # tempering=: the group that exchanges the rungs' states on the device.  The round of the
        # exchange after sweep s is (s + sweep_origin) // swap_every: a resumed run continues the
        # numbering, so no uniform is drawn twice.
        if temper_cfg is not None:
            return _lib.TemperGroup(self.engines, temper_cfg["betas"], seed=self.seed,
                                    patch=temper_cfg.get("patch"))
        return None

    def _loop(self, min_acceptance_rate, sweeps_per_call, checkpoint, temper_group):
        """MH within Gibbs loop (lib/run.py:336-537): the sweeps, up to ``max_iterations`` or to where
        the stopping rule ends them, and the checkpoints on the way.  Returns the round of the last
        ``tempering=`` exchange, or None."""
        max_iterations, temper_cfg, acceptance = self.max_iterations, self.tempering_cfg, self._acceptance
        cur_iteration = 1
        cur_acceptance_rate = 0.
        last_swap_round = None
        self.mh_seconds = 0.0                      # wall time of the device calls of the loop
        # the reference re-evaluates the stopping rule (and logs) every sweep
        # (lib/run.py:344-364): one sweep per device call whenever the rule is
        # armed, so that the run stops exactly where the reference would; with
        # min_acceptance_rate <= 0 sweeps are batched up to the next saved one
        if sweeps_per_call is None:
            sweeps_per_call = 1 if min_acceptance_rate > 0 else max(1, min(self.keep_one_in, 64))
        if self._host_model:
            sweeps_per_call = 1
        self.iterations_done = 1
        while cur_iteration < max_iterations and \
                (cur_acceptance_rate > min_acceptance_rate or cur_acceptance_rate == 0.):
            cur_acceptance_rate = acceptance.running_rate(cur_iteration)
            n = min(sweeps_per_call, max_iterations - cur_iteration)
            swap_round = None
            if temper_cfg is not None:      # (a call ends at every sweep an exchange follows)
                n, swap_round = _tempering.calls_until_swap(n, cur_iteration, self.sweep_origin,
                                                            temper_cfg["swap_every"])
            self.logger.info("Iteration #%d / %d, %2.0f%%" %
                             (cur_iteration + 1, max_iterations, 100 * cur_acceptance_rate))
            acceptance.add(self._advance(n, cur_iteration, temper_group, swap_round))
            if swap_round is not None:
                last_swap_round = swap_round
            before = cur_iteration
            cur_iteration += n
            # write_every: documented (lib/run.py:89-92) but never used by the
            # reference; here it is the checkpoint cadence when a path is given
            if checkpoint is not None and \
                    before // self.write_every != cur_iteration // self.write_every:
                self.iterations_done = cur_iteration
                self._write_checkpoint(checkpoint, cur_iteration)
        self.iterations_done = cur_iteration
        self.acceptance_rate, self.acceptance_rates = acceptance.final_rates(cur_iteration)
        if self._chain_file is not None:
            n_valid = self._n_valid(cur_iteration)
            for ch, lk in zip(self.chains, self.all_likelihoods):
                ch[n_valid:] = np.nan
                lk[n_valid:] = np.nan
                ch.flush()
                lk.flush()
        return last_swap_round

    def _advance(self, n, first, temper_group=None, swap_round=None):
        """Sweeps ``first .. first + n - 1`` of every chain, whatever carries them, and then the
        exchange of round ``swap_round`` between the rungs.  Returns the accepted counts, one per
        chain.  ``run.mh_seconds`` takes the wall time of the device calls; the host-evaluated
        chains (one sweep per call) are not timed."""
        if self._host_model:
            save = first % self.keep_one_in == 0
            slot = first // self.keep_one_in
            acc = [hc.sweep(first, self.all_likelihoods[r][slot] if save else None)
                   for r, hc in enumerate(self._host_chains)]
            if save:
                for r, hc in enumerate(self._host_chains):
                    self.chains[r][slot] = hc.params
            return acc
        if self.n_chains == 1:
            t_call = time.perf_counter()
            acc = self.engine.mh_sweeps(n, first, self.keep_one_in, self.chain, self.likelihoods)
            self.mh_seconds += time.perf_counter() - t_call
            return [acc]
        t_call = time.perf_counter()
        acc = self._sweep_chains(n, first, self.all_likelihoods)
        self.mh_seconds += time.perf_counter() - t_call
        if swap_round is not None:     # (the sweep's chain slot is saved: the rungs trade states)
            t_call = time.perf_counter()
            temper_group.swap(swap_round)
            self.mh_seconds += time.perf_counter() - t_call
        return acc

    def _read_adaptation(self):
        """Jump scales and acceptance-rate maps (adapt_sweeps=): ``run.jump_scales``,
        ``run.acceptance_maps`` and ``run.adapted_until``."""
        adapt_cfg = self._adapt_cfg
        self.jump_scales = self.acceptance_maps = None
        self.jump_scale = self.acceptance_map = self.adapted_until = None
        if adapt_cfg is not None:
            self.jump_scales, self.acceptance_maps = [], []
            for eng in self.engines:
                scale, acc, n_win, k = eng.adapt_get()
                with np.errstate(invalid="ignore", divide="ignore"):
                    rate = acc / float(n_win) if n_win > 0 else np.full(scale.shape, np.nan)
                self.jump_scales.append(scale)
                self.acceptance_maps.append(np.where(self.mask == 1, rate, np.nan))
                self.adapted_until = int(k) * adapt_cfg.window
            self.jump_scale, self.acceptance_map = self.jump_scales[0], self.acceptance_maps[0]

    def _outputs(self, temper_group, last_swap_round, posterior_burn_in, hist_cfg):
        """Outputs (lib/run.py:539-549): ``run.rhat``, ``run.tempering``, ``run.parameters``, the two
        cubes and the posteriors."""
        cube, cube_shape, temper_cfg = self.cube, self.cube.data.shape, self.tempering_cfg
        # (tempering=: the rungs sample different distributions)
        self.rhat = self.gelman_rubin() if self.n_chains > 1 and temper_cfg is None else None
        self.tempering = None
        if temper_group is not None:
            self.tempering = _tempering.TemperingReport.from_group(temper_group, temper_cfg["betas"],
                                                                   temper_cfg["swap_every"], last_swap_round,
                                                                   temper_cfg.get("patch"))
            temper_group.close()
        self.parameters = self.extract_parameters()
        self.convolved_cube = Cube(data=self.simulate_convolved(cube_shape, self.parameters),
                                   meta=self.cube.meta, x=cube.x, y=cube.y, z=cube.z)
        self.clean_cube = Cube(data=self.simulate_clean(cube_shape, self.parameters),
                               meta=self.cube.meta, x=cube.x, y=cube.y, z=cube.z)
        # posterior moments of the samples' cubes (still on the device: fetched on access)
        self.posteriors, self.posterior = None, None
        if posterior_burn_in is not None:
            self.posteriors = [_posterior.PosteriorMoments.from_engine(eng, self.cube, hist_cfg is not None)
                               for eng in (self.engines if temper_cfg is None else self.engines[:1])]
            if hist_cfg is not None:
                for pm in self.posteriors:
                    pm.histograms.pilot, pm.histograms.span = hist_cfg["pilot"], hist_cfg["span"]
            self.posterior = self.posteriors[0] if len(self.posteriors) == 1 else \
                _posterior.pooled(self.posteriors, self.cube)
            if self._regions_cfg is not None:      # every chain its own; the pooled one concatenates them
                for pm, eng in zip(self.posteriors, self.engines):
                    pm.regions = _regions.RegionPosterior.from_engine(eng, self._regions_cfg["ids"])
                if len(self.posteriors) > 1:
                    self.posterior.regions = _regions.pooled([pm.regions for pm in self.posteriors])
            if self._predictive_cfg is not None:   # every chain its own; the pooled one merges them exactly
                nu = 0 if self._robust_cfg is None else self._robust_cfg["nu"]
                for pm, eng in zip(self.posteriors, self.engines):
                    pm.predictive = _predictive.PredictiveAccuracy.from_engine(eng, nu)
                if len(self.posteriors) > 1:
                    self.posterior.predictive = _predictive.pooled(
                        [pm.predictive for pm in self.posteriors],
                        _predictive.base_ivar(self.cube.data, self.variance_cube))
            if self.posterior.count == 0:
                self.logger.warning("posterior_burn_in=%d: the run stopped at iteration %d, before "
                                    "the first accumulated sweep; run.posterior holds no sample"
                                    % (posterior_burn_in, self.iterations_done))
        # robust=: the weights (still on the device: fetched on access)
        self.robusts, self.robust = None, None
        if self._robust_cfg is not None:
            self.robusts = [_robust.RobustReport.from_engine(eng, self._robust_cfg, self.cube)
                            for eng in self.engines]
            self.robust = self.robusts[0] if len(self.robusts) == 1 else \
                _robust.pooled(self.robusts, self.cube)
        # noise=: the series of scales (still on the device: fetched on access)
        self.noises, self.noise = None, None
        if self._noise_cfg is not None:
            burn_in = None if posterior_burn_in is None else posterior_burn_in + self.sweep_origin
            self.noises = [_noise.NoiseReport.from_engine(eng, self._noise_cfg, burn_in, self.sweep_origin + 1)
                           for eng in self.engines]
            self.noise = self.noises[0] if len(self.noises) == 1 else _noise.pooled(self.noises)

    # ------------------------------------------------------------------------

    def roughness(self, parameters=None):
        """``(E_a, E_c, E_w, pairs)``: the sums of squared differences between horizontally and
        vertically adjacent unmasked spaxels of an (H, W, 3) parameter map, and the number of such
        pairs -- what ``smoothness=`` penalises, summed on the device (d3d_prior_energy).
        ``parameters=None``: ``run.parameters``, the extracted map."""
        if self._host_model:
            self._refuse_host_model("roughness()")
        if parameters is None:
            parameters = self.parameters
        parameters = np.asarray(getattr(parameters, "data", parameters), dtype=np.float64)
        return self.engine.prior_energy(parameters)

    def _sweep_chains(self, n, first, all_likelihoods):
        """n sweeps of every chain: ONE launch per colour class for all of them where the
        library can (d3d_mh_sweeps_batch: cubes up to 256 channels -- a small cube's launch
        carries R times the windows for about the same latency), else the chains' own
        launches on their own streams, enqueued concurrently (ensemble.sweep_chains)."""
        if getattr(self, "_batched", True):
            try:
                acc = ensemble.sweep_chains_batched(self.engines, n, first, self.keep_one_in,
                                                    self.chains, all_likelihoods)
                self._batched = True
                return acc
            except NotImplementedError as exc:
                self.logger.info("chains advance on their own streams (%s)" % exc)
                self._batched = False
        return ensemble.sweep_chains(self.engines, n, first, self.keep_one_in, self.chains,
                                     all_likelihoods)

    def gelman_rubin(self, percentage=50.):
        """Per-parameter potential scale reduction R-hat (Gelman & Rubin 1992) over the last
        ``percentage`` % of the saved samples of the ``chains=R`` chains, shape (H, W, P):
        sqrt(((n-1)/n W + B/n) / W), W the mean within-chain variance and B/n the variance of
        the chain means.  NaN where a parameter did not move (masked spaxels)."""
        if self.n_chains < 2 or self.tempering_cfg is not None:
            raise ValueError("R-hat needs chains >= 2 (the rungs of tempering= sample different "
                             "distributions)")
        n_valid = min(self._n_valid(self.iterations_done), self.chain.shape[0])
        if n_valid < 2:                          # (a variance needs two saved samples)
            return np.full(self.chain.shape[1:], np.nan)
        first = min(int((100. - percentage) * n_valid / 100.), n_valid - 2)
        tail = np.stack([np.asarray(ch[first:n_valid]) for ch in self.chains])   # (R, n, H, W, P)
        n = tail.shape[1]
        with np.errstate(invalid="ignore", divide="ignore"):
            within = tail.var(axis=1, ddof=1).mean(axis=0)
            between = tail.mean(axis=1).var(axis=0, ddof=1)
            return np.sqrt(((n - 1.) / n * within + between) / within)

    def _n_valid(self, iteration):
        """The chain slots written once sweep ``iteration`` is done: slot 0 is the start."""
        return (iteration - 1) // self.keep_one_in + 1

    # (what test_gpu_run reads of the whole-chain accounting of a resumed run)
    _acc_base = property(lambda self: self._acceptance._acc_base)
    _it_base = property(lambda self: self._acceptance._it_base)

    def _read_checkpoint(self, resume_state):
        """``resume_state=``, the ``<name>_state.npz`` that `_write_checkpoint` wrote: refuses a
        state this run cannot continue, and returns the sweep origin of this segment, the state
        (whose accepted counts `_Acceptance` goes on from) and what `adapt.check_resume` restores
        per chain -- ``(0, None, None)`` without one.  No device work."""
        if resume_state is None:
            return 0, None, None
        state = np.load(resume_state) if isinstance(resume_state, str) else resume_state
        files = getattr(state, "files", state)
        saved_chains = int(state["n_chains"]) if "n_chains" in files else 1
        if saved_chains != self.n_chains:
            raise ValueError("resume_state holds %d chain(s), this run has chains=%d"
                             % (saved_chains, self.n_chains))
        if int(state["seed"]) != self.seed:
            self.logger.warning("resume_state was written with seed %d, this run uses %d"
                                % (int(state["seed"]), self.seed))
        sweep_origin = int(state["sweep_origin"]) + int(state["iteration"]) - 1
        resumed_adapt = _adapt.check_resume(state, files, self._adapt_cfg, self.n_chains,
                                            self.mask.shape)
        _prior.check_resume(state, files, self.smoothness)
        _tempering.check_resume(state, files, self.tempering_cfg)
        _robust.check_resume(state, files, self._robust_cfg)
        _noise.check_resume(state, files, self._noise_cfg)
        _prepare.check_resume(state, files,
                              None if self.prepared is None else self.prepared.settings)
        # (a checkpoint without a line shape was written by a single-Gaussian run)
        if self.line_shape is not None:
            saved = SINGLE_LINE_SHAPE
            if "line_offsets" in files:
                saved = (state["line_offsets"], state["line_ratios"])
            if not (np.array_equal(np.asarray(saved[0], dtype=np.float64),
                                   np.asarray(self.line_shape[0], dtype=np.float64))
                    and np.array_equal(np.asarray(saved[1], dtype=np.float64),
                                       np.asarray(self.line_shape[1], dtype=np.float64))):
                raise ValueError("resume_state was written with the line shape offsets %s, "
                                 "ratios %s; this run's model has offsets %s, ratios %s"
                                 % (tuple(np.ravel(saved[0])), tuple(np.ravel(saved[1])),
                                    self.line_shape[0], self.line_shape[1]))
            # (a checkpoint without a table digest was written by a run of Gaussians)
            saved_digest = str(state["line_table_digest"]) if "line_table_digest" in files else None
            if saved_digest != self.line_table_digest:
                raise ValueError("resume_state was written with %s; this run's model has %s"
                                 % ("Gaussian lines" if saved_digest is None
                                    else "the line table " + saved_digest[:16],
                                    "Gaussian lines" if self.line_table_digest is None
                                    else "the line table " + self.line_table_digest[:16]))
        return sweep_origin, state, resumed_adapt

    def _write_checkpoint(self, name, iteration):
        """`<name>_parameters.npy` (current map, reusable as initial_parameters,
        lib/run.py:790-797), `<name>_chain.npy` (slots written so far) and
        `<name>_state.npz` (iteration, seed, accepted count, `n_valid` = chain slots
        written so far: `resume_state=`).
        A memory-mapped chain (`chain_file=`) is flushed where it lives instead of
        copied: the checkpoint then names its files, and `chain_file == checkpoint`
        cannot rewrite the file under the open mapping.
        ``chains=R``: the parameter file holds the R maps, (R, H, W, P) -- what
        `initial_parameters=` takes for R chains --, chain r > 0 goes to
        `<name>_c<r>_chain.npy`, and the state records the chains' own accepted counts."""
        n_valid = self._n_valid(iteration)
        state = dict(iteration=iteration, seed=self.seed, sweep_origin=self.sweep_origin,
                     keep_one_in=self.keep_one_in, n_valid=n_valid, n_chains=self.n_chains,
                     chain_file="" if self._chain_file is None else str(self._chain_file))
        state.update(self._acceptance.state_record(iteration))
        if self.line_shape is not None:     # (resume_state= checks it)
            state["line_offsets"] = np.array(self.line_shape[0], dtype=np.float64)
            state["line_ratios"] = np.array(self.line_shape[1], dtype=np.float64)
        if self.line_table_digest is not None:
            state["line_table_digest"] = np.array(self.line_table_digest)
        if self.prepared is not None:       # (resume_state= checks them)
            state["prepare_settings"] = _prepare.settings_record(self.prepared.settings)
        if self.smoothness is not None:     # (resume_state= checks them)
            state["smoothness_sigmas"] = _prior.keyword_record(self.smoothness)
        if self._robust_cfg is not None:    # (resume_state= checks them; the weights are redrawn)
            state["robust_keywords"] = _robust.keyword_record(self._robust_cfg)
        if self._noise_cfg is not None:     # (resume_state= checks them; the series starts afresh)
            state.update(_noise.keyword_record(self._noise_cfg))
        if self.tempering_cfg is not None:  # (resume_state= checks them; counters and labels start afresh)
            state.update(_tempering.state_record(self.tempering_cfg))
        if self._adapt_cfg is not None:     # (resume_state= checks the keywords, restores the rest)
            got = [eng.adapt_get() for eng in self.engines]
            state["adapt_keywords"] = _adapt.keyword_record(self._adapt_cfg)
            state["adapt_scale"] = np.stack([g[0] for g in got])
            state["adapt_accepted"] = np.stack([g[1] for g in got])
            state["adapt_n_win"] = np.array([g[2] for g in got], dtype=np.int64)
            state["adapt_k"] = np.array([g[3] for g in got], dtype=np.int64)
        np.savez("%s_state.npz" % name, **state)
        if self._host_model:
            maps = [hc.params for hc in self._host_chains]
        else:
            maps = [eng.get_params() for eng in self.engines]
        params = maps[0] if self.n_chains == 1 else np.stack(maps)
        np.save("%s_parameters.npy" % name, params)
        if self._chain_file is not None:
            # slots past n_valid (recorded in the state file) are not written yet
            for ch, lk in zip(self.chains, self._likelihoods_maps):
                ch.flush()
                lk.flush()
        else:
            for r, ch in enumerate(self.chains):
                prefix = name if r == 0 else "%s_c%d" % (name, r)
                np.save("%s_chain.npy" % prefix, ch[:n_valid])
        self.logger.info("checkpoint at iteration %d (%d accepted) -> %s_*.npy"
                         % (iteration, state["accepted_count"], name))

    # ITERATORS ###############################################################

    def spaxel_iterator(self):
        """(y, x) of every unmasked spaxel, row-major (lib/run.py:553-566).
        The device sweep visits the same set colour by colour."""
        h, w = self.mask.shape
        for y in range(h):
            for x in range(w):
                if self.mask[y, x] == 1:
                    yield (y, x)

    # MCMC ####################################################################

    def jump_from(self, parameters, amplitude):
        """Host mirror of the Cauchy proposal (lib/run.py:570-579); the device
        draws its own from Philox."""
        size = len(parameters)
        u = np.random.default_rng().uniform(-CIRCLE_4TH, CIRCLE_4TH, size=size)
        return parameters + amplitude * np.tan(u)

    def extract_parameters(self, percentage=20.):
        """Mean of the last ``percentage`` % of the saved chain -- of every chain with
        ``chains=R`` -- (lib/run.py:581-593); slots never written (early stop) are ignored."""
        n_valid = max(1, min(self._n_valid(self.iterations_done), self.chain.shape[0]))
        s = int((100. - percentage) * n_valid / 100.)
        if self.n_chains == 1 or self.tempering_cfg is not None:     # (tempering=: rung 0 alone)
            return np.nanmean(self.chain[s:n_valid, ...], 0)
        # chains=R: the chains are pooled (equal lengths: the mean of their means)
        return np.nanmean(np.stack([np.nanmean(ch[s:n_valid, ...], 0) for ch in self.chains]), 0)

    # SIMULATOR ###############################################################

    def simulate_clean(self, shape, parameters):
        """Cube of the raw lines (lib/run.py:597-621), built on the device."""
        self._check_shape(shape)
        if self._host_model:
            return self._host_chain.clean_cube(np.asarray(parameters, dtype=np.float64))
        return self.engine.simulate(parameters, convolved=False)

    def simulate_convolved(self, shape, parameters):
        """Cube of the LSF- and FSF-convolved lines (lib/run.py:623-652), by the
        fused device forward model."""
        self._check_shape(shape)
        if self._host_model:
            return self.engine.convolve(
                self._host_chain.clean_cube(np.asarray(parameters, dtype=np.float64)))
        return self.engine.simulate(parameters, convolved=True)

    def contribution_of_spaxel(self, x, y, parameters, cube_width, cube_height, cube_depth,
                               fsf=None, lsf=None, lsf_fft=None):
        """
        Full-size cube holding the convolved contribution of one spaxel's line
        (lib/run.py:654-708).  Returns ``(cube, lsf_fft)`` like the reference;
        ``lsf_fft`` is passed through (the device does not use FFTs).  The taps
        are the run's own.
        """
        self._check_shape((cube_depth, cube_height, cube_width))
        # the line on the host (one spectrum), LSF and FSF on the device; like the
        # reference this ignores the mask, and the chain state is not touched
        one = np.zeros((cube_depth, cube_height, cube_width))
        one[:, y, x] = np.asarray(self.model.modelize(self, np.arange(cube_depth, dtype=float),
                                                      parameters), dtype=np.float64)
        return self.engine.convolve(one), lsf_fft

    def _check_shape(self, shape):
        if tuple(shape) != tuple(self.cube.data.shape):
            raise ValueError("shape %s differs from the run's cube %s"
                             % (tuple(shape), tuple(self.cube.data.shape)))

    # SAVES ###################################################################

    def save(self, name, clobber=False):
        """Write ``<name>_parameters.npy``, ``_chain.npy``, ``_matlab.mat``,
        ``_images.png``, ``_chain.png``, ``_convolved_cube.fits``,
        ``_clean_cube.fits``, ``_result.npz`` (lib/run.py:742-788); with ``noise=`` also
        ``_noise.npz``."""
        self.save_parameters_npy("%s_parameters.npy" % name)
        self.save_chain_npy("%s_chain.npy" % name)
        try:
            self.save_matlab("%s_matlab.mat" % name)
        except Exception as e:  # noqa
            self.logger.error(str(e))
        self.plot_images("%s_images.png" % name)
        self.plot_chain(filepath="%s_chain.png" % name)
        self.convolved_cube.to_fits("%s_convolved_cube.fits" % name, clobber)
        self.clean_cube.to_fits("%s_clean_cube.fits" % name, clobber)
        maps = {}
        if self.jump_scale is not None:
            maps = dict(jump_scale=self.jump_scale, acceptance_map=self.acceptance_map)
        np.savez("%s_result.npz" % name, chain=self.chain, likelihoods=self.likelihoods,
                 fsf=self.fsf, lsf=self.lsf if self.lsf is not None else np.zeros(0), **maps)
        if self.noise is not None:
            self.noise.save(name)

    def save_parameters_npy(self, filepath):
        """lib/run.py:790-797; reusable as ``initial_parameters``."""
        np.save(filepath, self.extract_parameters())

    def save_chain_npy(self, filepath):
        """lib/run.py:799-810."""
        np.save(filepath, self.chain)

    def save_matlab(self, filepath):
        """lib/run.py:812-840."""
        from scipy.io import savemat
        savemat(filepath, dict(parameters=self.extract_parameters(), chain=self.chain))

    # PLOTS ###################################################################

    def plot_chain(self, x=None, y=None, filepath=None, bound=True):
        """Chain and log acceptance ratio of one spaxel (lib/run.py:844-894)."""
        from matplotlib import pyplot as plot
        self._check_image_filepath(filepath)
        if x is None:
            x = int(math.floor(self.cube.shape[2] / 2.))
        if y is None:
            y = int(math.floor(self.cube.shape[1] / 2.))
        chain_t = np.transpose(self.chain[:, y, x, :])
        names = self.model.parameters()
        bmin, bmax = self.min_boundaries, self.max_boundaries
        plot.clf()
        for i, name in enumerate(names):
            plot.subplot2grid((2, len(names)), (0, i))
            plot.plot(chain_t[i])
            if bound:
                plot.ylim(bmin[i], bmax[i])
            plot.title(name, fontsize='small')
        plot.subplot2grid((2, len(names)), (1, 0), colspan=len(names))
        plot.plot(self.likelihoods[:, y, x])
        plot.title('likelihood', fontsize='small')
        if filepath is None:
            plot.show()
        else:
            plot.savefig(filepath)

    def plot_images(self, filepath=None):
        """Mosaic of measured / convolved / FSF / clean / mask images
        (lib/run.py:896-985)."""
        from matplotlib import pyplot as plot
        self._check_image_filepath(filepath)
        p = self.extract_parameters()
        panels = [
            ('Measured', np.nanmean(self.cube.data, 0)),
            ('Simulation Convolved', self.simulate_convolved(self.cube.data.shape, p).mean(0)),
            ('FSF', self.fsf),
            ('Simulation Clean', self.simulate_clean(self.cube.data.shape, p).mean(0)),
            ('Mask', self.mask),
        ]
        fig = plot.figure(1, figsize=(16, 9))
        plot.clf()
        plot.subplots_adjust(wspace=0.25, hspace=0.25, bottom=0.05, top=0.95, left=0.05,
                             right=0.95)
        for i, (title, image) in enumerate(panels):
            sub = fig.add_subplot(2, 3, i + 1)
            sub.set_title(title)
            plot.imshow(image, interpolation='nearest', origin='lower')
            plot.xticks(fontsize=8)
            plot.yticks(fontsize=8)
            plot.colorbar().ax.tick_params(labelsize=8)
        if filepath is None:
            plot.show()
        else:
            plot.savefig(filepath)

    def _check_image_filepath(self, filepath):
        if filepath is not None:
            _, extension = splitext(filepath)
            supported = ['.png', '.pdf']
            if extension not in supported:
                raise ValueError("Extension '%s' is not supported, you may use one of %s"
                                 % (extension, ', '.join(supported)))
