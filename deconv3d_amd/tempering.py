# coding=utf-8
"""
Parallel tempering of ``Run(tempering=...)``: keyword validation, the ladder of inverse
temperatures, the report and the checkpoint record.  The reference runs one chain whose MH ratio
is the likelihood's (lib/run.py:426-438); it cannot cross between modes of ``c``.  Here R rungs
sample ``L^beta_r x prior`` -- the same model with the variance divided by ``beta_r`` -- and
adjacent rungs trade their states on the device (include/deconv3d_hip.h: d3d_temper_swap).
Nothing here touches the device.
"""
from __future__ import annotations

import math

import numpy as np

KEYS = ("betas", "rungs", "beta_min", "swap_every", "patch")
MAX_RUNGS = 64            # d3d_temper_create


def geometric_ladder(rungs, beta_min):
    """``beta_min ** (r / (rungs - 1))`` for r = 0 .. rungs - 1: 1 first, ``beta_min`` last."""
    return tuple(float(beta_min) ** (r / float(rungs - 1)) for r in range(rungs))


def _integer(name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < least:
        raise ValueError("tempering %s= MUST be an integer >= %d, got %r" % (name, least, v))
    return int(v)


def check_keywords(tempering):
    """``tempering=`` as ``dict(betas=(1., ...), swap_every=n)``, or None when the keyword is None;
    ValueError otherwise.  A dict with either ``betas`` (1 first, strictly decreasing, finite and
    > 0) or ``rungs`` plus ``beta_min`` (the geometric ladder), ``swap_every`` (default 1) and
    ``patch`` (default None: the rungs trade whole cubes; an integer p >= 1: the unmasked spaxels of
    tiles of p x p spaxels, d3d_temper_set_patch)."""
    if tempering is None:
        return None
    if not isinstance(tempering, dict):
        raise ValueError("tempering= MUST be a dict with betas= or rungs= and beta_min=, got %r" % (tempering,))
    unknown = sorted(set(tempering) - set(KEYS), key=str)
    if unknown:
        raise ValueError("tempering= has unknown key(s) %s: any of %s"
                         % (", ".join(repr(k) for k in unknown), ", ".join(KEYS)))
    has_betas = tempering.get("betas") is not None
    has_ladder = tempering.get("rungs") is not None or tempering.get("beta_min") is not None
    if has_betas == has_ladder:
        raise ValueError("tempering= takes either betas= or rungs= with beta_min=, not %s"
                         % ("both" if has_betas else "neither"))
    if has_betas:
        if isinstance(tempering["betas"], (str, bytes)):
            raise ValueError("tempering betas= MUST be a sequence of numbers, got %r" % (tempering["betas"],))
        try:
            betas = tuple(float(b) for b in tempering["betas"])
        except (TypeError, ValueError):
            raise ValueError("tempering betas= MUST be a sequence of numbers, got %r" % (tempering["betas"],))
    else:
        if tempering.get("rungs") is None or tempering.get("beta_min") is None:
            raise ValueError("tempering= as a ladder needs both rungs= and beta_min=")
        rungs = _integer("rungs", tempering["rungs"], 2)
        try:
            beta_min = float(tempering["beta_min"])
        except (TypeError, ValueError):
            raise ValueError("tempering beta_min= MUST be a number in (0, 1), got %r" % (tempering["beta_min"],))
        if isinstance(tempering["beta_min"], bool) or math.isnan(beta_min) or not 0. < beta_min < 1.:
            raise ValueError("tempering beta_min= MUST be a number in (0, 1), got %r" % (tempering["beta_min"],))
        betas = geometric_ladder(rungs, beta_min)
    if not 2 <= len(betas) <= MAX_RUNGS:
        raise ValueError("tempering= takes 2 to %d rungs, got %d" % (MAX_RUNGS, len(betas)))
    if betas[0] != 1.:
        raise ValueError("tempering betas= MUST start with 1 (rung 0 samples the posterior), got %r" % (betas[0],))
    for r, b in enumerate(betas):
        if not (math.isfinite(b) and b > 0.):
            raise ValueError("tempering betas= MUST be finite and > 0, got %r at rung %d" % (b, r))
        if r and not b < betas[r - 1]:
            raise ValueError("tempering betas= MUST be strictly decreasing, got %r after %r" % (b, betas[r - 1]))
    swap_every = _integer("swap_every", tempering.get("swap_every", 1), 1)
    cfg = dict(betas=betas, swap_every=swap_every)
    if tempering.get("patch") is not None:      # (no key: whole cubes, the dict of a run without it)
        cfg["patch"] = _integer("patch", tempering["patch"], 1)
    return cfg


def check_run(cfg, n_chains, host_model, model_name):
    """The refusals of ``Run``: the rungs take the chains' place; the device swaps device state."""
    if cfg is None:
        return
    if n_chains != 1:
        raise ValueError("tempering= with chains=%d: the rungs take the chains' place, use chains=1" % n_chains)
    if host_model:
        raise NotImplementedError(
            "tempering=: the line model %s is evaluated on the host; the device exchanges the "
            "states only of the models it evaluates itself" % model_name)


def calls_until_swap(n, iteration, sweep_origin, swap_every):
    """``n`` sweeps, the first of them sweep ``iteration``, capped so that the call ends at the next
    sweep s with ``(s + sweep_origin) % swap_every == 0``; and the round ``(s + sweep_origin) //
    swap_every`` of the exchange due after the call, or None when it ends before s."""
    to_next = (-(iteration + sweep_origin)) % swap_every + 1     # 1 .. swap_every sweeps up to s
    if n < to_next:
        return n, None
    return to_next, (iteration + to_next - 1 + sweep_origin) // swap_every


class TemperingReport(object):
    """What the exchange did: ``betas`` (R), ``swap_attempts`` / ``swap_accepts`` / ``swap_rates``
    per adjacent pair (R - 1; NaN where nothing was proposed), ``energy_mean`` / ``energy_std`` per
    rung (R) -- of ``E = 1/2 sum err^2 / var`` under the untempered variance, of the state at the
    rung before each exchange; what thermodynamic integration would need --, ``energy_count``,
    ``labels`` (R: the rung whose start the state now at rung r descends from) and ``rounds``;
    ``last_round`` is the number of the last exchange round (None: none yet) and ``last`` its
    ``energy`` (R), ``u``, ``logu`` and ``decided`` (R - 1; NaN / -1 for a pair not proposed).
    With ``patch`` (the tile side; None: whole cubes) the rungs trade patches of spaxels:
    ``patch_attempts`` / ``patch_accepts`` / ``patch_rates`` per pair count the patches proposed
    and accepted, the ``swap_*`` counters stand still, ``labels`` is None (states no longer travel
    whole) and ``last_patches`` is the per-tile record of the last round
    (``TemperGroup.last_patches``)."""

    def __init__(self, betas, swap_every, rounds, attempts, accepts, energy_n, energy_mean, energy_m2, labels,
                 last_round=None, last=None, patch=None, patch_attempts=None, patch_accepts=None,
                 last_patches=None):
        self.betas = np.array(betas, dtype=np.float64)
        self.swap_every = int(swap_every)
        self.rounds = int(rounds)
        self.swap_attempts = np.array(attempts, dtype=np.int64)
        self.swap_accepts = np.array(accepts, dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.swap_rates = np.where(self.swap_attempts > 0,
                                       self.swap_accepts / self.swap_attempts.astype(np.float64), np.nan)
        self.energy_count = np.array(energy_n, dtype=np.int64)
        self.energy_mean = np.where(self.energy_count > 0, np.array(energy_mean, dtype=np.float64), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.energy_std = np.where(self.energy_count > 1,
                                       np.sqrt(np.array(energy_m2, dtype=np.float64)
                                               / np.maximum(self.energy_count - 1, 1)), np.nan)
        self.patch = None if patch is None else int(patch)
        self.labels = np.array(labels, dtype=np.int32) if self.patch is None else None
        self.last_round = None if last_round is None else int(last_round)
        self.last = last
        n_pairs = len(self.betas) - 1
        self.patch_attempts = np.zeros(n_pairs, dtype=np.int64) if patch_attempts is None \
            else np.array(patch_attempts, dtype=np.int64)
        self.patch_accepts = np.zeros(n_pairs, dtype=np.int64) if patch_accepts is None \
            else np.array(patch_accepts, dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.patch_rates = np.where(self.patch_attempts > 0,
                                        self.patch_accepts / self.patch_attempts.astype(np.float64), np.nan)
        self.last_patches = last_patches

    @classmethod
    def from_group(cls, group, betas, swap_every, last_round=None, patch=None):
        got = group.get()
        patches = group.get_patches() if patch is not None else dict(attempts=None, accepts=None)
        return cls(betas, swap_every, got["rounds"], got["attempts"], got["accepts"], got["energy_n"],
                   got["energy_mean"], got["energy_m2"], got["labels"], last_round,
                   group.last() if got["rounds"] > 0 else None, patch, patches["attempts"], patches["accepts"],
                   group.last_patches() if patch is not None and got["rounds"] > 0 else None)

    def save(self, prefix):
        """``<prefix>_tempering.npz``."""
        np.savez("%s_tempering.npz" % prefix, betas=self.betas, swap_every=self.swap_every, rounds=self.rounds,
                 swap_attempts=self.swap_attempts, swap_accepts=self.swap_accepts, swap_rates=self.swap_rates,
                 energy_count=self.energy_count, energy_mean=self.energy_mean, energy_std=self.energy_std,
                 labels=np.zeros(0, dtype=np.int32) if self.labels is None else self.labels,
                 patch=0 if self.patch is None else self.patch, patch_attempts=self.patch_attempts,
                 patch_accepts=self.patch_accepts, patch_rates=self.patch_rates)


def _fmt(values):
    return "(%s)" % ", ".join("%g" % float(v) for v in np.ravel(values))


def state_record(cfg):
    """What a checkpoint's state holds of the keyword (``tempering_patch``: 0 for whole cubes)."""
    return dict(tempering_betas=np.array(cfg["betas"], dtype=np.float64),
                swap_every=np.array(cfg["swap_every"], dtype=np.int64),
                tempering_patch=np.array(cfg.get("patch") or 0, dtype=np.int64))


def check_resume(state, files, cfg):
    """ValueError when ``resume_state`` was written with another ladder, cadence or patch size than
    this run's (a state without ``tempering_patch`` was written with whole-cube exchanges)."""
    saved = "tempering_betas" in files
    if cfg is None and not saved:
        return
    if cfg is None:
        raise ValueError("resume_state was written with tempering betas=%s; this run has none"
                         % _fmt(state["tempering_betas"]))
    if not saved:
        raise ValueError("resume_state was written without tempering=; this run asks for betas=%s"
                         % _fmt(cfg["betas"]))
    old, new = np.asarray(state["tempering_betas"], dtype=np.float64), np.array(cfg["betas"], dtype=np.float64)
    if old.shape != new.shape or not np.array_equal(old, new):
        raise ValueError("resume_state was written with tempering betas=%s; this run has betas=%s"
                         % (_fmt(old), _fmt(new)))
    if int(state["swap_every"]) != cfg["swap_every"]:
        raise ValueError("resume_state was written with tempering swap_every=%d; this run has swap_every=%d"
                         % (int(state["swap_every"]), cfg["swap_every"]))
    old_patch = int(state["tempering_patch"]) if "tempering_patch" in files else 0
    new_patch = cfg.get("patch") or 0
    if old_patch != new_patch:
        raise ValueError("resume_state was written with tempering patch=%s; this run has patch=%s"
                         % (old_patch or None, new_patch or None))
