# coding=utf-8
"""
Per-spaxel jump scales of ``Run(adapt_sweeps=N)``: keyword validation and the checkpoint
record.  The reference proposes every spaxel's (c, w) with the one ``jump_amplitude``
(lib/run.py:251-262, 570-579); the device keeps a multiplicative scale per spaxel and moves it
towards ``adapt_target`` every ``adapt_window`` sweeps of the first N (include/deconv3d_hip.h:
d3d_adapt_begin).  Nothing here touches the device.
"""
from __future__ import annotations

import math

import numpy as np

# order of the values in a checkpoint's ``adapt_keywords``
KEYWORDS = ("adapt_sweeps", "adapt_window", "adapt_target", "adapt_gain", "adapt_scale_min",
            "adapt_scale_max")


def check_keywords(adapt_sweeps, adapt_window=50, adapt_target=0.25, adapt_gain=2.0,
                   adapt_scale_range=(1e-3, 1e3)):
    """The five keywords as (sweeps, window, target, gain, (scale_min, scale_max)), or
    ValueError: the checks of d3d_adapt_begin, made before any device work."""
    def integer(value, name):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError("%s= MUST be an integer, got %r" % (name, value))
        return int(value)
    sweeps = integer(adapt_sweeps, "adapt_sweeps")
    window = integer(adapt_window, "adapt_window")
    if sweeps < 1:
        raise ValueError("adapt_sweeps= MUST be a positive number of sweeps, got %d" % sweeps)
    if window < 1:
        raise ValueError("adapt_window= MUST be a positive number of sweeps, got %d" % window)
    if window > sweeps:
        raise ValueError("adapt_window=%d exceeds adapt_sweeps=%d: no window would ever fill"
                         % (window, sweeps))
    target, gain = float(adapt_target), float(adapt_gain)
    if not 0. < target < 1.:
        raise ValueError("adapt_target= MUST be an acceptance rate inside (0, 1), got %r"
                         % (adapt_target,))
    if not (gain > 0. and math.isfinite(gain)):
        raise ValueError("adapt_gain= MUST be a positive number, got %r" % (adapt_gain,))
    try:
        lo, hi = (float(v) for v in adapt_scale_range)
    except (TypeError, ValueError):
        raise ValueError("adapt_scale_range= MUST be a (min, max) pair, got %r" % (adapt_scale_range,))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo > 0. and hi > 0.):
        raise ValueError("adapt_scale_range= MUST hold finite, positive scales, got %r"
                         % (adapt_scale_range,))
    if lo > hi:
        raise ValueError("adapt_scale_range= has min %g > max %g" % (lo, hi))
    return sweeps, window, target, gain, (lo, hi)


def keyword_record(cfg):
    """The keywords as the float64 vector a checkpoint's state holds."""
    sweeps, window, target, gain, (lo, hi) = cfg
    return np.array([sweeps, window, target, gain, lo, hi], dtype=np.float64)


def check_resume(state, files, cfg, n_chains, hw):
    """What ``resume_state=`` must restore -- per chain (scale map, counters, n_win, k) -- or None
    when neither the state nor this run adapts.  ValueError when they disagree."""
    saved = "adapt_keywords" in files
    if cfg is None and not saved:
        return None
    if cfg is None:
        raise ValueError("resume_state was written with adapt_sweeps=%d; this run has none "
                         "(its jump scales would be lost)" % int(state["adapt_keywords"][0]))
    if not saved:
        raise ValueError("resume_state was written without adapt_sweeps=; this run asks for "
                         "adapt_sweeps=%d" % cfg[0])
    old, new = np.asarray(state["adapt_keywords"], dtype=np.float64), keyword_record(cfg)
    if old.shape != new.shape or not np.array_equal(old, new):
        raise ValueError("resume_state was written with %s; this run has %s"
                         % (", ".join("%s=%g" % kv for kv in zip(KEYWORDS, old)),
                            ", ".join("%s=%g" % kv for kv in zip(KEYWORDS, new))))
    scale = np.asarray(state["adapt_scale"], dtype=np.float64)
    acc = np.asarray(state["adapt_accepted"], dtype=np.uint32)
    if scale.shape != (n_chains,) + tuple(hw) or acc.shape != scale.shape:
        raise ValueError("resume_state holds jump scale maps of shape %s, this run needs %s"
                         % (scale.shape, (n_chains,) + tuple(hw)))
    n_win = np.asarray(state["adapt_n_win"], dtype=np.int64).reshape(n_chains)
    k = np.asarray(state["adapt_k"], dtype=np.int64).reshape(n_chains)
    return [(scale[r], acc[r], int(n_win[r]), int(k[r])) for r in range(n_chains)]
