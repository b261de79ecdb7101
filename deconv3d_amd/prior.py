# coding=utf-8
"""
Smoothness prior of ``Run(smoothness=...)``: keyword validation and the checkpoint record.
The reference samples a flat prior inside the bounds, every spaxel on its own
(lib/run.py:426-438, 491-496); the device adds a pairwise Gaussian prior between 4-neighbours,
``-1/2 sum_<i,j> sum_k (theta_i,k - theta_j,k)^2 / sigma_k^2`` (include/deconv3d_hip.h:
d3d_prior_begin).  Nothing here touches the device.
"""
from __future__ import annotations

import math

import numpy as np

# the parameters a sigma may be given for, in the order of the device's lam[3]
NAMES = ("a", "c", "w")


def check_keywords(smoothness):
    """``smoothness=`` as the sigmas ``(sigma_a, sigma_c, sigma_w)`` -- ``inf`` where the
    parameter has no prior -- or None when the keyword is None; ValueError otherwise.  A dict
    with any of ``a``, ``c``, ``w``, or a 3-sequence; a sigma is the expected difference between
    neighbouring spaxels in the parameter's own unit, ``None`` or ``inf`` for none."""
    if smoothness is None:
        return None
    if isinstance(smoothness, dict):
        unknown = sorted(set(smoothness) - set(NAMES), key=str)
        if unknown:
            raise ValueError("smoothness= has unknown parameter(s) %s: any of %s"
                             % (", ".join(repr(k) for k in unknown), ", ".join(NAMES)))
        values = [smoothness.get(k) for k in NAMES]
    else:
        if isinstance(smoothness, (str, bytes)):
            raise ValueError("smoothness= MUST be a dict or a 3-sequence, got %r" % (smoothness,))
        try:
            values = list(smoothness)
        except TypeError:
            raise ValueError("smoothness= MUST be a dict or a 3-sequence, got %r" % (smoothness,))
        if len(values) != 3:
            raise ValueError("smoothness= as a sequence MUST hold the 3 sigmas of %s, got %d value(s)"
                             % (NAMES, len(values)))
    sigmas = []
    for name, v in zip(NAMES, values):
        if v is None:
            sigmas.append(math.inf)
            continue
        if isinstance(v, bool):
            raise ValueError("smoothness %s= MUST be a positive number, got %r" % (name, v))
        try:
            s = float(v)
        except (TypeError, ValueError):
            raise ValueError("smoothness %s= MUST be a positive number, got %r" % (name, v))
        if math.isnan(s) or not s > 0.:
            raise ValueError("smoothness %s= MUST be a positive sigma (None or inf: no prior), got %r"
                             % (name, v))
        sigmas.append(s)
    return tuple(sigmas)


def lam_of(sigmas):
    """lam_k = 1 / sigma_k^2 (0 for an infinite sigma) as the float64 vector of d3d_prior_begin."""
    return np.array([0. if math.isinf(s) else 1. / (s * s) for s in sigmas], dtype=np.float64)


def check_fsf(sigmas, fsf_shape):
    """ValueError for an FSF one spaxel wide: adjacent spaxels would share a colour class."""
    if sigmas is not None and (fsf_shape[0] == 1 or fsf_shape[1] == 1):
        raise ValueError("smoothness= with a %d x %d FSF: adjacent spaxels would share a colour "
                         "class of the sweep" % (fsf_shape[0], fsf_shape[1]))


def _fmt(values):
    return "(%s)" % ", ".join("%g" % float(v) for v in np.ravel(values))


def keyword_record(sigmas):
    """The sigmas as the float64 vector a checkpoint's state holds."""
    return np.array(sigmas, dtype=np.float64)


def check_resume(state, files, sigmas):
    """ValueError when ``resume_state`` was written with other sigmas than this run's."""
    saved = "smoothness_sigmas" in files
    if sigmas is None and not saved:
        return
    if sigmas is None:
        raise ValueError("resume_state was written with smoothness=%s; this run has none"
                         % _fmt(state["smoothness_sigmas"]))
    if not saved:
        raise ValueError("resume_state was written without smoothness=; this run asks for "
                         "smoothness=%s" % _fmt(sigmas))
    old, new = np.asarray(state["smoothness_sigmas"], dtype=np.float64), keyword_record(sigmas)
    if old.shape != new.shape or not np.array_equal(old, new):
        raise ValueError("resume_state was written with smoothness=%s; this run has smoothness=%s"
                         % (_fmt(old), _fmt(new)))
