"""
d3d_ctx_set_stream: the library on a caller-owned HIP stream, which is how a host program keeps
the library's launches ordered with its own.  Everything the context queues -- the forward model,
the reference-layout convolution, the residual, the chi2 map, MH sweeps -- must give the bits it
gives on the context's own stream, and NULL must return the context to that stream.

The caller's stream is created with the HIP runtime libdeconv3d_hip.so is linked to (found as
already loaded: no second copy).  ``torch.cuda.Stream().cuda_stream`` is such a handle only where
torch runs on that same runtime; a wheel that bundles its own libamdhip64 is a second runtime in
the process, which finds no device once the first holds it, and whose handles would mean nothing
to the library (include/deconv3d_hip.h: d3d_ctx_set_stream).
"""
import ctypes
import os

import numpy as np
import pytest

from deconv3d_amd import _lib
from tests.cases import make_case

pytestmark = pytest.mark.gpu

HIP_STREAM_NON_BLOCKING = 1


def library_hip_runtime():
    """The libamdhip64 that was loaded with libdeconv3d_hip.so (RTLD_NOLOAD: never another)."""
    _lib.load()
    for major in range(12, 4, -1):
        try:
            return ctypes.CDLL("libamdhip64.so.%d" % major, mode=os.RTLD_NOLOAD)
        except OSError:
            pass
    raise RuntimeError("libdeconv3d_hip.so is loaded but no libamdhip64.so.<major> is")


def test_caller_owned_stream_gives_the_same_bits_as_the_own_stream():
    case = make_case("c1")
    shape = (case["D"], case["H"], case["W"])
    cube = np.random.default_rng(3).normal(size=shape)
    engines = []
    for k in range(2):
        eng = _lib.Engine(shape, case["fsf"].shape)
        eng.set_taps(case["fsf"], case["lsf"])
        eng.set_data(case["data"], case["var"], mask=case["mask"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=5, refresh_every=0)
        engines.append(eng)
    hip = library_hip_runtime()
    stream = ctypes.c_void_p(None)
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), HIP_STREAM_NON_BLOCKING) == 0 and stream.value
    try:
        engines[1].set_stream(stream.value)

        def step(eng, first_sweep, n_sweeps, everything):
            out = {}
            if everything:
                eng.set_params(case["init"])
                out["sim"] = eng.forward()
                out["conv"] = eng.convolve(cube)
                out["residual"] = eng.residual()
                out["chi2"], out["chi2_total"] = eng.chi2_map()
            out["accepted"] = eng.mh_sweeps(n_sweeps, first_sweep)
            out["params"] = eng.get_params()
            out["err"] = eng.download_slot(_lib.SLOT_ERR)
            return out

        def same(a, b):
            assert sorted(a) == sorted(b)
            for key in a:
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)

        own, theirs = [step(e, 1, 2, True) for e in engines]
        assert own["accepted"] > 0
        same(own, theirs)
        engines[1].set_stream(None)                      # back on the context's own stream
        own, theirs = [step(e, 3, 1, False) for e in engines]
        same(own, theirs)
    finally:
        for eng in engines:
            eng.close()
        assert hip.hipStreamDestroy(stream) == 0
