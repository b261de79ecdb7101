"""Cost of one replica-exchange round (d3d_temper_swap: k_temper_energy, k_temper_decide,
k_temper_exchange on the leader's stream) on one GPU:

    python tools/temper_time.py [shapes=64,64,64,8;128,300,300,2]

For every `D,H,W,rungs` (the bench's taps: Moffat 11x11, 17-tap LSF; geometric ladder down to
beta = 0.05) one round of parity 0 -- rungs / 2 pairs proposed --
  * with every proposed pair ACCEPTED: the even rungs hold the starting map and the odd ones the truth,
    so that the colder state of every pair has by far the higher energy; the states are put back before
    every repetition (an accepted pair is in order afterwards);
  * with NO pair accepted: the round after it, repeated;
and beside them one sweep of all rungs (d3d_mh_sweeps_batch), the work a round sits between.

HIP events on the leader's stream around the call, median of 7 repetitions (20 rounds per repetition
where none is accepted); the wall clock of the call with the wait for the stream beside it.
profiles/temper_time.txt.

    python tools/temper_time.py --patch P [shapes=...]

times the exchange of patches of P x P spaxels instead (d3d_temper_set_patch: the energies, the
lines of the proposed rungs, one k_temper_patch launch per tile colour), the same two states -- the
round right after arming, in which (nearly) every patch is accepted, and the same round repeated,
in which (nearly) none is; the shares are printed -- and writes profiles/patch_time.txt."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
if "--patch" in sys.argv:
    args["patch"] = sys.argv[sys.argv.index("--patch") + 1]
PATCH = int(args.get("patch", 0))
LINES = []


def report(line):
    print(line, flush=True)
    LINES.append(line)
SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.get("shapes", "64,64,64,8;128,300,300,2").split(";")]
REPS = 7


def measure(D, H, W, R):
    import bench as B
    from deconv3d_amd import _lib, tempering
    fsf, lsf = B.build_taps(D, 11)
    betas = tempering.geometric_ladder(R, 0.05)
    engines = []
    for r in range(R):
        eng = _lib.Engine((D, H, W), fsf.shape)
        eng.set_taps(fsf, lsf)
        if r == 0:
            data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
        eng.set_data(data, var / betas[r])
        eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345 + r, refresh_every=0)
        engines.append(eng)
    lead = engines[0]

    def arm():
        for r, eng in enumerate(engines):
            eng.set_params(truth if r % 2 else init)
            eng.residual(fetch=False)
        for eng in engines:
            eng.sync()

    def timed(call, per=1):
        t0 = time.perf_counter()
        lead.timer_start()
        for _ in range(per):
            call()
        ms = lead.timer_stop()
        return ms * 1e3 / per, (time.perf_counter() - t0) * 1e6 / per

    def share():
        d = group.last_patches()["decided"]
        return int((d == 1).sum()), int((d >= 0).sum())

    with _lib.TemperGroup(engines, betas, seed=1, patch=PATCH or None) as group:
        arm()
        group.swap(0)                                  # warm-up: code objects, first launches
        assert PATCH or (group.last()["decided"][0::2] == 1).all()
        acc, rej, shares = [], [], [None, None]
        for _ in range(REPS):
            arm()
            acc.append(timed(lambda: group.swap(0)))
            assert PATCH or (group.last()["decided"][0::2] == 1).all()
            shares[0] = share() if PATCH else None
            rej.append(timed(lambda: group.swap(0), per=20))
            assert PATCH or (group.last()["decided"][0::2] == 0).all()
            shares[1] = share() if PATCH else None
        _lib.mh_sweeps_batch(engines, 2, first_sweep=1)
        sweep = [timed(lambda: _lib.mh_sweeps_batch(engines, 1, first_sweep=3)) for _ in range(REPS)]
    for eng in engines:
        eng.close()
    pairs = R // 2
    moved = pairs * 4 * (lead.shape[1] * lead.shape[2] * ((D + 1) // 2 * 2 + 3)) * 8 / 1e6
    names = ("every pair accepted", "no pair accepted") if not PATCH else (
        "patch %d, %d of %d patches accepted" % ((PATCH,) + shares[0]),
        "patch %d, %d of %d patches accepted" % ((PATCH,) + shares[1]))
    for name, rows in ((names[0], acc), (names[1], rej), ("one sweep of all rungs", sweep)):
        dev, wall = np.median([r[0] for r in rows]), np.median([r[1] for r in rows])
        report("%dx%dx%d x %d rungs, %d pair(s) proposed  %-40s %10.1f us on the device  %10.1f us wall clock"
               % (W, H, D, R, pairs, name, dev, wall))
    if not PATCH:
        report("    (an accepted round reads and writes %.1f MB of residuals and parameters; the energies read %.1f MB)"
               % (moved, R * 2 * H * W * ((D + 1) // 2 * 2) * 8 / 1e6))


for shape in SHAPES:
    measure(*shape)
if PATCH:
    with open(os.path.join(ROOT, "profiles", "patch_time.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
