"""Cost of the region posteriors kept on the device (d3d_region_*, d3d_region.hip) on one GPU:

    python tools/region_time.py [shape=D,H,W]

At 300x300x128 (the bench's config 3: Moffat 11x11, 17-tap LSF), us per d3d_post_accumulate -- one
accumulated sample -- with the map's moments alone (d3d_post_begin(0): no forward model, k_post_accum
touches the map only, so nothing hides the regions' launches), for three label layouts: one region
over the field (K = 1), 8 annuli, and 10 x 10 blocks (K = 900), each without and with the spectra.
The difference to the row without regions is what a region sample costs.  Beside them, from the same
run: the row without regions twice (their spread is what "equal" can mean on this box), one sample of
the clean cube's moments (k_post_accum over the cube: the same exp work as the spectra's first
stage), one sample of both cubes' moments, and one MH sweep.

HIP events on the context's stream after a warm-up; every figure is the median of 7 batches of 20
(tools/posterior_time.py's method).  profiles/region_time.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
D, H, W = (int(v) for v in args.get("shape", "128,300,300").split(","))


def median_us(eng, call, per_batch=20, batches=7, warm=3):
    for _ in range(warm):
        call()
    eng.sync()
    out = []
    for _ in range(batches):
        eng.timer_start()
        for _ in range(per_batch):
            call()
        out.append(eng.timer_stop() / per_batch)
    return float(np.median(out)) * 1e3


def main():
    import bench as B
    from deconv3d_amd import _lib, regions
    fsf, lsf = B.build_taps(D, 11)
    layouts = [("K = 1", np.ones((H, W), dtype=np.int32)),
               ("8 annuli", regions.annuli((H, W), ((H - 1) / 2., (W - 1) / 2.),
                                           np.linspace(0., min(H, W) / 2., 9), pa=30., inclination=50.)),
               ("10x10 blocks", regions.blocks((H, W), 10))]
    print("# tools/region_time.py on one MI355X (default build; HIP events, median of 7 batches of 20)")
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
        eng.set_data(data, var)
        eng.set_params(init)
        eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=12345, refresh_every=0)
        eng.residual(fetch=False)

        def line(what, us, base=None):
            more = "" if base is None else "   (+%.2f us)" % (us - base)
            print("%dx%dx%d %-58s %9.2f us%s" % (W, H, D, what, us, more), flush=True)

        sweep = [0]

        def one_sweep():
            sweep[0] += 1
            eng.mh_sweeps(1, sweep[0])
        line("one MH sweep", median_us(eng, one_sweep, per_batch=5))
        eng.set_params(init)
        for what, label in ((3, "both cubes' moments, no regions"), (1, "the clean cube's moments, no regions")):
            eng.post_begin(what)
            line("one sample of " + label, median_us(eng, eng.post_accumulate))
        eng.post_begin(0)
        base = median_us(eng, eng.post_accumulate)
        line("one sample of the map's moments alone, no regions", base)
        line("one sample of the map's moments alone, no regions, again", median_us(eng, eng.post_accumulate))
        for name, labels in layouts:
            K = int(labels.max())
            for spectra in (False, True):
                eng.region_begin(labels, K, capacity=200, spectra=spectra)      # (the series never fills here)
                us = median_us(eng, eng.post_accumulate)
                sizes = eng.region_get()[3]
                line("  + regions: %s (%d members), %s" % (name, int(sizes.sum()), "with spectra" if spectra else "scalars only"),
                     us, base)
                eng.region_end()
        line("one sample of the map's moments alone, no regions, after", median_us(eng, eng.post_accumulate))


if __name__ == "__main__":
    main()
