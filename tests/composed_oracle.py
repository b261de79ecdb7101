"""
The end of a sweep with several features armed (csrc/d3d_sweep.hip: end_sweep), composed from the
restatements the features' own tests use.  It adds no numerics of its own: an update is
tests/prior_oracle.py's mh_update with tests/test_gpu_adapt.py's amplitudes, a Welford step is
tests/predictive_oracle.py's Accum, the histograms are tests/histogram_oracle.py's, the regions
tests/region_oracle.py's, the draws RobustChain.reweight and NoiseChain.rescale.  What it fixes is the
ORDER after sweep s, the contract of DESIGN.md:

  1. the snapshot of the chain (parameters, log ratios);
  2. where the moments' schedule says so, one sample: the (a, c, w, F) map, the clean and the convolved
     cube, the predictive accumulators from the CARRIED residual, the regions, then the histograms'
     freeze (sample number `pilot`) or their counters (later samples);
  3. the sweep is counted and, where it fills a window at or before the last adapted sweep, the jump
     scales take a step and the counters start again;
  4. every `refresh_every` sweeps the residual is rebuilt from the parameters;
  5. where due, the Student-t weights or the noise scales are drawn from the residual of 4 and
     1/variance is rewritten.

A Composed is built from a STATE -- everything the device carries between two sweeps, as a dict (see
fresh_state) -- so that a test can seed it from what a context holds, run one sweep and compare.
Test infrastructure only.
"""
import numpy as np

from oracle import deconv3d_oracle as O
from tests import histogram_oracle as HO
from tests import noise_oracle as NO
from tests import predictive_oracle as PO
from tests import prior_oracle
from tests import region_oracle as RG
from tests import robust_oracle as RB

SINGLE = ((0.,), (1.,))


def problem_of(case, jump=0.1, ra=35.0, seed=77, line=SINGLE):
    """What does not change along the chain, from a case dict (D, H, W, fsf, lsf, data, var, mask, init,
    min_b, max_b): the mask the device runs with (a spaxel with a NaN voxel is masked), the data its
    residual is made from (NaN voxels hold 0) and the base 1/variance."""
    data = np.asarray(case["data"], dtype=np.float64)
    mask = np.array(case["mask"], dtype=np.float64)
    mask[np.isnan(data).any(axis=0)] = 0
    return dict(dims=(case["D"], case["H"], case["W"]), fsf=case["fsf"], lsf=case["lsf"], data=data,
                data0=np.where(np.isnan(data), 0., data), var=case["var"], i0=RB.base_ivar(data, case["var"]),
                mask=mask, init=np.array(case["init"], dtype=np.float64), min_b=np.asarray(case["min_b"], dtype=np.float64),
                max_b=np.asarray(case["max_b"], dtype=np.float64), jump=jump, ra=ra, seed=seed, line=line,
                flux_k=HO.flux_factor(line[1]))


def features_of(lam=(0., 0., 0.), adapt=None, robust=None, noise=None, post=None, hist=None, regions=None,
                pred=False, refresh_every=0):
    """The armed features.  ``adapt``: dict(target, window, last, gain, range); ``robust``: dict(nu, every,
    start, accumulate_from); ``noise``: dict(group, every, start, shape, rate, spaxels); ``post``:
    dict(first, every, cubes); ``hist``: dict(pilot, span); ``regions``: dict(labels, K, spectra)."""
    assert not (robust and noise), "one holder of SLOT_IVAR"
    assert post is not None or not (hist or regions or pred), "histograms, regions and predictive hang on the moments"
    return dict(lam=np.asarray(lam, dtype=np.float64), adapt=adapt, robust=robust, noise=noise, post=post,
                hist=hist, regions=regions, pred=pred, refresh_every=refresh_every)


def fresh_state(pb, ft):
    """The state of a context that has just been configured: the start map and its residual, the base
    1/variance, scales of 1, every accumulator empty."""
    D, H, W = pb["dims"]
    state = dict(params=pb["init"].copy(),
                 err=pb["data0"] - O.forward_full(pb["dims"], pb["init"], pb["mask"], pb["fsf"], pb["lsf"]),
                 ivar=pb["i0"].copy(), scale=np.ones((H, W)), acc=np.zeros((H, W), dtype=np.int64), n_win=0, k=0)
    if ft["post"]:
        cube = (np.zeros((D, H, W)), np.zeros((D, H, W)))
        state["post"] = dict(n=0, map=(np.zeros((H, W, 4)), np.zeros((H, W, 4))),
                             clean=cube if ft["post"].get("cubes", True) else None,
                             conv=tuple(c.copy() for c in cube) if ft["post"].get("cubes", True) else None)
    if ft["hist"]:
        state["hist"] = dict(bins=np.zeros((H, W, 4, HO.BINS), dtype=np.uint32), tails=np.zeros((H, W, 4, 2), dtype=np.uint32),
                             range=np.full((H, W, 4, 2), np.nan))
    if ft["regions"]:
        K = ft["regions"]["K"]
        state["regions"] = dict(spec=(np.zeros((K, D)), np.zeros((K, D))) if ft["regions"].get("spectra", True) else None)
    if ft["pred"]:
        state["pred"] = tuple(np.zeros((D, H, W)) for _ in range(4))
    if ft["robust"]:
        state["robust"] = dict(mean=np.zeros((D, H, W)), count=0)
    if ft["noise"]:
        state["tau_g"] = np.ones(int(np.max(ft["noise"]["group"])) + 1)
    return state


def welford_step(n_before, mean, m2, sample):
    """(mean, M2) after sample number n_before + 1: the recurrence of predictive_oracle.Accum."""
    acc = PO.Accum(np.shape(sample))
    acc.n, acc.mean, acc.m2 = int(n_before), np.array(mean, dtype=np.float64), np.array(m2, dtype=np.float64)
    acc.add(sample)
    return acc.mean, acc.m2


class Composed(object):
    """One chain with the features of ``ft`` on the problem ``pb``, from ``state`` (default: fresh)."""

    def __init__(self, pb, ft, state=None, draw_before_refresh=False):
        self.pb, self.ft = pb, ft
        self.draw_before_refresh = draw_before_refresh      # the mistake the order rules out (tests only)
        state = fresh_state(pb, ft) if state is None else state
        # (the chain classes take the base 1/variance from the state they are made on)
        st = O.MHState(pb["data"], pb["var"], pb["mask"], pb["fsf"], pb["lsf"], state["params"], pb["min_b"],
                       pb["max_b"], pb["jump"], pb["ra"], pb["seed"], err=state["err"])
        self.robust = self.noise = None
        if ft["robust"]:
            r = ft["robust"]
            self.robust = RB.RobustChain(st, r["nu"], r["every"], r["start"], r["accumulate_from"])
            self.robust.mean = np.nan_to_num(np.array(state["robust"]["mean"], dtype=np.float64))
            self.robust.count = int(state["robust"]["count"])
        if ft["noise"]:
            n = ft["noise"]
            self.noise = NO.NoiseChain(st, n["group"], n["every"], n["start"], n["shape"], n["rate"], n["spaxels"])
            self.noise.tau_g = np.array(state["tau_g"], dtype=np.float64)
        st.data = pb["data0"]
        with np.errstate(divide="ignore"):
            st.var = 1.0 / np.asarray(state["ivar"], dtype=np.float64)     # (inf where the voxel carries nothing)
        self.st = st
        self.scale = np.array(state["scale"], dtype=np.float64)
        self.acc = np.array(state["acc"], dtype=np.int64)
        self.n_win, self.k = int(state["n_win"]), int(state["k"])
        self.ivar = np.array(state["ivar"], dtype=np.float64)
        self.post = self.hist = self.spec = self.pred = None
        self.rows = []                       # the regions' (F, C, S) of the samples taken since the state
        if ft["post"]:
            p = state["post"]
            self.post = dict(n=int(p["n"]), map=p["map"], clean=p.get("clean"), conv=p.get("conv"))
        if ft["hist"]:
            self.hist = dict((k, np.array(v)) for k, v in state["hist"].items())
        if ft["regions"]:
            self.spec = state["regions"]["spec"]
        if ft["pred"]:
            self.pred = PO.Accum(pb["i0"].shape)
            self.pred.n = self.post["n"]
            self.pred.M, self.pred.S, self.pred.mean, self.pred.m2 = (np.array(a, dtype=np.float64) for a in state["pred"])
        self.chain, self.dlog, self.counts = {}, {}, None

    def state(self):
        """The state now: what another Composed can be made from."""
        out = dict(params=self.st.params.copy(), err=self.st.err.copy(), ivar=self.ivar.copy(), scale=self.scale.copy(),
                   acc=self.acc.copy(), n_win=self.n_win, k=self.k)
        if self.post:
            out["post"] = dict(self.post)
        if self.hist:
            out["hist"] = dict((k, v.copy()) for k, v in self.hist.items())
        if self.ft["regions"]:
            out["regions"] = dict(spec=self.spec)
        if self.pred:
            out["pred"] = (self.pred.M, self.pred.S, self.pred.mean, self.pred.m2)
        if self.robust:
            out["robust"] = dict(mean=self.robust.mean.copy(), count=self.robust.count)
        if self.noise:
            out["tau_g"] = self.noise.tau_g.copy()
        return out

    # ---- the sweep ---------------------------------------------------------------------------------
    def updates(self, s):
        """The updates of sweep s in the device's colour order, every spaxel with its own jump scale;
        ``counts`` takes the accepted proposals per spaxel."""
        st, jump = self.st, self.pb["jump"]
        self.counts = np.zeros(st.mask.shape, dtype=np.int64)
        for (y, x) in O.colour_order(st.mask, *st.fsf.shape):
            st.amp = np.ones(3) * np.asarray(jump) * self.scale[y, x]      # (0.1 s, as tests/test_gpu_adapt.py)
            st.amp[0] = 0.
            self.counts[y, x] += bool(prior_oracle.mh_update(st, y, x, s, self.ft["lam"]))
        self.acc = self.acc + self.counts

    def sweep(self, s, device=None):
        self.updates(s)
        self.end_of_sweep(s, device)

    # ---- what follows it ----------------------------------------------------------------------------
    def post_due(self, s):
        p = self.ft["post"]
        return bool(p) and s >= p["first"] and (s - p["first"]) % p["every"] == 0

    def refresh_due(self, s):
        return self.ft["refresh_every"] > 0 and s % self.ft["refresh_every"] == 0

    def rescale_due(self, s):
        r = self.ft["robust"] or self.ft["noise"]
        return bool(r) and s >= r["start"] and (s - r["start"]) % r["every"] == 0

    def end_of_sweep(self, s, device=None):
        """Steps 1 to 5 after sweep s.  ``device``: dict(params, err) downloaded from a context AFTER its
        own step, for the quantities a test compares bit for bit: the samples are then taken from the
        device's parameters (the end of a sweep does not change them), the draw from the device's
        residual, and so is the predictive sample where no refresh came between the two."""
        st, pb = self.st, self.pb
        self.chain[s], self.dlog[s] = st.params.copy(), st.dlog.copy()                      # 1
        if self.post_due(s):                                                                # 2
            carried = st.err if (device is None or self.refresh_due(s)) else device["err"]
            self.sample(st.params if device is None else device["params"], carried)
        self.adapt_step(s)                                                                  # 3
        if self.draw_before_refresh:
            self.draw(s, None)
        if self.refresh_due(s):                                                             # 4
            st.err = pb["data0"] - O.forward_full(pb["dims"], st.params, st.mask, st.fsf, st.lsf)
        if not self.draw_before_refresh:
            self.draw(s, device)                                                            # 5

    def sample(self, params, carried):
        pb, ft, post = self.pb, self.ft, self.post
        n = post["n"]
        post["map"] = welford_step(n, *post["map"], HO.series(params, pb["flux_k"]))
        if post["clean"] is not None:
            assert pb["line"] == SINGLE, "the oracle's cubes are the single Gaussian's"
            post["clean"] = welford_step(n, *post["clean"], O.simulate_clean(pb["dims"], params, pb["mask"]))
            post["conv"] = welford_step(n, *post["conv"], O.forward_full(pb["dims"], params, pb["mask"], pb["fsf"], pb["lsf"]))
        if self.pred:
            nu = ft["robust"]["nu"] if ft["robust"] else 0
            self.pred.add(PO.q_of(carried, pb["i0"], nu), pb["i0"] != 0.)
        if ft["regions"]:
            r = ft["regions"]
            self.rows.append(RG.scalars(params, r["labels"], pb["mask"], r["K"], pb["flux_k"]))
            if self.spec is not None:
                one = RG.spectra(params, r["labels"], pb["mask"], r["K"], pb["dims"][0], RG.gaussian_unit_line(*pb["line"]))
                self.spec = welford_step(n, *self.spec, one)
        post["n"] = n + 1
        if self.hist:
            h, pilot = self.hist, ft["hist"]["pilot"]
            if post["n"] == pilot:
                L, U = HO.bounds(pb["min_b"], pb["max_b"], pb["flux_k"])
                lo, hi = HO.freeze(post["map"][0], post["map"][1], pilot, ft["hist"]["span"], L, U, pb["mask"])
                h["range"] = np.stack((lo, hi), axis=-1)
            elif post["n"] > pilot:
                bins, tails = HO.count(HO.series(params, pb["flux_k"])[None], h["range"][..., 0], h["range"][..., 1])
                h["bins"], h["tails"] = h["bins"] + bins, h["tails"] + tails

    def adapt_step(self, s):
        """tests/test_gpu_adapt.py: test_the_rule_window_by_window_against_numpy_and_the_oracle."""
        a = self.ft["adapt"]
        if not a:
            return
        self.n_win += 1
        if a["window"] <= 0 or self.n_win != a["window"] or s > a["last"]:
            return
        self.k += 1
        want = np.clip(self.scale * np.exp(a["gain"] / np.sqrt(self.k) * (self.acc / float(a["window"]) - a["target"])),
                       *a["range"])
        live = self.pb["mask"] == 1
        self.scale = np.where(live, want, self.scale)
        self.acc = np.where(live, 0, self.acc)
        self.n_win = 0

    def draw(self, s, device):
        if not self.rescale_due(s):
            return
        if device is not None:
            self.st.err = np.array(device["err"], dtype=np.float64)
        self.ivar = self.robust.reweight(s) if self.robust else self.noise.rescale(s)


# ---- at the Run level (tests/test_gpu_robust.py, tests/test_gpu_noise.py) ------------------------------

def run_outputs(run):
    """name -> array: every output of a Run with adaptation, moments, histograms, regions and robust= or
    noise=, for a comparison of two runs bit for bit."""
    p, h, r = run.posterior, run.posterior.histograms, run.posterior.regions
    out = dict(chain=run.chain, likelihoods=run.likelihoods, parameters=run.parameters, jump_scale=run.jump_scale,
               acceptance_map=run.acceptance_map, adapted_until=run.adapted_until, post_count=p.count,
               parameters_mean=p.parameters_mean, parameters_std=p.parameters_std, flux_mean=p.flux_mean,
               flux_std=p.flux_std, clean_mean=p.clean_mean, clean_std=p.clean_std, convolved_mean=p.convolved_mean,
               convolved_std=p.convolved_std, hist_count=h.count, hist_counts=h.counts, hist_tails=h.tails,
               hist_range=h.range, hist_median=h.median, hist_mode=h.mode, hist_outside=h.outside,
               region_series=r.series, region_sizes=r.sizes, region_spectrum_mean=r.spectrum_mean,
               region_spectrum_std=r.spectrum_std, residual=run.engine.download_slot(2),
               ivar=run.engine.download_slot(1))
    if run.robust is not None:
        out.update(robust_count=run.robust.count, robust_weights=run.robust.weights,
                   robust_weight_mean=run.robust.weight_mean)
    if run.noise is not None:
        out.update(noise_scale=run.noise.scale, noise_sweeps=run.noise.sweeps, noise_voxels=run.noise.voxels,
                   noise_last_sum=run.noise.last_sum, noise_channel_scale=run.noise.channel_scale)
    return dict((k, np.asarray(v)) for k, v in out.items())


def chain_of_run(run, data, var, fsf, lsf, ft, n_sweeps):
    """The first ``n_sweeps`` sweeps of a single-chain Run from its own start ``run.chain[0]``, with the
    features ``ft``: the oracle's chain (n_sweeps + 1, H, W, 3) and the Composed after it."""
    D, H, W = data.shape
    case = dict(D=D, H=H, W=W, fsf=fsf, lsf=lsf, data=data, var=var, mask=np.asarray(run.mask, dtype=np.float64),
                init=run.chain[0], min_b=run.min_boundaries, max_b=run.max_boundaries)
    pb = problem_of(case, run.jumping_amplitude, run.gibbs_apriori_variance, run.seed)
    co = Composed(pb, ft)
    chain = [run.chain[0].copy()]
    for s in range(1, n_sweeps + 1):
        co.sweep(s)
        chain.append(co.chain[s])
    return np.stack(chain), co
