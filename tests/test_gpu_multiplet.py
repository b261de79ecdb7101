"""
GPU tests of the multiplet line model (GaussianMultipletLineModel, d3d_set_line_shape): every
line build of the device -- forward model, simulate, window statistics, the MH kernels of every
depth class, the residual refresh, Run with one or R chains, checkpoints -- against the oracle
with its line patched to the multiplet (every oracle function builds its lines through
O.gaussian_line), with K = 2 and K = 3 shapes, one of which reaches past the cube's edge.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests.cases import ALL_CASES, make_case

pytestmark = pytest.mark.gpu

CUBE_RTOL = 1e-12
SHAPES = {
    "doublet": ([0., 3.8], [1., 1.4]),                      # [OII]-like
    "triplet": ([0., -14.5, 15.2], [1., 0.34, 0.11]),       # Halpha + [NII]-like: past the edge of short cubes
}
# K = 4 (LINE_KMAX, the last unrolled component): one component with ratio 0, one that leaves
# short cubes on the low side and one on the high side (tests/test_gpu_multiplet_variants.py)
QUAD = ([0., 2.5, -6.0, 11.25], [1., 0.0, 2.5, 0.3])


def multiplet(offsets, ratios):
    """The oracle's line, a * sum_k r_k exp(-((x - c) - d_k)^2 / (2 w^2))."""
    def line(x, a, c, w):
        x = np.asarray(x, dtype=np.float64)
        s = 0.
        for d, r in zip(offsets, ratios):
            s = s + r * np.exp(-1. * ((x - c) - d) ** 2 / (2. * w ** 2))
        return a * s
    return line


def engine_for(case, shape, options=None):
    eng = _lib.Engine((case["D"], case["H"], case["W"]), case["fsf"].shape, options=options)
    eng.set_taps(case["fsf"], case["lsf"])
    eng.set_data(case["data"], case["var"], mask=case["mask"])
    eng.set_line_shape(*SHAPES[shape])
    return eng


def assert_cube_close(a, b, what, rtol=CUBE_RTOL):
    scale = max(np.max(np.abs(b)), 1e-300)
    err = np.max(np.abs(a - b))
    assert err <= rtol * scale, "%s: max|d|=%g vs scale %g" % (what, err, scale)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", ALL_CASES)
def test_forward_and_simulate_match_the_multiplet_oracle(name, shape, monkeypatch):
    case = make_case(name)
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES[shape]))
    dims = (case["D"], case["H"], case["W"])
    with engine_for(case, shape) as eng:
        eng.set_params(case["truth"])
        ref = O.forward_full(dims, case["truth"], case["mask"], case["fsf"], case["lsf"])
        assert_cube_close(eng.forward(), ref, "forward")
        clean = eng.simulate(case["init"], convolved=False)
        assert_cube_close(clean, O.simulate_clean(dims, case["init"], case["mask"]), "simulate clean")
        conv = eng.simulate(case["init"], convolved=True)
        assert_cube_close(conv, O.forward_full(dims, case["init"], case["mask"], case["fsf"], case["lsf"]),
                          "simulate convolved")
        eng.set_params(case["init"])
        ref_err = O.compute_error_in_one_step(case["data"], case["init"], case["mask"], case["fsf"], case["lsf"])
        assert_cube_close(eng.residual(), ref_err, "residual")
        # back to one Gaussian: the default context's cube, bit for bit
        eng.set_line_shape([0.], [1.])
        single = eng.simulate(case["init"], convolved=True)
    with _lib.Engine(dims, case["fsf"].shape) as ref_eng:
        ref_eng.set_taps(case["fsf"], case["lsf"])
        ref_eng.set_data(case["data"], case["var"], mask=case["mask"])
        np.testing.assert_array_equal(single, ref_eng.simulate(case["init"], convolved=True))
    if case["D"] >= 16:      # (the 2-channel cube sees no second component)
        assert not np.allclose(single, conv)


@pytest.mark.parametrize("name", ALL_CASES)
def test_window_stats_probe(name, monkeypatch):
    case = make_case(name)
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES["doublet"]))
    rng = case["rng"]
    H, W = case["H"], case["W"]
    with engine_for(case, "doublet") as eng:
        eng.set_params(case["init"])
        err = eng.residual()
        spaxels = [(0, 0), (H - 1, W - 1), (0, W - 1), (H // 2, W // 2)]
        spaxels += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(6)]
        for (y, x) in spaxels:
            p_old = case["init"][y, x]
            p_new = p_old + np.array([0., 1., 0.3]) * np.tan(np.pi * (rng.random(3) - 0.5)) * 0.5
            p_new[2] = abs(p_new[2]) + 0.2
            got = eng.window_stats(y, x, p_new)
            ref = O.window_stats(err, case["var"], p_old, p_new, y, x, case["fsf"], case["lsf"])
            floor = 1e-12 * max(ref[0], ref[1])
            np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-10, atol=floor, err_msg="chi2 at %s" % ((y, x),))
            np.testing.assert_allclose(got[3:], ref[3:], rtol=1e-10, atol=1e-12 * max(abs(ref[3]), abs(ref[4])),
                                       err_msg="gibbs moments at %s" % ((y, x),))


def chain_against_oracle(eng, data, var, mask, fsf, lsf, init, min_b, max_b, n_sweeps, seed):
    st = O.MHState(data, var, mask, fsf, lsf, init, min_b, max_b, jump_amplitude=0.1, seed=seed)
    H, W = mask.shape
    eng.set_params(init)
    eng.mh_config(min_b, max_b, 0.1, st.ra, seed=seed, refresh_every=0)
    chain = np.full((n_sweeps + 1, H, W, 3), np.nan)
    dlog = np.full((n_sweeps + 1, H, W), np.nan)
    accepted = eng.mh_sweeps(n_sweeps, 1, 1, chain, dlog)
    err_dev = eng.download_slot(_lib.SLOT_ERR)
    live = mask == 1
    for s in range(1, n_sweeps + 1):
        O.mh_sweep(st, s)
        np.testing.assert_allclose(chain[s][live], st.params[live], rtol=1e-9, atol=1e-9,
                                   err_msg="params after sweep %d" % s)
        scale = np.max(np.abs(st.dlog[live])) + 1.0
        np.testing.assert_allclose(dlog[s][live], st.dlog[live], rtol=1e-8, atol=1e-10 * scale,
                                   err_msg="dlog sweep %d" % s)
    assert accepted == st.accepted
    assert np.max(np.abs(err_dev - st.err)) <= 1e-11 * np.max(np.abs(st.err)), "carried residual"


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", ["c1", "odd_depth", "asym", "nolsf", "rect_fsf", "tiny", "uniform"])
def test_mh_chain_matches_the_multiplet_oracle_update_by_update(name, shape, monkeypatch):
    """"uniform": c1 with one constant variance (the uniform-variance kernels)."""
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES[shape]))
    case = make_case("c1" if name == "uniform" else name)
    if name == "uniform":
        case["var"] = np.full(case["var"].shape, float(np.median(case["var"])))
    with engine_for(case, shape) as eng:
        if name == "uniform":
            assert eng.variance_is_uniform()
        chain_against_oracle(eng, case["data"], case["var"], case["mask"], case["fsf"], case["lsf"],
                             case["init"], case["min_b"], case["max_b"], 3, 777)


@pytest.mark.parametrize("D,lsf_kind", [(128, "gauss"), (256, "gauss"), (300, "gauss"), (512, "gauss"),
                                        (600, "muse"), (1025, "muse")])
def test_every_default_mh_kernel_depth_matches_the_multiplet_oracle(D, lsf_kind, monkeypatch):
    """Depths that select each default MH kernel (as test_deep_cubes_chain_matches_oracle):
    k_mh_ws with 256 / 512 streaming threads, the z-blocked form beyond 512 channels with
    the MUSE-like LSF, the thread-looped deep kernels beyond 1024."""
    monkeypatch.setattr(O, "gaussian_line", multiplet(*SHAPES["triplet"]))
    depth_chain_against_oracle(D, lsf_kind, SHAPES["triplet"])


def depth_chain_against_oracle(D, lsf_kind, line_shape, lsf_fits=None):
    """The 5 x 6 problem of test_deep_cubes_chain_matches_oracle at depth D with the line shape
    (the caller has patched the oracle's line to it): forward model and two sweeps against the
    oracle.  lsf_fits: the value option lsf_fits must report (0: the taps do not fit +-8
    channels, so the plain deferred / thread-looped kernels run beyond 512 channels)."""
    off, rat = line_shape
    H, W = 5, 6
    fsf = O.gaussian_fsf_image(1.6)
    lsf = O.gaussian_lsf_vector(D, 1.1) if lsf_kind == "gauss" else O.muse_like_lsf(D)
    rng = np.random.default_rng(D)
    truth = np.dstack((1 + 5 * rng.random((H, W)), D * (0.3 + 0.4 * rng.random((H, W))),
                       1.0 + 2 * rng.random((H, W))))
    mask = np.ones((H, W))
    clean = O.forward_full((D, H, W), truth, mask, fsf, lsf)
    sigma = 0.05 * clean.max()
    data = clean + rng.normal(0, sigma, clean.shape)
    var = np.full(clean.shape, sigma ** 2)
    min_b = O.model_min_boundaries()
    max_b = O.model_max_boundaries(data, fsf)
    init = min_b + (max_b - min_b) * rng.random((H, W, 3))
    init[..., 2] = np.maximum(init[..., 2], 0.5)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        if lsf_fits is not None:
            assert eng.get_option("lsf_fits") == lsf_fits
        eng.set_data(data, var, mask=mask)
        eng.set_line_shape(off, rat)
        eng.set_params(truth)
        assert_cube_close(eng.forward(), clean, "forward")
        chain_against_oracle(eng, data, var, mask, fsf, lsf, init, min_b, max_b, 2, 3)


def test_full_size_sweep_matches_the_multiplet_oracle(monkeypatch):
    """One whole sweep of the bench's config-3 shape, 300x300x128 (Moffat 11x11, 17-tap LSF, default
    kernel selection), K = 2, update by update against the oracle fed the device's initial residual."""
    import bench as B
    off, rat = SHAPES["doublet"]
    monkeypatch.setattr(O, "gaussian_line", multiplet(off, rat))
    D, H, W = 128, 300, 300
    fsf, lsf = B.build_taps(D, 11)
    with _lib.Engine((D, H, W), fsf.shape) as eng:
        eng.set_taps(fsf, lsf)
        eng.set_line_shape(off, rat)
        data, var, truth, init, min_b, max_b = B.synthetic_inputs(eng, D, H, W, fsf, 12345)
        mask = np.ones((H, W))
        mask[17, 200] = mask[H // 2, W // 2] = 0
        eng.set_data(data, var, mask=mask)
        ra = float(max_b[0] ** 2)
        eng.set_params(init)
        eng.mh_config(min_b, max_b, 0.1, ra, seed=12345, refresh_every=0)
        err0 = eng.residual()
        st = O.MHState(data, var, mask, fsf, lsf, init, min_b, max_b, 0.1, ra, 12345, err=err0)
        accepted = eng.mh_sweeps(1, 1)
        O.mh_sweep(st, 1)
        live = mask == 1
        np.testing.assert_allclose(eng.get_params()[live], st.params[live], rtol=1e-9, atol=1e-9)
        assert accepted == st.accepted
        err = eng.download_slot(_lib.SLOT_ERR)
        assert np.max(np.abs(err - st.err)) <= 1e-11 * np.max(np.abs(st.err))


def test_residual_refresh_builds_the_multiplet(monkeypatch):
    """refresh_every = 2 over 6 sweeps: the residual rebuilt from scratch after sweep 6 is
    data - forward(multiplet) -- a refresh that ignored the shape would leave single Gaussians."""
    off, rat = SHAPES["doublet"]
    monkeypatch.setattr(O, "gaussian_line", multiplet(off, rat))
    case = make_case("c1")
    with engine_for(case, "doublet") as eng:
        eng.set_params(case["init"])
        eng.mh_config(case["min_b"], case["max_b"], 0.1, 50.0, seed=9, refresh_every=2)
        eng.mh_sweeps(6, 1)
        err = eng.download_slot(_lib.SLOT_ERR)
        want = case["data"] - O.forward_full((case["D"], case["H"], case["W"]), eng.get_params(), case["mask"],
                                             case["fsf"], case["lsf"])
    assert np.max(np.abs(err - want)) <= 1e-11 * np.max(np.abs(want))


def run_inputs(D, H, W, offsets, ratios, seed, noise=0.05, fsf=None):
    """A Run()-ready cube built by the (patched-free) multiplet oracle: Moffat FSF, 17-tap LSF."""
    fsf = O.moffat_cropped(11, 3.0, 2.5) if fsf is None else fsf
    lsf = O.muse_like_lsf(D)
    rng = np.random.default_rng(seed)
    y, x = np.indices((H, W))
    r2 = (y - H / 2.) ** 2 + (x - W / 2.) ** 2
    truth = np.dstack((10. * np.exp(-r2 / (2. * (H / 4.) ** 2)) + 0.5,
                       D / 2.5 + 2. * np.tanh((x - W / 2.) / (W / 4.)),
                       rng.uniform(1.4, 2.2, size=(H, W))))
    clean = np.zeros((D, H, W))
    line = multiplet(offsets, ratios)
    for (yy, xx) in zip(y.ravel(), x.ravel()):
        clean[:, yy, xx] = O.spectral_convolve(line(np.arange(D), *truth[yy, xx]), lsf)
    clean = O.spatial_convolve(clean, fsf)
    sigma = noise * clean.max()
    data = clean + rng.normal(0., sigma, clean.shape)
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    cube = d3d.MUSE().build_cube(data)
    return inst, cube, np.full(data.shape, sigma ** 2), truth


@pytest.mark.parametrize("chains", [1, 4])
@pytest.mark.parametrize("shape", [(32, 16, 16), (64, 64, 64)])
def test_one_component_run_is_the_single_gaussian_run_bit_for_bit(shape, chains):
    inst, cube, var, _ = run_inputs(*shape, [0.], [1.], seed=5)
    kw = dict(variance=var, max_iterations=5, seed=7, chains=chains, min_acceptance_rate=0.)
    one = d3d.Run(cube, inst, model=d3d.SingleGaussianLineModel, **kw)
    multi = d3d.Run(cube, inst, model=d3d.GaussianMultipletLineModel([0], [1]), **kw)
    assert not multi._host_model
    for r in range(chains):
        np.testing.assert_array_equal(multi.chains[r], one.chains[r])
        np.testing.assert_array_equal(multi.all_likelihoods[r], one.all_likelihoods[r])
    np.testing.assert_array_equal(multi.parameters, one.parameters)
    np.testing.assert_array_equal(multi.convolved_cube.data, one.convolved_cube.data)
    np.testing.assert_array_equal(multi.clean_cube.data, one.clean_cube.data)


@pytest.mark.parametrize("batched", [True, False])
def test_doublet_chains_are_the_single_runs_of_their_seeds(batched):
    off, rat = SHAPES["doublet"]
    inst, cube, var, _ = run_inputs(32, 12, 12, off, rat, seed=6)
    model = d3d.GaussianMultipletLineModel(off, rat)
    kw = dict(variance=var, max_iterations=7, keep_one_in=2, min_acceptance_rate=0., model=model)

    class Threads(d3d.Run):
        _batched = False

    multi = (d3d.Run if batched else Threads)(cube, inst, seed=11, chains=3, **kw)
    for r in range(3):
        one = d3d.Run(cube, inst, seed=11 + r, **kw)
        np.testing.assert_array_equal(multi.chains[r], one.chain)
        np.testing.assert_array_equal(multi.all_likelihoods[r][1:], one.likelihoods[1:])


def test_doublet_checkpoint_and_resume(tmp_path, monkeypatch):
    off, rat = SHAPES["doublet"]
    inst, cube, var, _ = run_inputs(32, 12, 12, off, rat, seed=7)
    model = d3d.GaussianMultipletLineModel(off, rat)
    name = str(tmp_path / "ck")
    kw = dict(variance=var, seed=3, min_acceptance_rate=0., refresh_every=0, model=model)
    whole = d3d.Run(cube, inst, max_iterations=13, **kw)
    first = d3d.Run(cube, inst, max_iterations=7, write_every=7, checkpoint=name, **kw)
    state = np.load(name + "_state.npz")
    np.testing.assert_array_equal(state["line_offsets"], off)
    np.testing.assert_array_equal(state["line_ratios"], rat)
    second = d3d.Run(cube, inst, max_iterations=7, initial_parameters=name + "_parameters.npy",
                     resume_state=name + "_state.npz", **kw)
    np.testing.assert_array_equal(first.chain[-1], np.load(name + "_parameters.npy"))
    # (the resumed run rebuilds the residual from the parameters: rounding-level differences)
    np.testing.assert_allclose(second.chain[-1], whole.chain[-1], rtol=1e-8, atol=1e-8)
    # the same checkpoint with another line shape -- or the single Gaussian's -- is refused
    for other in (d3d.GaussianMultipletLineModel([0., 3.9], [1., 1.4]), d3d.SingleGaussianLineModel()):
        kw2 = dict(kw, model=other)
        with pytest.raises(ValueError, match="line shape"):
            d3d.Run(cube, inst, max_iterations=3, initial_parameters=name + "_parameters.npy",
                    resume_state=name + "_state.npz", **kw2)
    # a checkpoint without a line shape (older runs) is a single Gaussian's
    legacy = {k: state[k] for k in state.files if not k.startswith("line_")}
    np.savez(name + "_legacy_state.npz", **legacy)
    with pytest.raises(ValueError, match="line shape"):
        d3d.Run(cube, inst, max_iterations=3, initial_parameters=name + "_parameters.npy",
                resume_state=name + "_legacy_state.npz", **kw)
    d3d.Run(cube, inst, max_iterations=3, initial_parameters=name + "_parameters.npy",
            resume_state=name + "_legacy_state.npz", **dict(kw, model=d3d.SingleGaussianLineModel))



def test_contribution_of_spaxel_matches_the_multiplet_oracle(monkeypatch):
    """Run.contribution_of_spaxel with the doublet: a corner, an edge and an interior spaxel,
    one whose second line lies past the last channel, against the patched oracle."""
    off, rat = SHAPES["doublet"]
    inst, cube, var, truth = run_inputs(32, 12, 12, off, rat, seed=9)
    run = d3d.Run(cube, inst, variance=var, model=d3d.GaussianMultipletLineModel(off, rat), max_iterations=2)
    monkeypatch.setattr(O, "gaussian_line", multiplet(off, rat))
    for (y, x), p in [((0, 0), truth[0, 0]), ((11, 5), truth[11, 5]), ((6, 6), truth[6, 6]),
                      ((3, 9), np.array([4.0, 30.5, 1.2]))]:
        got, _ = run.contribution_of_spaxel(x, y, p, 12, 12, 32)
        want = O.contribution_of_spaxel(x, y, p, 12, 12, 32, run.fsf, run.lsf)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (y, x)
    sim = run.simulate_convolved(cube.data.shape, truth)
    want = O.forward_full(cube.data.shape, truth, np.ones((12, 12)), run.fsf, run.lsf)
    assert_cube_close(sim, want, "simulate_convolved")


def test_oii_science_check():
    """A synthetic [OII]-like cube (K = 2, 3.79 channels apart, ratio 1.4; 17-tap LSF, a compact
    Gaussian FSF, 2 % noise) fitted from a start 0.3 channel and 15 % off: the multiplet's posterior
    median centre and width of the bright spaxels lie within 0.2 channel of the truth, and its last
    sample fits the cube to the noise while the single Gaussian's does not.  (With the 11x11 Moffat
    FSF neighbouring spaxels trade flux -- a spaxel may switch its line off and leave it to its
    neighbours, which also lets single Gaussians mimic a doublet -- so per-spaxel truth recovery
    is not a property of that geometry: DESIGN.md, "Multiplet line model".)"""
    blank = d3d.MUSE().build_cube(np.zeros((64, 14, 14)))
    oii = d3d.GaussianMultipletLineModel.from_rest_wavelengths(blank, [0.372603, 0.372882], [1.0, 1.4], 0.7)
    assert abs(oii.offsets[1] - 3.79) < 0.01
    inst, cube, var, truth = run_inputs(64, 14, 14, oii.offsets, oii.ratios, seed=8, noise=0.02,
                                        fsf=O.gaussian_fsf_image(1.0))
    start = truth.copy()
    start[..., 0] *= 0.8
    start[..., 1] += 0.3
    start[..., 2] *= 1.15
    kw = dict(variance=var, max_iterations=600, seed=21, min_acceptance_rate=0., initial_parameters=start)
    fit = d3d.Run(cube, inst, model=oii, **kw)
    single = d3d.Run(cube, inst, model=d3d.SingleGaussianLineModel, **kw)
    bright = truth[..., 0] > 0.5 * truth[..., 0].max()
    assert bright.sum() >= 20
    post = np.median(fit.chain[-200:], axis=0)
    dc = np.abs(post[..., 1] - truth[..., 1])[bright]
    dw = np.abs(post[..., 2] - truth[..., 2])[bright]
    assert np.median(dc) < 0.2 and np.max(dc) < 0.5, "centre: %s" % np.sort(dc)
    assert np.median(dw) < 0.2 and np.max(dw) < 0.5, "width: %s" % np.sort(dw)

    def chi2(run):
        sim = run.simulate_convolved(cube.data.shape, run.chain[-1])
        return float(np.sum((cube.data - sim) ** 2 / var))

    n = cube.data.size
    assert chi2(fit) < 1.1 * n, chi2(fit)
    assert chi2(single) > chi2(fit) + 0.2 * n, (chi2(single), chi2(fit))
