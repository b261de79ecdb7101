"""
GPU tests of the cube preparation (d3d_running_median, d3d_channel_stats, d3d_prepare,
deconv3d_amd/prepare.py, Run(prepare=)) against its numpy restatement (tests/prepare_oracle.py).

Every device-against-oracle comparison is np.array_equal(..., equal_nan=True): both selections
are exact and the only arithmetic is one subtraction, one * 0.5 and one * 1.4826, so there is
no tolerance (-0.0 == 0.0 holds under ==).
"""
import functools

import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd import _lib
from deconv3d_amd.spread_functions import ImageFieldSpreadFunction, VectorLineSpreadFunction
from oracle import deconv3d_oracle as O
from tests import prepare_oracle as P

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def engine(shape):
    return _lib.Engine(shape, (1, 1))


# ---- running median ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spectra(name):
    """(cube, valid or None, half window) of one comparison; never modified."""
    valid = None
    if name in ("odd", "ties", "whole"):
        # odd depth (the pad channel), 35 spectra of 21 channels: two workgroups, the second
        # partly beyond the cube; scattered NaN and +-inf, one all-NaN spectrum
        rng = np.random.default_rng(1)
        cube = rng.normal(0., 1., (21, 5, 7))
        if name == "ties":
            cube = np.floor(rng.random((21, 5, 7)) * 5.)       # integers 0 .. 4: ties everywhere
        cube[rng.random(cube.shape) < 0.1] = NAN
        cube[3, 1, 2] = cube[20, 4, 6] = INF
        cube[0, 0, 0] = cube[11, 2, 3] = -INF
        cube[8:12, 3, 3] = NAN                                 # a window of h = 1 .. 3 with few values
        cube[:, 2, 5] = NAN
        h = 30 if name == "whole" else 3
    elif name == "valid":
        rng = np.random.default_rng(2)
        cube = rng.normal(0., 1., (64, 9, 8))
        cube[rng.random(cube.shape) < 0.05] = NAN
        valid = (rng.random(cube.shape) < 0.7).astype(np.uint8)
        valid[10:40, 4, 4] = 0                                 # windows without a valid voxel
        h = 8
    elif name == "widest":
        cube = np.random.default_rng(3).normal(0., 1., (130, 3, 5))
        cube[5, 1, 1] = NAN
        h = 128
    elif name == "long":
        cube = np.random.default_rng(4).normal(0., 1., (1030, 2, 3))
        cube[500:560, 1, 1] = NAN
        h = 25
    else:
        raise KeyError(name)
    cube.setflags(write=False)
    return cube, valid, h


@pytest.mark.parametrize("name", ["odd", "ties", "whole", "valid", "widest", "long"])
def test_running_median_equals_nanmedian(name):
    cube, valid, h = spectra(name)
    want = P.running_median(cube, valid, h)
    with engine(cube.shape) as eng:
        got = eng.running_median(cube, h, valid=valid)
    assert same(got, want), "%d voxels differ" % np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))


# ---- channel statistics --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planes(name):
    """(cube, select or None)"""
    rng = np.random.default_rng(5)
    select = None
    if name in ("1", "2", "35", "72"):                          # n < 2, even and odd counts
        shape = {"1": (4, 1, 1), "2": (4, 1, 2), "35": (4, 5, 7), "72": (4, 8, 9)}[name]
        cube = rng.normal(0., 1., shape)
        if cube[0].size > 2:
            cube[1, 0, 0] = NAN                                 # the other parity in one channel
            cube[2, 0, 1] = INF
    elif name == "big":                                         # 4690 values: several passes of a workgroup
        cube = rng.normal(0., 1., (3, 70, 67)) * np.array([1., 1e-3, 1e6])[:, None, None]
        cube[1, 3, 3] = NAN
    elif name == "ties":
        cube = np.floor(rng.random((5, 9, 11)) * 4.) - 1.        # -1 .. 2, with both zeros
        cube[cube == 0.] *= np.where(rng.random(np.sum(cube == 0.)) < 0.5, -1., 1.)
    elif name == "select":
        cube = rng.normal(0., 1., (6, 10, 12))
        select = np.zeros((10, 12), dtype=np.uint8)
        select[:, :6] = 1
        cube[2, :, :6] = NAN                                    # nothing selected is finite there
    elif name == "nan_and_flat":
        cube = rng.normal(0., 1., (5, 6, 7))
        cube[1] = NAN                                           # an all-NaN channel
        cube[3] = 2.5                                           # identical values: mad == 0
    else:
        raise KeyError(name)
    cube.setflags(write=False)
    return cube, select


@pytest.mark.parametrize("name", ["1", "2", "35", "72", "big", "ties", "select", "nan_and_flat"])
def test_channel_stats_equal_nanmedian(name):
    cube, select = planes(name)
    m, mad, n = P.channel_stats(cube, select)
    with engine(cube.shape) as eng:
        gm, gmad, gn = eng.channel_stats(cube, select=select)
    assert np.array_equal(gn, n)
    assert same(gm, m) and same(gmad, mad)
    if name == "1":
        assert np.array_equal(n, [1] * 4) and np.isnan(P.sigma_of(mad, n)).all()
    if name == "select":
        assert n[2] == 0 and np.isnan(gm[2]) and np.isnan(gmad[2])
    if name == "nan_and_flat":
        assert n[1] == 0 and np.isnan(gm[1]) and gmad[3] == 0. and gm[3] == 2.5


# ---- the whole preparation -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted():
    return P.Planted()


@functools.lru_cache(maxsize=None)
def raw_case(name):
    """(raw cube, noise mask, half window, reject)"""
    if name in ("planted", "planted_no_reject"):
        pl = planted()
        raw, select = pl.raw, pl.noise_mask
        reject = 3.0 if name == "planted" else None
        h = 25
    elif name == "odd":
        fsf, lsf = O.gaussian_fsf_image(3.0), O.gaussian_lsf_vector(21, 0.9088)
        data = O.synthetic_case(21, 12, 10, fsf, lsf, seed=7)[0]
        rng = np.random.default_rng(8)
        raw = data + 3. * rng.random((12, 10))[None] + 0.02 * np.arange(21.)[:, None, None]
        raw[4, 5, 5] = NAN
        raw[:, 11, 9] = NAN
        raw[7] = NAN                                            # a channel of one value: its sigma is NaN
        raw[7, 0, 0] = 9.                                       # and rejects nothing
        select, reject, h = None, 3.0, 4
    else:
        raise KeyError(name)
    raw.setflags(write=False)
    return raw, select, h, reject


@pytest.mark.parametrize("name", ["planted", "planted_no_reject", "odd"])
def test_prepare_equals_the_oracle_composed_on_the_host(name):
    raw, select, h, reject = raw_case(name)
    cont, res, m, sigma, n = P.prepare(raw, select, h, reject)
    with engine(raw.shape) as eng:
        gcont, gres, gm, gsigma, gn = eng.prepare(raw, h, reject, select)
    assert np.array_equal(gn, n)
    assert same(gcont, cont)
    assert same(gres, res)
    assert same(gsigma, sigma)
    assert same(gm, m)
    assert np.isnan(res).any() and np.isfinite(sigma).any()
    if name == "odd":
        assert np.isnan(sigma[7]) and n[7] == 1 and np.isfinite(np.delete(sigma, 7)).all()


def test_prepare_cube_and_rescale_equal_the_oracle():
    pl = planted()
    cont, res, m, sigma, n = P.prepare(pl.raw, pl.noise_mask, 25, 3.0)
    got = d3d.prepare_cube(d3d.MUSE().build_cube(np.array(pl.raw)), noise_mask=pl.noise_mask)
    assert same(got.cube.data, res) and same(got.continuum, cont)
    assert same(got.sigma, sigma) and same(got.channel_median, m) and np.array_equal(got.channel_count, n)
    assert np.array_equal(got.variance, P.variance(sigma, pl.shape))
    assert got.settings["continuum_window"] == 51 and got.settings["reject"] == 3.0
    # a delivered variance that is off by a per-channel factor, with a channel of zeros and a NaN
    rng = np.random.default_rng(9)
    given = pl.true_variance * (0.5 + rng.random(pl.shape[0]))[:, None, None] * (0.9 + 0.2 * rng.random(pl.shape))
    given[5] = 0.
    given[9, 3, 3] = NAN
    want = P.variance(sigma, pl.shape, given, pl.noise_mask)
    got = d3d.prepare_cube(np.array(pl.raw), noise_mask=pl.noise_mask, variance=given, rescale=True)
    assert same(got.variance, want)
    assert same(got.variance[5], given[5]) and not same(got.variance[6], given[6])
    kept = d3d.prepare_cube(np.array(pl.raw), noise_mask=pl.noise_mask, variance=given)
    assert same(kept.variance, given)


def test_c_abi_refusals():
    cube = np.ones((8, 4, 4))
    with engine(cube.shape) as eng:
        for h in (0, 129, -1):
            with pytest.raises(ValueError, match="half_window"):
                eng.running_median(cube, h)
            with pytest.raises(ValueError, match="half_window"):
                eng.prepare(cube, h)
        for reject in (0., -1.):
            with pytest.raises(ValueError, match="reject"):
                eng.prepare(cube, 2, reject)
        assert np.array_equal(eng.running_median(cube, 128), cube)       # (the context is still good)
    with engine(cube.shape) as eng:
        eng.set_tile(0, 0, 4, 0, 4, 0, 4)
        for call in (lambda: eng.running_median(cube, 2), lambda: eng.channel_stats(cube),
                     lambda: eng.prepare(cube, 2)):
            with pytest.raises(NotImplementedError, match="tile"):
                call()


# ---- bit-identity and the public interface -----------------------------------------------------

def test_a_preparation_writes_none_of_the_chains_state():
    D, H, W = 32, 16, 16
    fsf, lsf = O.gaussian_fsf_image(3.0), O.gaussian_lsf_vector(D, 0.9088)
    data, var, mask, _, init, min_b, max_b = O.synthetic_case(D, H, W, fsf, lsf, seed=4242)
    out = []
    for prepared in (False, True):
        with _lib.Engine((D, H, W), fsf.shape) as eng:
            eng.set_taps(fsf, lsf)
            eng.set_data(data, var, mask=mask)
            eng.set_params(init)
            eng.mh_config(min_b, max_b, 0.1, float(max_b[0] ** 2), seed=31, refresh_every=0)
            eng.residual(fetch=False)
            eng.mh_sweeps(1, 1)
            if prepared:                                # (between sweeps: pending updates in flight)
                eng.prepare(data, 5, 3.0)
                eng.running_median(data, 5)
                eng.channel_stats(data)
            eng.mh_sweeps(2, 2)
            out.append((eng.get_params(), eng.download_slot(_lib.SLOT_ERR), eng.get_dlog(),
                        eng.download_slot(_lib.SLOT_DATA), eng.download_slot(_lib.SLOT_IVAR)))
    for a, b in zip(out[1], out[0]):
        assert a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def run_inputs():
    D, H, W = 32, 16, 16
    fsf, lsf = O.gaussian_fsf_image(3.0), O.gaussian_lsf_vector(D, 0.9088)
    data = O.synthetic_case(D, H, W, fsf, lsf, seed=4242)[0]
    rng = np.random.default_rng(10)
    raw = data + 2. * rng.random((H, W))[None] + 0.01 * np.arange(float(D))[:, None, None]
    inst = d3d.Instrument(lsf=VectorLineSpreadFunction(lsf), fsf=ImageFieldSpreadFunction(fsf))
    return inst, d3d.MUSE().build_cube(raw)


def test_run_prepare_is_run_on_the_prepared_cube(tmp_path):
    inst, cube = run_inputs()
    settings = dict(continuum_window=15, reject=3.0)
    kw = dict(max_iterations=21, seed=3, min_acceptance_rate=0.)
    name = str(tmp_path / "ck")
    run = d3d.Run(cube, inst, prepare=settings, write_every=21, checkpoint=name, **kw)
    prep = d3d.prepare_cube(cube, **settings)
    plain = d3d.Run(prep.cube, inst, variance=prep.variance, **kw)
    assert plain.prepared is None
    assert run.prepared is not None and same(run.prepared.cube.data, prep.cube.data)
    assert same(run.prepared.sigma, prep.sigma) and same(run.cube.data, prep.cube.data)
    assert np.array_equal(run.variance_cube, prep.variance)
    assert run.chain.tobytes() == plain.chain.tobytes()
    assert not same(run.cube.data, cube.data)
    # the checkpoint records the settings; a resume with others is refused, with the same it runs
    state = np.load(name + "_state.npz")
    assert same(state["prepare_settings"], [15., 3., 0., -1.])
    resume = dict(kw, max_iterations=3, initial_parameters=name + "_parameters.npy",
                  resume_state=name + "_state.npz")
    for other in (dict(continuum_window=17, reject=3.0), dict(continuum_window=15, reject=None), None):
        with pytest.raises(ValueError, match="preparation settings"):
            d3d.Run(cube, inst, prepare=other, **resume)
    again = d3d.Run(cube, inst, prepare=settings, **resume)
    assert same(again.cube.data, prep.cube.data) and again.sweep_origin == 20


def test_prepare_with_chains_search_and_line_search():
    inst, cube = run_inputs()
    run = d3d.Run(cube, inst, prepare=dict(continuum_window=15), chains=2, initial_search=True,
                  max_iterations=3, seed=3, min_acceptance_rate=0.)
    prep = run.prepared
    found = d3d.line_search(prep.cube, inst, variance=prep.variance)
    assert np.array_equal(run.search.best_index, found.best_index)      # (the search sees the prepared cube)
    direct = d3d.line_search(cube, inst, prepare=dict(continuum_window=15))
    assert np.array_equal(direct.best_index, found.best_index) and same(direct.stat, found.stat)
    assert (found.snr >= 5.).sum() > 50
    assert len(run.chains) == 2 and np.isfinite(run.chains[1][-1]).all()
