"""transform_kind='DCT' on the GPU (csrc/p3d_dct.hip through the C ABI and functions/POCS.py) against SciPy's dctn / idctn and against the
reference's own POCS_algorithm run with that pair (tests/golden/dct.npz, make_golden_dct.py).  Needs a real MI355X:  python -m pytest tests -m gpu"""
import os
from functools import partial

import numpy as np
import pytest
import yaml

from conftest import load_golden, parse_params, rel_l2

pytestmark = pytest.mark.gpu

NORMS = ("backward", "ortho")
# 2e-6 rel-L2: the bar test_gpu_parity.py holds fft2 to against NumPy.  Where a shape measures above it, the bound becomes twice the error of SciPy's
# own single-precision dctn (of the complex64 input) against its float64 result, computed in the test.
TRANSFORM_TOL = 2e-6
# (7, 12) ... (90, 50): the any-length FFT; (8, 8), (64, 64): the tuned kernels (64 x 64 is the resident loop's size class); (256, 256): a register-engine plan
SHAPES = [(2, 3), (8, 8), (7, 12), (33, 20), (90, 50), (64, 64), (256, 256)]


@pytest.fixture(scope="module")
def G():
    return load_golden("dct.npz")


@pytest.fixture(scope="module")
def ffi():
    from pseudo_3d_interpolation_amd import _ffi
    assert _ffi.device_count() >= 1, "no GPU visible"
    return _ffi


@pytest.fixture(scope="module")
def P():
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    yield mod
    mod.release_plans()


def _scipy_pair(norm):
    import scipy.fft
    return partial(scipy.fft.dctn, norm=norm), partial(scipy.fft.idctn, norm=norm)


_pairs = {}


def _pairs_of(G, shape):
    """x (3 slices, the middle one zero) and SciPy's float64 dctn / idctn of it for both norms: stored for the small shapes, computed here (once) for the
    others, which would not fit a committed file."""
    if shape not in _pairs:
        key = f"pair_{shape[0]}x{shape[1]}"
        if key + "_x" in G.files:
            _pairs[shape] = (G[key + "_x"], {n: G[f"{key}_{n}_dctn"] for n in NORMS}, {n: G[f"{key}_{n}_idctn"] for n in NORMS})
        else:
            import scipy.fft
            rng = np.random.default_rng(shape[0] * 10007 + shape[1])
            x = (rng.standard_normal((3,) + shape) + 1j * rng.standard_normal((3,) + shape)).astype(np.complex64)
            x[1] = 0
            xd = x.astype(np.complex128)
            _pairs[shape] = (x, {n: scipy.fft.dctn(xd, axes=(-2, -1), norm=n) for n in NORMS}, {n: scipy.fft.idctn(xd, axes=(-2, -1), norm=n) for n in NORMS})
    return _pairs[shape]


def _bound(measured, single, want):
    """TRANSFORM_TOL, or -- only where the device measures above it -- twice SciPy's own single-precision error."""
    if measured < TRANSFORM_TOL:
        return TRANSFORM_TOL
    return 2 * rel_l2(single(), want)


# ------------------------------------------------------------------------------------------------
# transform hook
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dct2_matches_scipy(ffi, G, shape, norm):
    import scipy.fft
    x, fwd, inv = _pairs_of(G, shape)
    with ffi.Plan(shape[0], shape[1], 3) as plan:
        X = plan.dct2(x, norm=norm)
        y = plan.dct2(x, inverse=True, norm=norm)
        back = plan.dct2(X, inverse=True, norm=norm)
        one = plan.dct2(x[0], norm=norm)          # a single 2-D slice is accepted as well
    e_fwd, e_inv, e_rt = rel_l2(X, fwd[norm]), rel_l2(y, inv[norm]), rel_l2(back, x)
    print(f"dct2 {shape[0]}x{shape[1]} {norm}: forward {e_fwd:.2e} inverse {e_inv:.2e} round trip {e_rt:.2e}")
    assert X.dtype == np.complex64 and X.shape == x.shape
    assert not X[1].any() and not y[1].any()      # the zero slice of the batch stays zero
    assert e_fwd < _bound(e_fwd, lambda: scipy.fft.dctn(x, axes=(-2, -1), norm=norm), fwd[norm]), e_fwd
    assert e_inv < _bound(e_inv, lambda: scipy.fft.idctn(x, axes=(-2, -1), norm=norm), inv[norm]), e_inv
    assert e_rt < _bound(e_rt, lambda: scipy.fft.idctn(scipy.fft.dctn(x, axes=(-2, -1), norm=norm), axes=(-2, -1), norm=norm), x.astype(np.complex128)), e_rt
    assert np.array_equal(one, X[0])


# ------------------------------------------------------------------------------------------------
# statistics for the schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,norm", [((33, 20), "ortho"), ((64, 64), "backward"), ((90, 50), "ortho")])
def test_dct_stats_match_scipy(ffi, G, shape, norm):
    x, fwd, _ = _pairs_of(G, shape)
    X = fwd[norm]
    with ffi.Plan(shape[0], shape[1], 3) as plan:
        st = plan.dct_stats(x, norm=norm)
        xd = plan.alloc(x.nbytes).upload(x)
        st_dev = plan.dct_stats_dev(xd.ptr, ffi.P3D_C64, 3, norm=norm)
        st_real = plan.dct_stats(x.real.astype(np.float32), norm=norm)
        xd.free()
    assert np.array_equal(st, st_dev)
    for s in range(3):
        if s == 1:
            assert st[s, 2] == 0 and st[s, 4] == 0
            continue
        pk = X[s].max()                           # NumPy's lexicographic complex maximum (POCS.py:288)
        assert abs(st[s, 0] - pk.real) < 1e-5 * abs(pk) and abs(st[s, 1] - pk.imag) < 1e-5 * abs(pk)
        assert abs(st[s, 2] - np.abs(X[s]).max()) < 1e-5 * np.abs(X[s]).max()
        assert abs(st[s, 3] - np.abs(X[s]).min()) < 1e-5 * np.abs(X[s]).max()     # (an absolute error of the size of the largest coefficient's rounding)
        assert abs(st[s, 4] - np.linalg.norm(X[s]) ** 2) < 1e-5 * np.linalg.norm(X[s]) ** 2
    # a float32 cube runs as complex with zero imaginary part: the statistics of the real part's DCT
    import scipy.fft
    Xr = scipy.fft.dctn(x.real.astype(np.float64), axes=(-2, -1), norm=norm)
    for s in (0, 2):
        assert abs(st_real[s, 0] - Xr[s].max()) < 1e-5 * np.abs(Xr[s]).max()
        assert abs(st_real[s, 2] - np.abs(Xr[s]).max()) < 1e-5 * np.abs(Xr[s]).max()
        assert abs(st_real[s, 4] - np.linalg.norm(Xr[s]) ** 2) < 1e-5 * np.linalg.norm(Xr[s]) ** 2


# ------------------------------------------------------------------------------------------------
# golden vectors of the reference
# ------------------------------------------------------------------------------------------------
CASES = ["soft_lin", "real_hard_exp", "real_garrote_odd", "fast", "adaptive", "pmin_adaptive_early", "sqrt_decay", "factors", "alpha08", "hard_pct",
         "tiny_8x8", "niter1", "cplx_hard_exp"]


def test_golden_fixture_holds_the_cases_and_the_binding_bound(G):
    assert list(G["names"]) == CASES
    spreads = [rel_l2(G[n + "_out"], G[n + "_out_f64"]) for n in CASES]
    assert sum(5 * s < 1e-5 for s in spreads) >= 10          # 1e-5 is the binding bound of at least ten cases
    assert int(G["pmin_adaptive_early_niter"][1]) == 8       # the early exit: 8 of 10 iterations


@pytest.mark.parametrize("name", CASES)
def test_golden_case(P, G, name):
    params = parse_params(G[name + "_params"])
    x, mask, norm = G[name + "_x"], G[name + "_mask"], str(G[name + "_norm"])
    fwd, inv = _scipy_pair(norm)
    info = {}
    y = P.POCS_algorithm(x, mask, transform=fwd, itransform=inv, transform_kind="DCT", results_dict=info, **params)
    want = G[name + "_out_f64"]
    assert y.shape == want.shape
    assert np.iscomplexobj(y) == np.iscomplexobj(want)
    assert y.dtype == x.dtype
    spread = rel_l2(G[name + "_out"], want)
    err = rel_l2(y, want)
    print(f"golden {name}: rel-L2 {err:.2e} (reference's own single-vs-double spread {spread:.2e}), niter {info['niterations']}")
    assert info["niterations"] == int(G[name + "_niter"][1])
    c_ref = G[name + "_costs_f64"]
    assert abs(info["cost"] - c_ref[-1]) <= 2e-2 * abs(c_ref[-1]) + 1e-12
    assert err < max(5 * spread, 1e-5), (name, err, spread)


def test_zero_slice_comes_back_untouched(P):
    z = np.zeros((16, 24), np.float32)
    m = np.ones((16, 24), np.uint8)
    info = {}
    fwd, inv = _scipy_pair("ortho")
    y = P.POCS(z, m, transform=fwd, itransform=inv, transform_kind="DCT", niter=5, eps=0, results_dict=info)
    assert y.dtype == np.float32 and not y.any() and info["niterations"] == 0 and info["cost"] == 0


def test_double_cubes_warn_and_run_the_float32_kernels(P, G):
    name = "tiny_8x8"
    params = parse_params(G[name + "_params"])
    x, mask = G[name + "_x"], G[name + "_mask"]
    with pytest.warns(RuntimeWarning, match="does not cover the DCT transform"):
        y = P.pocs_cube(x[None].astype(np.complex128), mask, transform_kind="DCT", dct_norm="backward", **params)
    assert y.dtype == np.complex128
    assert np.array_equal(y.astype(np.complex64), P.pocs_cube(x[None], mask, transform_kind="DCT", dct_norm="backward", **params))


# ------------------------------------------------------------------------------------------------
# keep / zero decisions of the hard threshold
# ------------------------------------------------------------------------------------------------
# (thresholds of the case's own schedule: the first keeps one coefficient, the middle ones cut through the body of the spectrum, the late ones sit in the floor)
@pytest.mark.parametrize("name,iteration", [("real_hard_exp", 0), ("real_hard_exp", 6), ("real_hard_exp", 11), ("cplx_hard_exp", 8), ("cplx_hard_exp", 18)])
def test_dct_shrink_decisions(ffi, P, G, name, iteration):
    """The method of test_step_decisions_and_result (test_gpu_parity.py): the device's keep / zero pattern differs from the float64 spectrum's only
    where | |X| - Re tau | lies within the float32 rounding band of the spectrum's peak."""
    import scipy.fft
    params = parse_params(G[name + "_params"])
    norm = str(G[name + "_norm"])
    x = G[name + "_x"].astype(np.complex64)
    X = scipy.fft.dctn(x.astype(np.complex128), norm=norm)
    tau = P.get_threshold_decay(params["thresh_model"], params["niter"], "DCT", params["p_max"], params["p_min"], X, "values")
    t = tau[iteration]
    with ffi.Plan(x.shape[0], x.shape[1], 1) as plan:
        shr = plan.dct_shrink(x, t, "hard", norm=norm)
    band = np.abs(np.abs(X) - t.real) <= 2e-6 * np.abs(X).max()
    assert band.mean() < 0.06, "tie band should be a sliver of the spectrum"
    kept_gpu, kept_ref = shr != 0, ~np.less(np.abs(X), t)
    assert 0 < kept_ref.sum() < X.size
    assert np.array_equal(kept_gpu[~band], kept_ref[~band]), int(np.count_nonzero(kept_gpu[~band] != kept_ref[~band]))
    assert np.count_nonzero(kept_gpu != kept_ref) <= max(4, 2e-4 * X.size)
    assert np.abs(shr - np.where(kept_gpu, X, 0)).max() < 4e-6 * np.abs(X).max()     # what is kept is the coefficient itself


# ------------------------------------------------------------------------------------------------
# batching
# ------------------------------------------------------------------------------------------------
def _cube5(G, real):
    x, mask = G["adaptive_x"], G["adaptive_mask"]
    rng = np.random.default_rng(17)
    cube = np.stack([x, np.roll(x, 3, axis=0), np.zeros_like(x), np.roll(x, 5, axis=1) * 0.5, x * np.exp(0.7j)]) * mask
    cube = cube + (0.01 * rng.standard_normal(cube.shape) * mask * (np.abs(cube) > 0)).astype(np.float32)
    return (cube.real.astype(np.float32) if real else cube.astype(np.complex64)), mask


def test_batch_equals_slice_by_slice_complex(P, G):
    _check_batch(P, G, False)


def test_batch_equals_slice_by_slice_real(P, G):
    _check_batch(P, G, True)


def _check_batch(P, G, real):
    cube, mask = _cube5(G, real)
    prm = dict(transform_kind="DCT", dct_norm="ortho", niter=6, thresh_op="hard", thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    rows = []
    whole = P.pocs_cube(cube, mask, results=rows, **prm)
    assert whole.dtype == cube.dtype and not whole[2].any() and rows[2]["niterations"] == 0 and rows[0]["niterations"] == 6
    for s in range(5):
        assert np.array_equal(P.pocs_cube(cube[s:s + 1], mask, **prm)[0], whole[s]), s
    assert np.array_equal(P.pocs_cube(cube, mask, batch_slices=2, **prm), whole)
    # the observed traces are kept (alpha = 1), the missing ones filled
    obs = mask > 0
    assert rel_l2(whole[0][obs], cube[0][obs]) < 1e-6 and np.abs(whole[0][~obs]).max() > 0


def test_dct_run_dev_equals_dct_run(ffi, G):
    cube, mask = _cube5(G, False)
    maskf = mask.astype(np.float32)
    n, nil, nxl = cube.shape
    with ffi.Plan(nil, nxl, n) as plan:
        st = plan.dct_stats(cube, norm="ortho")
        active = st[:, 2] > 0
        tau = np.linspace(0.5, 0.01, 5)[None, :] * st[:, 2:3]
        out, done, sums, _ = plan.dct_run(cube, maskf, tau, 5, thresh_op="soft", eps=0.0, active=active, norm="ortho")
        xd, md, od = plan.alloc(cube.nbytes).upload(cube), plan.alloc(maskf.nbytes).upload(maskf), plan.alloc(cube.nbytes)
        done_d, sums_d, _ = plan.dct_run_dev(xd.ptr, ffi.P3D_C64, md.ptr, tau, 5, od.ptr, n, thresh_op="soft", eps=0.0, active=active, norm="ortho")
        out_d = od.download(cube.shape, cube.dtype)
        for b in (xd, md, od):
            b.free()
    assert np.array_equal(out, out_d) and np.array_equal(done, done_d) and list(done) == [5, 5, 0, 5, 5]
    assert np.allclose(sums, sums_d, rtol=1e-12)         # (block sums meet in atomic additions: the order of the last bits is not fixed)
    assert not out[2].any()


# ------------------------------------------------------------------------------------------------
# step 13 driver
# ------------------------------------------------------------------------------------------------
def test_cli_step13_with_dct(P, G, tmp_path):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, open_cube, save_cube

    x, mask = G["adaptive_x"], G["adaptive_mask"]          # 32 x 48
    nil, nxl = x.shape
    data = np.stack([x, np.roll(x, 2, axis=0) * mask, x * 0.5, np.roll(x, 7, axis=1) * mask]).astype(np.complex64)
    fold = (mask * 2).astype(np.uint8)                      # fold 2 where observed: the driver's mask is min(fold, 1)
    cube = Cube({'freq_env': data, 'fold': fold}, {'freq_env': ('freq_twt', 'iline', 'xline'), 'fold': ('iline', 'xline')},
                {'freq_twt': 0.5 * np.arange(4), 'iline': np.arange(nil), 'xline': np.arange(nxl)},
                {'long_name': 'test cube', 'description': 'synthetic', 'history': 'made;', 'text': ''}, {}, {})
    path = save_cube(cube, str(tmp_path / 'cube_freq.npz'))
    metadata = dict(transform_kind='dct', niter=6, eps=0, thresh_op='soft', thresh_model='exponential', decay_kind='values', p_max=0.99, p_min=0.01,
                    alpha=1.0, sqrt_decay=False, version='regular', verbose=False)
    for given, norm in ((None, 'ortho'), ('backward', 'backward')):
        meta = dict(metadata) if given is None else dict(metadata, dct_norm=given)
        yml = tmp_path / f'pocs_{norm}.yml'
        yml.write_text(yaml.safe_dump({'dim': 'freq_twt', 'var': 'freq_env', 'batch_chunk': 3, 'output_runtime_results': True, 'metadata': meta}))
        out_dir = tmp_path / f'out_{norm}'
        step13.main(['13_cube_interpolate_POCS', path, '--path_pocs_parameter', str(yml), '--path_output_dir', str(out_dir)])
        prefix = f'cube_freq_DCT_soft_niter-6_{norm}'
        files = sorted(p for p in os.listdir(out_dir) if p.endswith('.npz'))
        assert len(files) == 2 and all(f.startswith(prefix + '_') for f in files), files
        assert (out_dir / f'runtimes_{prefix}.txt').exists()
        icube = open_cube(f'{out_dir}.npz')
        Y = icube.data_vars['freq_env_interp.real'] + 1j * icube.data_vars['freq_env_interp.imag']
        params = {k: v for k, v in metadata.items() if k != 'verbose'}
        want = P.pocs_cube(data, np.where(fold <= 1, fold, 1), **dict(params, transform_kind='DCT', dct_norm=norm))
        assert np.array_equal(Y.astype(np.complex64), want)
        assert 'DCT' in icube.attrs['history'] and 'dct_norm' in icube.attrs['interp_params_keys']
