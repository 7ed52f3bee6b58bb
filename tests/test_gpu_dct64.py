"""transform_kind='DCT' with precision='reference' on the GPU: the double-precision DCT loop (csrc/p3d_dct64.hip through the C ABI, _ffi.Plan64 and
functions/POCS.py) against SciPy's float64 dctn / idctn, against the reference's own double-precision runs (tests/golden/dct.npz, *_out_f64) and against
the NumPy oracle run with SciPy's pair.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import os
import warnings
from functools import partial

import numpy as np
import pytest
import yaml

from conftest import load_golden, parse_params, rel_l2

pytestmark = pytest.mark.gpu

NORMS = ("backward", "ortho")
# ten times the 1e-14 that p3d_fft2_c128 is held to (test_gpu_parity.py): the combine / split multiplies on either side of the transform
TRANSFORM_TOL = 1e-13
# (2, 3): every index self-paired or nearly so; (7, 12), (33, 20): odd x even; (45, 63): both odd, no N/2 partner; (8, 8), (64, 64): powers of two;
# (90, 50): generic line passes; (96, 120): both extents have plans on the double register engine; (256, 256): tile edges of the group kernel's 64 x 4 blocks
SHAPES = [(2, 3), (7, 12), (8, 8), (33, 20), (45, 63), (64, 64), (90, 50), (96, 120), (256, 256)]


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


def _pairs_of(shape):
    """x (3 complex128 slices, the middle one zero) and SciPy's float64 dctn / idctn of it for both norms, computed once per shape."""
    if shape not in _pairs:
        import scipy.fft
        rng = np.random.default_rng(shape[0] * 10007 + shape[1])
        x = rng.standard_normal((3,) + shape) + 1j * rng.standard_normal((3,) + shape)
        x[1] = 0
        _pairs[shape] = (x, {n: scipy.fft.dctn(x, axes=(-2, -1), norm=n) for n in NORMS}, {n: scipy.fft.idctn(x, axes=(-2, -1), norm=n) for n in NORMS})
    return _pairs[shape]


# ------------------------------------------------------------------------------------------------
# transform hook
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dct2_matches_scipy(ffi, shape, norm):
    x, fwd, inv = _pairs_of(shape)
    with ffi.Plan64(shape[0], shape[1], 3) as plan:
        X = plan.dct2(x, norm=norm)
        y = plan.dct2(x, inverse=True, norm=norm)
        back = plan.dct2(X, inverse=True, norm=norm)
        one = plan.dct2(x[0], norm=norm)          # a single 2-D slice is accepted as well
    e_fwd, e_inv, e_rt = rel_l2(X, fwd[norm]), rel_l2(y, inv[norm]), rel_l2(back, x)
    print(f"dct2 (double) {shape[0]}x{shape[1]} {norm}: forward {e_fwd:.2e} inverse {e_inv:.2e} round trip {e_rt:.2e}")
    assert X.dtype == np.complex128 and X.shape == x.shape
    assert not X[1].any() and not y[1].any() and not back[1].any()      # the zero slice of the batch stays exactly zero
    assert e_fwd <= TRANSFORM_TOL and e_inv <= TRANSFORM_TOL and e_rt <= TRANSFORM_TOL, (e_fwd, e_inv, e_rt)
    assert np.array_equal(one, X[0])


# ------------------------------------------------------------------------------------------------
# statistics for the schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,norm", [((33, 20), "ortho"), ((64, 64), "backward"), ((90, 50), "ortho")])
def test_dct_stats_match_scipy(ffi, shape, norm):
    import scipy.fft
    x, fwd, _ = _pairs_of(shape)
    X = fwd[norm]
    xr = np.ascontiguousarray(x.real)
    with ffi.Plan64(shape[0], shape[1], 3) as plan:
        st = plan.dct_stats_dev(x.ctypes.data, ffi.P3D_C128, 3, norm=norm)                # a host pointer ...
        xd = ffi.DeviceArray(x.shape, x.dtype).upload(x)
        st_dev = plan.dct_stats_dev(xd.ptr, ffi.P3D_C128, 3, norm=norm)                   # ... and a device pointer
        xd.free()
        st_real = plan.dct_stats_dev(xr.ctypes.data, ffi.P3D_F64, 3, norm=norm)
    assert np.array_equal(st, st_dev)
    for s in range(3):
        if s == 1:
            assert st[s, 2] == 0 and st[s, 4] == 0
            continue
        pk, top = X[s].max(), np.abs(X[s]).max()          # NumPy's lexicographic complex maximum (POCS.py:288)
        assert abs(st[s, 0] - pk.real) <= 1e-12 * abs(pk) and abs(st[s, 1] - pk.imag) <= 1e-12 * abs(pk)
        assert abs(st[s, 2] - top) <= 1e-12 * top
        assert abs(st[s, 3] - np.abs(X[s]).min()) <= 1e-12 * top
        assert abs(st[s, 4] - np.linalg.norm(X[s]) ** 2) <= 1e-12 * np.linalg.norm(X[s]) ** 2
    # a float64 cube runs as complex with zero imaginary part: the statistics of the real part's DCT; the imaginary part of its peak is rounding noise,
    # which pocs_cube sets to zero before it builds the (real) schedule
    Xr = scipy.fft.dctn(xr, axes=(-2, -1), norm=norm)
    for s in (0, 2):
        top = np.abs(Xr[s]).max()
        assert abs(st_real[s, 0] - Xr[s].max()) <= 1e-12 * top and abs(st_real[s, 1]) <= 1e-12 * top
        assert abs(st_real[s, 2] - top) <= 1e-12 * top
        assert abs(st_real[s, 3] - np.abs(Xr[s]).min()) <= 1e-12 * top
        assert abs(st_real[s, 4] - np.linalg.norm(Xr[s]) ** 2) <= 1e-12 * np.linalg.norm(Xr[s]) ** 2


# ------------------------------------------------------------------------------------------------
# golden vectors of the reference: its own double-precision runs
# ------------------------------------------------------------------------------------------------
CASES = ["soft_lin", "real_hard_exp", "real_garrote_odd", "fast", "adaptive", "pmin_adaptive_early", "sqrt_decay", "factors", "alpha08", "tiny_8x8",
         "niter1", "cplx_hard_exp"]          # (every case of dct.npz but the percentile one)
_golden_runs = {}


def _golden_run(P, G, name, wide):
    """pocs_cube(..., precision='reference') of one golden case, fed in double precision (``wide``) or as stored; any warning is an error."""
    if (name, wide) not in _golden_runs:
        params = parse_params(G[name + "_params"])
        x, mask, norm = G[name + "_x"], G[name + "_mask"], str(G[name + "_norm"])
        if wide:
            x = x.astype(G[name + "_out_f64"].dtype)
        rows = []
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = P.pocs_cube(x[None], mask, transform_kind="DCT", dct_norm=norm, precision="reference", results=rows, **params)
        _golden_runs[(name, wide)] = (x, y[0], rows[0])
    return _golden_runs[(name, wide)]


def test_golden_fixture_holds_the_cases(G):
    assert [n for n in G["names"] if "percentile" not in parse_params(G[n + "_params"])["thresh_op"]] == CASES
    assert int(G["pmin_adaptive_early_niter"][1]) == 8       # the early exit: 8 of 10 iterations


@pytest.mark.parametrize("name", CASES)
def test_golden_case_in_double(P, G, name):
    x, y, info = _golden_run(P, G, name, True)
    want = G[name + "_out_f64"]
    err = rel_l2(y, want)
    print(f"golden {name} (double): rel-L2 {err:.2e}, niter {info['niterations']}")
    assert y.dtype == x.dtype == want.dtype and y.shape == want.shape
    assert info["niterations"] == int(G[name + "_niter"][1])
    assert np.allclose(info["costs"], G[name + "_costs_f64"], rtol=1e-6, atol=1e-18)   # (a cost is a squared difference of two nearly equal sums)
    assert err <= 1e-10, (name, err)


@pytest.mark.parametrize("name", CASES)
def test_golden_case_as_stored(P, G, name):
    x, y, info = _golden_run(P, G, name, False)
    _, y64, info64 = _golden_run(P, G, name, True)
    want = G[name + "_out_f64"]
    err = rel_l2(y, want)
    print(f"golden {name} (as stored, {x.dtype}): rel-L2 {err:.2e}")
    assert y.dtype == x.dtype and x.dtype in (np.complex64, np.float32)
    assert err <= 1e-7, (name, err)                                   # (the final cast)
    assert info["niterations"] == info64["niterations"]
    assert np.array_equal(y, y64.astype(x.dtype))                     # the double run's result, cast down


# ------------------------------------------------------------------------------------------------
# larger plans against the oracle with SciPy's pair in double
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh_op", ["soft", "hard"])
@pytest.mark.parametrize("shape", [(90, 50), (96, 120), (256, 256)])
def test_larger_plans_match_the_oracle(P, shape, thresh_op):
    from oracle import pocs_oracle as orc
    _, mask, obs = orc.synthetic_cube(shape[0], shape[1], 3, 0.5)
    wide = obs.astype(np.complex128)
    params = dict(niter=4, thresh_op=thresh_op, thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    fwd, inv = _scipy_pair("ortho")
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = P.pocs_cube(wide, mask, transform_kind="DCT", dct_norm="ortho", precision="reference", results=rows, **params)
    assert got.dtype == np.complex128
    for s in range(3):
        info = {}
        want = orc.pocs_slice(wide[s], mask, transform_kind="DCT", fwd=fwd, inv=inv, info=info, **params)
        err = rel_l2(got[s], want)
        print(f"{shape[0]}x{shape[1]} {thresh_op} slice {s}: rel-L2 {err:.2e}")
        assert err <= 1e-10, (s, err)
        assert rows[s]["niterations"] == info["niterations"] == 4


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def _cube5(G, real):
    """Five 32 x 48 slices made of the `adaptive` case's slice (shifted, scaled, rotated; the third one zero), a little noise on the observed samples."""
    x, mask = G["adaptive_x"], G["adaptive_mask"]
    rng = np.random.default_rng(17)
    cube = np.stack([x, np.roll(x, 3, axis=0), np.zeros_like(x), np.roll(x, 5, axis=1) * 0.5, x * np.exp(0.7j)]) * mask
    cube = cube + (0.01 * rng.standard_normal(cube.shape) * mask * (np.abs(cube) > 0)).astype(np.float32)
    return (cube.real.astype(np.float64) if real else cube.astype(np.complex128)), mask


@pytest.mark.parametrize("real", [False, True])
def test_batch_equals_slice_by_slice(P, G, real):
    cube, mask = _cube5(G, real)
    prm = dict(transform_kind="DCT", dct_norm="ortho", precision="reference", niter=6, thresh_op="hard", thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    rows = []
    whole = P.pocs_cube(cube, mask, results=rows, **prm)
    assert whole.dtype == cube.dtype and not whole[2].any() and rows[2]["niterations"] == 0 and rows[0]["niterations"] == 6
    for s in range(5):
        assert np.array_equal(P.pocs_cube(cube[s:s + 1], mask, **prm)[0], whole[s]), s
    assert np.array_equal(P.pocs_cube(cube, mask, batch_slices=2, **prm), whole)
    # the observed traces are kept (alpha = 1), the missing ones filled
    obs = mask > 0
    assert rel_l2(whole[0][obs], cube[0][obs]) < 1e-14 and np.abs(whole[0][~obs]).max() > 0


def test_dct_run_on_device_pointers_equals_host_pointers(ffi, G):
    cube, mask = _cube5(G, False)
    mask64 = mask.astype(np.float64)
    n, nil, nxl = cube.shape
    with ffi.Plan64(nil, nxl, n) as plan:
        st = plan.dct_stats_dev(cube.ctypes.data, ffi.P3D_C128, n, norm="ortho")
        active = st[:, 2] > 0
        tau = np.linspace(0.5, 0.01, 5)[None, :] * st[:, 2:3]
        out, done, sums, _ = plan.dct_run(cube, mask64, tau, 5, thresh_op="soft", eps=0.0, active=active, norm="ortho")
        xd, md, od = ffi.DeviceArray(cube.shape, cube.dtype).upload(cube), ffi.DeviceArray(mask64.shape, mask64.dtype).upload(mask64), ffi.DeviceArray(cube.shape, cube.dtype)
        done_d, sums_d, _ = plan.dct_run_dev(xd.ptr, ffi.P3D_C128, md.ptr, tau, 5, od.ptr, n, thresh_op="soft", eps=0.0, active=active, norm="ortho")
        out_d = od.download()
        for b in (xd, md, od):
            b.free()
    assert list(done) == [5, 5, 0, 5, 5] and np.array_equal(done, done_d)
    assert np.array_equal(out, out_d) and np.array_equal(sums, sums_d)         # no atomics: the sums are bitwise equal as well
    assert not out[2].any() and sums[1:, 0].all()


# ------------------------------------------------------------------------------------------------
# one mask per slice
# ------------------------------------------------------------------------------------------------
def test_per_slice_masks(P):
    from oracle import pocs_oracle as orc
    nil, nxl, n = 24, 40, 3
    _, _, obs = orc.synthetic_cube(nil, nxl, n, 0.0)
    masks = np.stack([orc.synthetic_mask(nil, nxl, m) for m in (0.3, 0.5, 0.7)])
    assert not np.array_equal(masks[0], masks[1])
    cube = (obs * masks).astype(np.complex128)
    prm = dict(transform_kind="DCT", dct_norm="backward", precision="reference", niter=5, thresh_op="garrote", thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    rows, one = [], []
    got = P.pocs_cube(cube, masks, results=rows, **prm)
    for s in range(n):
        assert np.array_equal(P.pocs_cube(cube[s:s + 1], masks[s], results=one, **prm)[0], got[s]), s
        assert one[-1]["costs"] == rows[s]["costs"]
    assert not np.array_equal(P.pocs_cube(cube[1:2], masks[0], **prm)[0], got[1])      # (slice 1 did use its own mask)
    # identical masks, stacked, equal the shared-mask call
    shared = P.pocs_cube(cube, masks[0], **prm)
    assert np.array_equal(P.pocs_cube(cube, np.stack([masks[0]] * n), **prm), shared)


# ------------------------------------------------------------------------------------------------
# what the double-precision loop does not cover keeps the float32 kernels
# ------------------------------------------------------------------------------------------------
def test_percentile_operator_warns_and_runs_the_float32_kernels(P, G):
    name = "hard_pct"
    params = parse_params(G[name + "_params"])
    x, mask, norm = G[name + "_x"], G[name + "_mask"], str(G[name + "_norm"])
    with pytest.warns(RuntimeWarning, match="does not cover"):
        y = P.pocs_cube(x[None], mask, transform_kind="DCT", dct_norm=norm, precision="reference", **params)
    assert y.dtype == x.dtype
    assert np.array_equal(y, P.pocs_cube(x[None], mask, transform_kind="DCT", dct_norm=norm, **params))


# ------------------------------------------------------------------------------------------------
# step 13 driver
# ------------------------------------------------------------------------------------------------
def test_cli_step13_passes_precision_on(P, G, tmp_path):
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
    listing, Y = {}, {}
    for tag, meta in (('plain', metadata), ('reference', dict(metadata, precision='reference'))):
        yml = tmp_path / f'pocs_{tag}.yml'
        yml.write_text(yaml.safe_dump({'dim': 'freq_twt', 'var': 'freq_env', 'batch_chunk': 3, 'output_runtime_results': True, 'metadata': meta}))
        out_dir = tmp_path / tag / 'out'
        os.makedirs(out_dir.parent)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            step13.main(['13_cube_interpolate_POCS', path, '--path_pocs_parameter', str(yml), '--path_output_dir', str(out_dir)])
        listing[tag] = sorted(os.listdir(out_dir))
        icube = open_cube(f'{out_dir}.npz')
        Y[tag] = icube.data_vars['freq_env_interp.real'] + 1j * icube.data_vars['freq_env_interp.imag']
        if tag == 'reference':
            assert 'precision' in icube.attrs['interp_params_keys']
    assert listing['reference'] == listing['plain'] and any(f.startswith('cube_freq_DCT_soft_niter-6_ortho_') for f in listing['plain'])
    params = {k: v for k, v in metadata.items() if k != 'verbose'}
    want = P.pocs_cube(data, np.where(fold <= 1, fold, 1), **dict(params, transform_kind='DCT', dct_norm='ortho', precision='reference'))
    assert want.dtype == np.complex64 and np.array_equal(Y['reference'].astype(np.complex64), want)
    assert not np.array_equal(Y['reference'].astype(np.complex64), Y['plain'].astype(np.complex64))    # (the key did change the arithmetic)
