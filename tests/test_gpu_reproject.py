"""The step-2 kernels (csrc/p3d_proj.hip) on the GPU: forward and inverse transverse Mercator against the mpmath oracle of
tests/golden/reproject.npz (make_golden_reproject.py) for every setting and for point counts around a wavefront and a workgroup, the exact values
on the central meridian and on the equator, host and device entry points bit for bit, grid -> grid on the device, and the smoothing convolution
against the reference's ``smooth``.

Tolerances (the issue's): forward 1e-6 m (three orders below the finest header unit, 1e-3 m at scalar -1000), inverse 1e-11 degrees (1e-6 m on
the ground), smoothing 1e-6 m (values up to 1e7: one rounding is 2e-9, at most 51 terms)."""
import os

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import crs as C
from pseudo_3d_interpolation_amd.functions import filter as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'reproject.npz'))
SETTINGS = [str(s) for s in G['proj/settings']]
TOL_M, TOL_DEG = 1e-6, 1e-11
COUNTS = [1, 63, 64, 65, 257, 1000]          # one lane, a wavefront and its neighbours, a workgroup of 256 and one more, four workgroups


def points(name, n):
    """The fixture's 63 points of a setting, tiled or cut to ``n``."""
    return tuple(np.resize(G[f'proj/{name}/{k}'], n) for k in ('lon', 'lat', 'E', 'N'))


@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('name', SETTINGS)
def test_forward_and_inverse_against_the_oracle(name, n):
    prm = G[f'proj/{name}/prm']
    lon, lat, E, N = points(name, n)
    gE, gN = _ffi.proj_tmerc(lon, lat, prm)
    print(name, n, 'forward', np.abs(gE - E).max(), np.abs(gN - N).max())
    assert gE.shape == (n,) and gE.dtype == np.float64
    assert np.abs(gE - E).max() <= TOL_M and np.abs(gN - N).max() <= TOL_M
    glon, glat = _ffi.proj_tmerc(E, N, prm, inverse=True)
    print(name, n, 'inverse', np.abs(glon - lon).max(), np.abs(glat - lat).max())
    assert np.abs(glon - lon).max() <= TOL_DEG and np.abs(glat - lat).max() <= TOL_DEG


@pytest.mark.parametrize('name', SETTINGS)
def test_central_meridian_and_equator_are_exact(name):
    prm = G[f'proj/{name}/prm']
    lon, lat, _, _ = points(name, 63)
    gE, gN = _ffi.proj_tmerc(lon, lat, prm)
    on_meridian, on_equator = lon == prm[2], lat == 0
    assert on_meridian.sum() == 9 and on_equator.sum() == 7
    assert np.all(gE[on_meridian] == prm[5])                       # lam = 0: E = x0, not a bit more
    if prm[3] == 0:
        assert np.all(gN[on_equator] == prm[6])                    # lat = 0 with lat0 = 0: N = y0


@pytest.mark.parametrize('n', COUNTS)
def test_host_and_device_entry_points_agree_bit_for_bit(n):
    prm = G['proj/tmerc_lat0/prm']
    lon, lat, E, N = points('tmerc_lat0', n)
    for inverse, (x, y) in ((False, (lon, lat)), (True, (E, N))):
        want = _ffi.proj_tmerc(x, y, prm, inverse=inverse)
        dx, dy, ox, oy = (_ffi.DeviceArray((n + 3,), np.float64) for _ in range(4))
        try:
            dx.upload(np.r_[x, 1.0, 2.0, 3.0])
            dy.upload(np.r_[y, 1.0, 2.0, 3.0])
            ox.upload(np.full(n + 3, 7.0))
            oy.upload(np.full(n + 3, 7.0))
            _ffi.proj_tmerc_dev(dx.ptr, dy.ptr, n, prm, inverse, ox.ptr, oy.ptr)
            gx, gy = ox.download(), oy.download()
            assert gx[:n].tobytes() == want[0].tobytes() and gy[:n].tobytes() == want[1].tobytes()
            assert np.all(gx[n:] == 7) and np.all(gy[n:] == 7)     # nothing is written behind point n - 1
            _ffi.proj_tmerc_dev(dx.ptr, dy.ptr, n, prm, inverse, dx.ptr, dy.ptr)          # in place
            assert dx.download()[:n].tobytes() == want[0].tobytes() and dy.download()[:n].tobytes() == want[1].tobytes()
            assert dx.download()[n:].tolist() == [1, 2, 3]
        finally:
            for b in (dx, dy, ox, oy):
                b.free()


def test_bad_parameters_are_refused_before_any_launch():
    x = np.zeros(4)
    for bad in ([0, 0.003, 9, 0, 1, 0, 0], [6378137, 1.0, 9, 0, 1, 0, 0], [6378137, 0.003, 9, 0, 0, 0, 0], [6378137, 0.003, 9, 91, 1, 0, 0],
                [6378137, 0.003, np.nan, 0, 1, 0, 0]):
        with pytest.raises(_ffi.P3DError):
            _ffi.proj_tmerc(x, x, bad)
    with pytest.raises(ValueError):
        _ffi.proj_tmerc(x, x, [1, 2, 3])
    with pytest.raises(ValueError):
        _ffi.proj_tmerc(x, np.zeros(5), G['proj/tmerc_lat0/prm'])
    empty = _ffi.proj_tmerc(np.zeros(0), np.zeros(0), G['proj/tmerc_lat0/prm'])
    assert empty[0].shape == (0,)


def test_transform_routes_and_refuses_non_finite_results():
    lon, lat, E, N = points('utm32n_grs80', 63)
    gE, gN = C.transform('EPSG:4258', 'EPSG:25832', lon, lat)
    assert np.abs(gE - E).max() <= TOL_M and np.abs(gN - N).max() <= TOL_M
    glon, glat = C.transform('EPSG:25832', '+proj=longlat +ellps=GRS80', E.reshape(7, 9), N.reshape(7, 9))
    assert glon.shape == (7, 9) and np.abs(glon.ravel() - lon).max() <= TOL_DEG and np.abs(glat.ravel() - lat).max() <= TOL_DEG
    bad = lon.copy()
    bad[5] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        C.transform('EPSG:4258', 'EPSG:25832', bad, lat)
    with pytest.raises(ValueError, match='non-finite'):
        C.transform('EPSG:25832', 'EPSG:4258', E, np.where(np.arange(63) == 62, np.inf, N))
    with pytest.raises(ValueError, match='non-finite'):
        C.transform('EPSG:25832', 'EPSG:25833', np.where(np.arange(63) == 0, np.nan, E), N)


def test_grid_to_grid_is_inverse_then_forward_on_the_device():
    src, dst = G['z2z/prm_src'], G['z2z/prm_dst']
    E, N = G['z2z/E_src'], G['z2z/N_src']
    gE, gN = C.transform('EPSG:32632', 'EPSG:32633', E, N)
    print('zone to zone', np.abs(gE - G['z2z/E_dst']).max(), np.abs(gN - G['z2z/N_dst']).max())
    assert np.abs(gE - G['z2z/E_dst']).max() <= TOL_M and np.abs(gN - G['z2z/N_dst']).max() <= TOL_M
    step = _ffi.proj_tmerc(*_ffi.proj_tmerc(E, N, src, inverse=True), dst)
    assert gE.tobytes() == step[0].tobytes() and gN.tobytes() == step[1].tobytes()


@pytest.mark.parametrize('length,wl', [tuple(c) for c in G['smooth/cases'].tolist()])
def test_smooth_against_the_reference(length, wl):
    data, want = G[f'smooth/in/{length}'], G[f'smooth/out/{length}/{wl}']
    got = F.smooth(data, wl)
    print(length, wl, np.abs(got - want).max())
    assert got.shape == data.shape and got.dtype == np.float64 and np.abs(got - want).max() <= TOL_M


def test_smooth_kernel_is_the_convolution_in_index_order():
    rng = np.random.default_rng(4)
    for n, wlen in ((1, 1), (1, 5), (300, 4), (257, 51)):                          # an asymmetric window: the weights are taken reversed
        padded, w = rng.uniform(1e5, 1e7, n + wlen - 1), rng.uniform(0, 1, wlen)
        want = np.zeros(n)
        for k in range(wlen):
            want = want + padded[k:k + n] * w[wlen - 1 - k]
        got = _ffi.proj_smooth(padded, w)
        assert got.tobytes() == want.tobytes(), (n, wlen)
    with pytest.raises(ValueError):
        _ffi.proj_smooth(np.zeros(3), np.zeros(4))
