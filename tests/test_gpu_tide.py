"""Step 6 on the GPU: ``tide_predict_kernel`` (csrc/p3d_tide.hip) through ``load_subset`` against the mpmath evaluation of tests/golden/tide.npz
(make_golden_tide.py) on the synthetic model, and ``compensate_tide`` against the reference's own results.

Tolerance of the prediction, 1e-8 m absolute: the arguments reach about 1.2e9 s x 2.9e-4 rad/s = 3.5e5 rad, where a double resolves about 1e-10 rad;
the fixture's amplitudes sum to less than 10 m, so the error is about 1e-9 m and 1e-8 m is a tenfold margin.  The compensation is exact."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import tide_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import tide as T  # noqa: E402
from pseudo_3d_interpolation_amd.functions import tide_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'tide.npz'))
TOL_M = 1e-8
EPOCH = np.datetime64('1992-01-01T00:00:00', 'us')
SETS = {1: ('k1',), 8: H.CONSTITUENTS[:8], 14: H.CONSTITUENTS[::-1]}          # 14: every id, in another order than the ids'


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('model'))
    H.make_model(folder)
    return folder


def expected(names, rows):
    cols = [H.CONSTITUENTS.index(c) for c in names]
    return G['pred/terms'][rows][:, cols].sum(axis=1)


@pytest.mark.parametrize('nc', sorted(SETS))
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_kernel_against_mpmath(model, n, nc):
    rows = np.arange(n) + (300 - n if n < 257 else 0)                           # the short ones from the end: seam and dry-patch points
    lon, lat, t = G['pred/lon'][rows], G['pred/lat'][rows], G['pred/t'][rows]
    sub = M.load_subset(model, SETS[nc], lon, lat)
    got = _ffi.tide_predict(sub.lon, lat, t, sub.hre, sub.him, sub.wet, sub.grid, sub.ids)
    want = expected(SETS[nc], rows)
    assert got.shape == (n,) and got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
    worst = np.nanmax(np.abs(got - want)) if not np.isnan(want).all() else 0.0
    print(f'n = {n}, nc = {nc}: worst {worst:.3e} m, {int(np.isnan(want).sum())} NaN')
    assert worst <= TOL_M


def test_tide_predict_takes_times_and_dry_points_are_nan_without_touching_their_neighbours(model):
    lon, lat, t, ndry = (G[f'pred/{k}'] for k in ('lon', 'lat', 't', 'ndry'))
    times = EPOCH + np.rint(t * 1e6).astype(np.int64).astype('timedelta64[us]')      # the nearest microsecond: 5e-7 s x 10 m x 3e-4 / s = 1.5e-9 m of the bound
    got = T.tide_predict(model, lat, lon, times, H.CONSTITUENTS[:8])
    want = expected(H.CONSTITUENTS[:8], np.arange(lon.size))
    dry = ndry == 4
    assert dry.sum() >= 5 and np.isnan(got[dry]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= TOL_M
    # the neighbours of a dry point, alone, give the same bits as in the batch
    k = int(np.flatnonzero(dry)[0])
    near = np.array([i for i in (k - 1, k + 1) if not np.isnan(want[i])])
    alone = T.tide_predict(model, lat[near], lon[near], times[near], H.CONSTITUENTS[:8])
    sub = M.load_subset(model, H.CONSTITUENTS[:8], lon, lat)                     # ... on the same subset (the unwrapped longitude is the same number)
    batch = _ffi.tide_predict(sub.lon, lat, t, sub.hre, sub.him, sub.wet, sub.grid, sub.ids)
    pick = _ffi.tide_predict(sub.lon[near], lat[near], t[near], sub.hre, sub.him, sub.wet, sub.grid, sub.ids)
    assert np.array_equal(pick, batch[near]) and np.abs(alone - want[near]).max() <= TOL_M
    strings = np.datetime_as_string(times[:5], 's')
    assert np.array_equal(T.tide_predict(model, lat[:5], lon[:5], list(strings), ['m2']), T.tide_predict(model, lat[:5], lon[:5], times[:5].astype('datetime64[s]'), ['m2']))
    assert T.tide_predict(model, [], [], np.array([], 'datetime64[s]')).shape == (0,)


def test_device_and_host_entry_points_agree_bit_for_bit(model):
    n = 257
    lon, lat, t = G['pred/lon'][:n], G['pred/lat'][:n], G['pred/t'][:n]
    sub = M.load_subset(model, H.CONSTITUENTS, lon, lat)
    host = _ffi.tide_predict(sub.lon, lat, t, sub.hre, sub.him, sub.wet, sub.grid, sub.ids)
    nc, nxs, nys = sub.hre.shape
    arrays = [(sub.lon, np.float64), (lat, np.float64), (t, np.float64), (sub.hre, np.int32), (sub.him, np.int32), (sub.wet, np.uint8)]
    bufs = [_ffi.DeviceArray(np.shape(a), dt).upload(np.ascontiguousarray(a, dtype=dt)) for a, dt in arrays]
    out = _ffi.DeviceArray((n,), np.float64)
    try:
        _ffi.tide_predict_dev(*(b.ptr for b in bufs[:3]), n, *(b.ptr for b in bufs[3:]), nc, nxs, nys, sub.grid, sub.ids, out.ptr)
        dev = out.download()
        _ffi.tide_predict_dev(*(b.ptr for b in bufs[:3]), 0, *(b.ptr for b in bufs[3:]), nc, nxs, nys, sub.grid, sub.ids, out.ptr)      # n = 0: nothing
        assert np.array_equal(out.download(), dev, equal_nan=True)
    finally:
        for b in bufs + [out]:
            b.free()
    assert np.array_equal(dev, host, equal_nan=True) and np.isnan(host).any() and not np.isnan(host).all()


def test_library_refuses_bad_tables_and_marks_points_outside_the_subset(model):
    sub = M.load_subset(model, ['m2'], [10.0], [10.0])
    args = (sub.hre, sub.him, sub.wet, sub.grid)
    outside = _ffi.tide_predict([sub.lon0 - 1.0, 10.0, np.nan, 10.0], [10.0, sub.lat0 + 100.0, 10.0, 10.0], [0.0, 0.0, 0.0, np.inf], *args, [0])
    assert np.isnan(outside).all()
    for ids, grid in (([14], sub.grid), ([-1], sub.grid), ([0], [0.0, 0.0, 0.0, 5.0]), ([0], [0.0, 5.0, np.nan, 5.0])):
        with pytest.raises(_ffi.P3DError):
            _ffi.tide_predict([10.0], [10.0], [0.0], sub.hre, sub.him, sub.wet, grid, ids)
    with pytest.raises(_ffi.P3DError):
        _ffi.tide_predict([10.0], [10.0], [0.0], sub.hre[:, :1], sub.him[:, :1], sub.wet[:1], sub.grid, [0])


def test_points_on_the_first_and_last_row_and_column_of_hand_cut_tables():
    """Tables cut by hand, without the one-node margin of ``load_subset``: 4 x 3 nodes at 50 ... 65 degrees east, -40 ... -30 north (exact in
    binary), one of them dry.  Points on every edge and corner of the tables, and within the kernel's 1e-9 of a cell outside them, against the helper;
    points further outside are NaN."""
    names = H.CONSTITUENTS[:8]
    _, _, fields, _ = H.model_fields(constituents=names)
    i0, j0, nxs, nys = 9, 10, 4, 3
    hre = np.array([fields[c][0][i0:i0 + nxs, j0:j0 + nys] for c in names])
    him = np.array([fields[c][1][i0:i0 + nxs, j0:j0 + nys] for c in names])
    wet = np.ones((nxs, nys), np.uint8)
    wet[1, 1] = 0
    grid = lon0, dlon, lat0, dlat = 50.0, 5.0, -40.0, 5.0
    east, north, tiny = lon0 + (nxs - 1) * dlon, lat0 + (nys - 1) * dlat, 2e-9                # tiny: 4e-10 of a cell
    lon = np.array([lon0, lon0, east, east, lon0, east, 57.0, 57.0, 61.3, 64.9, lon0 - tiny, east + tiny, 52.0, 63.0, east, east])
    lat = np.array([lat0, north, lat0, north, -33.0, -38.5, lat0, north, north, north, -36.0, -31.0, lat0 - tiny, north + tiny, -35.0, north - 1e-7])
    t = np.linspace(-2.0e8, 1.3e9, lon.size).round()
    ids = [H.CONSTITUENTS.index(c) for c in names]
    got = _ffi.tide_predict(lon, lat, t, hre, him, wet, grid, ids)
    want = H.predict(lon, lat, t, hre, him, wet.astype(bool), *grid, names)
    print(f'edges: worst {np.abs(got - want).max():.3e} m')
    assert np.isfinite(want).all() and np.abs(got - want).max() <= TOL_M
    corner = _ffi.tide_predict([east], [north], [0.0], hre, him, wet, grid, ids)              # the last node itself: weight 1 on it alone
    alone = H.predict([lon0 + dlon], [lat0 + dlat], [0.0], hre[:, -2:, -2:], him[:, -2:, -2:], np.array([[False, False], [False, True]]),
                      lon0, dlon, lat0, dlat, names)
    assert abs(corner[0] - alone[0]) <= TOL_M
    beyond = 1e-6
    outside = _ffi.tide_predict([lon0 - beyond, east + beyond, 55.0, 55.0], [-35.0, -35.0, lat0 - beyond, north + beyond], [0.0] * 4, hre, him, wet, grid, ids)
    assert np.isnan(outside).all()


CASES = json.loads(str(G['comp/cases']))


def test_compensate_tide_equals_the_reference():
    shapes = set()
    for k, case in enumerate(CASES):
        ns, ntr = case['ns'], case['ntr']
        data = (1 + np.arange(ns)[:, None] + 1000 * np.arange(ntr)[None, :]).astype(np.float32)
        before = data.copy()
        got = T.compensate_tide(data, G[f'comp/{k}/tide'], case['dt'], tide_units=case['tide_units'], units=case['units'], verbosity=0)
        want = G[f'comp/{k}/out']
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), case
        assert np.array_equal(data, before)
        shapes.add((ns, ntr))
    assert len(CASES) == 72 and len(shapes) == 9
    data = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert not T.compensate_tide(data, [4, -4, 1000], 1.0, tide_units='samples').any()          # |offset| >= ns: zeros
    assert np.array_equal(T.compensate_tide(data, [0.6, -0.6, 0.4], 1.0, tide_units='samples'), H.shift_section(data, [1, -1, 0]))
    with pytest.raises(ValueError, match='unknown unit'):
        T.compensate_tide(data, [0, 0, 0], 1.0, tide_units='feet')
    with pytest.raises(ValueError, match='non-finite'):
        T.compensate_tide(data, [0, np.nan, 0], 1.0)
