"""Step 5 on the GPU against the reference's recorded stages (tests/golden/static.npz): live mask, threshold, first crossings, baseline, peak
picks, final index and static_samples of every case are EQUAL to the fixture (the threshold within 1e-5, the margin the fixture's generator
asserts); the shift is bit-equal to NumPy."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import static_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import static as st  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'static.npz'))
CASES = [str(c) for c in G['cases']]


def case(name):
    rec = {k.split('/', 2)[2]: G[k] for k in G.files if k.startswith(f'case/{name}/')}
    rec['params'] = json.loads(str(rec['params']))
    return rec


def case_section(c):
    """(section samples x traces, nso or None, leading zeros per trace)"""
    data = G['section/' + c['params']['section']]
    if not c['params']['padded']:
        return data, None, np.zeros(data.shape[1], int)
    start, extra = G['pad/start'], int(G['pad/extra'])
    padded = np.zeros((data.shape[0] + extra, data.shape[1]), np.float32)
    for k, s in enumerate(start):
        padded[s:s + data.shape[0], k] = data[:, k]
    return padded, data.shape[0], start


@pytest.mark.parametrize('name', CASES)
def test_every_stage_equals_the_reference(name):
    c = case(name)
    data, nso, start = case_section(c)
    before = data.copy()
    stages = st.seafloor_stages(data, nso=nso, **c['params']['detect'])
    live = c['live']
    print(name, 'threshold', stages['threshold'], 'fixture', float(c['threshold']), 'raw differ', int(np.sum(stages['raw'] != c['raw'])),
          'peak differ', int(np.sum(stages['peak'] != c['peak'])), 'idx differ', int(np.sum(stages['idx'] != c['idx_amp'])))
    assert np.array_equal(data, before)
    assert stages['live'].shape == live.shape and np.array_equal(stages['live'], live) and live.sum() == live.size - 2
    assert (stages['nsta'], stages['nlta']) == tuple(int(v) for v in c['nsta_nlta'])
    assert abs(stages['threshold'] - c['threshold']) <= 1e-5 * c['threshold']
    assert stages['raw'].shape == c['raw'].shape and np.array_equal(stages['raw'], c['raw'])
    assert np.array_equal(stages['baseline'], c['baseline'])
    assert stages['peak'].shape == c['peak'].shape and np.array_equal(stages['peak'], c['peak'])
    assert stages['idx'].shape == c['idx_amp'].shape and np.array_equal(stages['idx'], c['idx_amp'])
    assert np.array_equal(stages['start'][live], start[live])
    idx = st.detect_seafloor_reflection(data, nso=nso, **c['params']['detect'])
    assert np.array_equal(idx, c['idx_amp'])
    static = st.get_static(idx + start if nso is not None else idx, **c['params']['static'])
    shifted, samples = st.compensate_static(data, static, dt=0.25, units='ms')
    assert samples.dtype == np.int32 and np.array_equal(samples, c['static_samples']) and np.count_nonzero(samples) >= 0.05 * samples.size
    assert shifted.dtype == np.float32 and shifted.tobytes() == H.compensate_static(data, samples).tobytes()
    assert np.array_equal(data, before)


def test_trace_major_is_the_transpose():
    c = case('B')
    data = G['section/B']
    section = np.ascontiguousarray(data.T)
    a = st.seafloor_stages(section, trace_major=True, **c['params']['detect'])
    assert np.array_equal(a['idx'], c['idx_amp']) and np.array_equal(a['raw'], c['raw'])
    up, s1 = st.compensate_static(section, c['static'], trace_major=True)
    down, s2 = st.compensate_static(data, c['static'])
    assert np.array_equal(s1, s2) and up.shape == section.shape and np.array_equal(up.T, down)
    assert np.array_equal(section.T, data)
    with_threshold = st.seafloor_stages(data, threshold=float(c['threshold']), **c['params']['detect'])
    assert np.array_equal(with_threshold['idx'], c['idx_amp'])
    flat = st.detect_seafloor_reflection(data, **dict(c['params']['detect'], win=0))
    x = np.arange(c['live'].size)
    assert np.array_equal(flat[c['live']], st.filter_interp_1d(np.interp(x, x[c['live']], c['baseline']).astype('int'), win=7, threshold=3).astype('int')[c['live']])


@pytest.mark.parametrize('ns,ntr', [(37, 19), (64, 5), (1, 3), (255, 130), (1024, 33)])
def test_shift_is_bit_equal_to_numpy(ns, ntr):
    rng = np.random.default_rng(ns * 1000 + ntr)
    data = rng.standard_normal((ns, ntr)).astype(np.float32)
    special = [0, 1, -1, ns - 1, -(ns - 1), ns, -ns, ns + 5, -(ns + 5), 2, -3, 4, -4, 7, 2**31 - 1, -2**31]
    shift = np.array([special[k % len(special)] if k < len(special) else rng.integers(-ns - 2, ns + 3) for k in range(ntr)], dtype=np.int64)
    before = data.copy()
    got, samples = st.compensate_static(data, shift.astype(np.float64))
    assert np.array_equal(samples, shift.astype(np.int32)) and got.tobytes() == H.compensate_static(data, shift).tobytes()
    assert np.array_equal(data, before)
    low = _ffi.static_shift(np.ascontiguousarray(data.T), shift.astype(np.int32))
    assert low.tobytes() == np.ascontiguousarray(got.T).tobytes()
    half, _ = st.compensate_static(data, np.full(ntr, 0.4))
    assert np.array_equal(half, data)


def test_host_entry_points_and_windows():
    c = case('A')
    data = G['section/A']
    section = np.ascontiguousarray(data.T)
    nsta, nlta = (int(v) for v in c['nsta_nlta'])
    first, thr, cross = _ffi.static_detect(section, nsta, nlta)
    live = c['live']
    assert np.array_equal(first >= 0, live) and abs(thr - c['threshold']) <= 1e-5 * c['threshold'] and np.array_equal(cross[live], c['raw'])
    assert not cross[~live].any() and np.array_equal(first, H.first_nonzero(data))
    _, thr2, cross2 = _ffi.static_detect(section, nsta, nlta, threshold=thr)
    assert thr2 == thr and np.array_equal(cross2, cross)
    base = np.zeros(live.size, np.int32)
    base[live] = c['baseline']
    for win, n in ((30, 5), (30, 1), (30, 61), (3, 2), (100, 7), (255, 5), (200, 40)):
        got = _ffi.static_peak(section, first, base, win, n)
        want = H.peaks(data, first, base, win, n)
        assert np.array_equal(got, want), (win, n)
    assert np.array_equal(_ffi.static_peak(section, first, base, 30, 5)[live], c['peak'])
    # windows clipped at either end of the trace, and a slice that starts inside the trace
    edge = base.copy()
    edge[live] = np.where(np.arange(live.sum()) % 2 == 0, 3, data.shape[0] - 2)
    assert np.array_equal(_ffi.static_peak(section, first, edge, 30, 5), H.peaks(data, first, edge, 30, 5))
    c2 = case('A-pad')
    start, extra = G['pad/start'], int(G['pad/extra'])
    padded = np.zeros((live.size, data.shape[0] + extra), np.float32)
    for k, s in enumerate(start):
        padded[k, s:s + data.shape[0]] = data[:, k]
    pfirst, pthr, pcross = _ffi.static_detect(padded, nsta, nlta, nvalid=data.shape[0])
    assert np.array_equal(pfirst[live], start[live]) and np.array_equal(pcross[live], c2['raw']) and abs(pthr - thr) <= 1e-12 * thr
    assert np.array_equal(_ffi.static_peak(padded, pfirst, base, 30, 5, nvalid=data.shape[0])[live], c2['peak'])


def test_refusals_happen_on_the_host():
    section = np.ones((4, 600), np.float32)
    first = np.zeros(4, np.int32)
    with pytest.raises(_ffi.UnsupportedError):
        _ffi.static_peak(section, first, first + 300, _ffi.STATIC_MAX_WIN + 1, 5)
    with pytest.raises(_ffi.UnsupportedError):
        _ffi.static_peak(section, first, first + 300, 2, 6)
    with pytest.raises(ValueError):
        _ffi.static_peak(section, first, first + 300, 0, 1)
    with pytest.raises(_ffi.UnsupportedError):
        _ffi.static_detect(np.ones((2, 20000), np.float32), 3, _ffi.STATIC_MAX_NLTA + 1)
    with pytest.raises(ValueError):
        _ffi.static_detect(section, 5, 3)
    with pytest.raises(ValueError):
        _ffi.static_detect(section, 3, 50, nvalid=601)
    with pytest.raises(ValueError, match='2D'):
        st.detect_seafloor_reflection(np.ones(10, np.float32))
    with pytest.raises(ValueError, match='only zero traces'):
        st.detect_seafloor_reflection(np.zeros((200, 8), np.float32))
    with pytest.raises(ValueError, match='long window'):
        st.detect_seafloor_reflection(np.ones((40, 8), np.float32))
    with pytest.raises(ValueError):
        st.compensate_static(np.ones((40, 8), np.float32), np.zeros(7))
    assert _ffi.static_detect(np.ones((2, 9000), np.float32), 3, _ffi.STATIC_MAX_NLTA)[2].tolist() == [0, 0]
