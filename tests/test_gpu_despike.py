"""Step 8 on the GPU (csrc/p3d_despike.hip through functions/despike.py) against the fixtures recorded from the reference's own despike_2D
(tests/golden/despike.npz) and against the NumPy restatement (tests/helpers/despike_numpy.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import despike_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import despike as D  # noqa: E402

pytestmark = pytest.mark.gpu
G = load_golden('despike.npz')
CASES = [str(c) for c in G['cases']]


def parse(name):
    sec, window, ov, w, mode, thr, out = name.split('-')
    return G['section/' + sec], dict(window=int(window), dt=1.0, overlap=int(ov), ntraces=int(w), mode=mode, threshold=int(thr), out=out)


def near_tie(a, w, mode, thr, flat):
    """Is sample ``flat`` of section a [ns][ntr] within the float32 summation-order bound of its deciding comparison?"""
    t, x = divmod(int(flat), a.shape[1])
    absa = np.abs(a[t].astype(np.float64))
    ms = [{'mean': np.mean, 'median': np.median, 'rms': lambda v: np.sqrt(np.mean(v**2))}[mode](absa[j:j + w])
          for j in range(max(0, x - w + 1), min(x, a.shape[1] - w) + 1)]
    return any(abs(absa[x] - thr * m) <= w * 2.0**-23 * max(absa[x], thr * m) for m in ms)


@pytest.mark.parametrize('name', CASES)
def test_reference_fixture(name):
    a, kw = parse(name)
    idx, val = G[f'case/{name}/idx'], G[f'case/{name}/val']
    got = D.despike_2D(a, **kw)
    if idx.size == 0:
        assert got is a                                         # nothing detected: the input itself comes back
        return
    assert got.shape == a.shape and got.dtype == np.float32
    zeros = D.despike_2D(a, **dict(kw, out='zeros'))
    written = np.flatnonzero(zeros != a)                        # (the sections hold no exact zeros)
    w, mode = kw['ntraces'], kw['mode']
    if mode == 'median' or w <= 7:
        np.testing.assert_array_equal(written, idx)
    else:
        for flat in np.setxor1d(written, idx):
            assert near_tie(a, w, mode, kw['threshold'], flat), (name, flat)
    untouched = np.ones(a.size, bool)
    untouched[written] = False
    assert got.ravel()[untouched].tobytes() == a.ravel()[untouched].tobytes()
    if np.array_equal(written, idx):
        g = got.ravel()[idx]
        if kw['out'] in ('zeros', 'median'):
            assert g.tobytes() == val.tobytes()
        else:
            err = rel_l2(g, val)
            print(f'{name}: rel-L2 over {idx.size} replaced samples {err:.3e}')
            assert err < 1e-5


def test_levels_matter_on_the_interacting_fixture():
    name = 'spiky-110-10-5-mean-3-median'
    a, kw = parse(name)
    idx, val = G[f'case/{name}/idx'], G[f'case/{name}/val']
    sec = np.ascontiguousarray(a.T)
    M, dy, main_end, add_start = D.window_rows(a.shape[0], kw['window'], 1.0, kw['overlap'])
    mask, counts = _ffi.despike_detect(sec, 5, 'mean', 3, main_end, add_start)
    rec = D.spikes_from_mask(mask, counts, a.shape[0], M, main_end, add_start, 5)
    lev = D.assign_levels(rec)
    assert lev.max() >= 1
    good = _ffi.despike_replace(sec, *D.order_by_level(rec, lev), 'mean', 'median', 3).T
    assert good.ravel()[idx].tobytes() == val.tobytes()
    # every spike forced to level 0, i.e. one launch (records in reverse order, so that a spike is dispatched before the ones it should
    # have waited for): the interacting spikes read the untouched section, which is NOT what the reference computes -- the fixture bites.
    # tests/test_despike_host.py shows the same on the CPU without relying on how the workgroups of one launch are scheduled.
    flat = _ffi.despike_replace(sec, rec[::-1].copy(), np.array([0, rec.shape[0]], np.int32), 'mean', 'median', 3).T
    assert flat.ravel()[idx].tobytes() != val.tobytes()


def planted(seed, ns, ntr, spikes, amp=30.0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((ns, ntr)).astype(np.float32)
    a[a == 0] = np.float32(0.01)
    for x, r0, r1 in spikes:
        a[r0:r1, x] = (amp * (1 + 0.1 * rng.random(r1 - r0)) * rng.choice([-1.0, 1.0], r1 - r0)).astype(np.float32)
    return a


KW = dict(window=100, dt=1.0, overlap=10, ntraces=5, mode='mean', threshold=3)


@pytest.mark.parametrize('out', ['zeros', 'median', 'threshold'])
def test_left_edge_replaces_the_spikes_own_trace(out):
    a = planted(1, 300, 60, [(0, 30, 60), (1, 100, 130), (30, 200, 230)])
    want, spikes = H.despike_2D(a, out=out, return_spikes=True, **KW)
    assert {x for x, *_ in spikes} >= {0, 1, 30}
    got = D.despike_2D(a, out=out, **KW)
    changed = np.nonzero((got != a).any(axis=0))[0]
    assert set(changed) == {0, 1, 30}                           # (the reference would have rewritten trace 2 twice instead of 0 and 1)
    if out == 'threshold':
        assert rel_l2(got, want) < 1e-5
    else:
        assert got.tobytes() == want.tobytes()


def test_splits_and_narrow_split_passes_through():
    a = planted(2, 300, 90, [(10, 30, 60), (39, 100, 130), (40, 110, 140), (43, 50, 80), (60, 200, 230)])
    splits = [40, 44]                                           # 0:40, 40:44 (narrower than the window), 44:90
    want, spikes = H.despike_2D(a, out='median', splits=splits, return_spikes=True, **KW)
    assert {x for x, *_ in spikes} == {10, 39, 60}
    with pytest.warns(RuntimeWarning, match='fewer than 5 traces'):
        got = D.despike_2D(a, out='median', splits=splits, **KW)
    assert got.tobytes() == want.tobytes()
    assert got[:, 40:44].tobytes() == a[:, 40:44].tobytes()
    whole = D.despike_2D(a, out='median', **KW)                 # without splits the windows cross trace 40: another result
    assert whole.tobytes() != got.tobytes()


@pytest.mark.parametrize('mode,thr', [('mean', 3), ('median', 6), ('rms', 3)])
def test_widest_window(mode, thr):
    a = planted(3, 300, 120, [(20, 30, 60), (70, 100, 130), (119, 200, 230)], amp=60.0)
    kw = dict(KW, ntraces=31, mode=mode, threshold=thr)
    want, spikes = H.despike_2D(a, out='zeros', return_spikes=True, **kw)
    assert len(spikes) >= 3
    got = D.despike_2D(a, out='zeros', **kw)
    if mode == 'median':
        assert got.tobytes() == want.tobytes()
    else:
        for flat in np.flatnonzero((got != a) != (want != a)):
            assert near_tie(a, 31, mode, thr, flat)
    with pytest.raises(_ffi.UnsupportedError, match='31'):
        D.despike_2D(a, out='zeros', **dict(kw, ntraces=33))
    with pytest.raises(_ffi.UnsupportedError, match='31'):
        _ffi.despike_detect(np.ascontiguousarray(a.T), 33, mode, thr, 280)


def test_device_buffers_equal_host_buffers():
    a = planted(4, 333, 70, [(10, 30, 60), (11, 40, 75), (69, 200, 230)])
    sec = np.ascontiguousarray(a.T)
    ntr, ns = sec.shape
    M, dy, main_end, add_start = D.window_rows(ns, 100, 1.0, 10)
    assert add_start is not None
    mask, counts = _ffi.despike_detect(sec, 5, 'rms', 2, main_end, add_start)
    bufs = [_ffi.DeviceArray(sec.shape, np.float32).upload(sec), _ffi.DeviceArray(mask.shape, np.uint64), _ffi.DeviceArray(counts.shape, np.int32)]
    try:
        _ffi.despike_detect_dev(bufs[0].ptr, ntr, ns, 5, 'rms', 2, main_end, add_start, bufs[1].ptr, bufs[2].ptr)
        assert bufs[1].download().tobytes() == mask.tobytes() and bufs[2].download().tobytes() == counts.tobytes()
        rec = D.spikes_from_mask(mask, counts, ns, M, main_end, add_start, 5)
        assert rec.shape[0] >= 3
        ordered, level_start = D.order_by_level(rec, D.assign_levels(rec))
        host = _ffi.despike_replace(sec, ordered, level_start, 'rms', 'scaled', 2)
        _ffi.despike_replace_dev(bufs[0].ptr, ntr, ns, ordered, level_start, 'rms', 'scaled', 2)
        assert bufs[0].download().tobytes() == host.tobytes()
        want = H.despike_2D(a, 100, 1.0, 10, 5, 'rms', 2, 'scaled')
        assert rel_l2(host.T[want != a], want[want != a]) < 1e-5
    finally:
        for b in bufs:
            b.free()


def test_wide_section():
    ntr, ns = 70016, 512
    rng = np.random.default_rng(5)
    sec = rng.standard_normal((ntr, ns)).astype(np.float32)
    sec[sec == 0] = np.float32(0.01)
    where = np.sort(rng.choice(np.arange(2, ntr - 2), 60, replace=False))
    where = np.r_[where, 66000, 69999, ntr - 1]
    for k, x in enumerate(where):
        r0 = 20 + (k * 37) % 400
        sec[x, r0:r0 + 40] = (30.0 * (1 + 0.1 * rng.random(40)) * rng.choice([-1.0, 1.0], 40)).astype(np.float32)
    kw = dict(window=128, dt=1.0, overlap=10, ntraces=5, mode='median', threshold=6, out='median')
    got = D.despike_2D(sec, trace_major=True, **kw)
    changed = np.nonzero((got != sec).any(axis=1))[0]
    assert set(where) <= set(changed)
    want = np.array(sec)
    for lo in range(0, ntr, 8192):                              # the helper on overlapping slabs (windows reach 4 traces, spikes read 2)
        s0, s1 = max(0, lo - 8), min(ntr, lo + 8192 + 8)
        part = H.despike_2D(sec[s0:s1].T, **kw).T
        want[lo:lo + 8192] = part[lo - s0:lo - s0 + min(8192, ntr - lo)]
    assert got.tobytes() == want.tobytes()
