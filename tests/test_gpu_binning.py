"""Step-10 trace stacking on the GPU (p3d_bin_stack / p3d_bin_stack_dev): the four methods against the reference's own stacked bins
(golden/binning.npz) and against the NumPy restatement on random CSR layouts (folds 0 ... 300, offsets before, inside and past the
window, lengths that differ per trace); chunked, repeated and device-buffer runs are bitwise equal."""
import os

import numpy as np
import pytest

from helpers.binning_numpy import bin_stack as np_bin_stack
from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import binning as B

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'binning.npz'))


def _golden_tables(method):
    folds, lengths = GOLD['stack/folds'], GOLD['stack/lengths']
    twt, dt = GOLD['stack/twt'], float(GOLD['stack/dt'])
    bid = np.repeat(np.arange(folds.size), folds)
    off = np.r_[0, np.cumsum(lengths)[:-1]]
    shift = B.trace_shifts(GOLD['stack/delays'], twt[0], dt)
    dist = GOLD['stack/dist']
    sel, weight = np.arange(bid.size), None
    if method == 'nearest':
        sel = B.nearest_per_bin(dist, bid)
    elif method == 'IDW':
        weight = B.idw_weights(dist, bid, float(GOLD['stack/factor']))
    bs = np.r_[0, np.cumsum(np.bincount(bid[sel], minlength=folds.size))]
    return GOLD['stack/samples'], off[sel], lengths[sel], shift[sel], bs, twt.size, weight


@pytest.mark.parametrize('method', ['average', 'median', 'nearest', 'IDW'])
def test_against_reference_stacks(method):
    smp, off, ln, sh, bs, nt, w = _golden_tables(method)
    got = _ffi.bin_stack(smp, off, ln, sh, bs, 1, bs.size - 1, nt, method=method, weight=w)[:, 0, :].T
    want = GOLD[f'stack/{method}']
    if method in ('median', 'nearest'):
        np.testing.assert_array_equal(got, want)
    else:
        for b in range(want.shape[0]):
            assert np.abs(got[b] - want[b]).max() <= 1e-6 * np.abs(want[b]).max(), b


def random_case(seed, nil=5, nxl=70, nt=300, maxfold=300):
    rng = np.random.default_rng(seed)
    nb = nil * nxl
    fold = np.where(rng.random(nb) < 0.35, 0, rng.integers(1, 9, nb))
    fold[rng.choice(nb, 4, replace=False)] = [17, 40, 255, maxfold]          # the radix path and fold > 255
    fold[rng.choice(nb, 3, replace=False)] = [9, 12, 16]                      # the 16-wide network
    ntr = int(fold.sum())
    ln = rng.integers(1, 2 * nt, ntr).astype(np.int32)
    ln[rng.random(ntr) < 0.05] = 0
    sh = rng.integers(-nt, nt, ntr).astype(np.int32)
    sh[rng.random(ntr) < 0.05] = nt + 5                                      # wholly below the window
    sh[rng.random(ntr) < 0.05] = -3 * nt                                     # wholly above it
    off = np.r_[0, np.cumsum(ln)[:-1]].astype(np.int64)
    smp = rng.standard_normal(int(ln.sum())).astype(np.float32)
    smp[rng.random(smp.size) < 0.02] = 0.0
    smp[rng.random(smp.size) < 0.05] = np.float32(0.5)                        # ties for the median
    bs = np.r_[0, np.cumsum(fold)].astype(np.int64)
    bid = np.repeat(np.arange(nb), fold)
    dist = rng.uniform(0, 10, ntr)
    dist[rng.random(ntr) < 0.02] = 0.0
    w = B.idw_weights(dist, bid, 2.0) if ntr else np.zeros(0)
    return smp, off, ln, sh, bs, nil, nxl, nt, w


@pytest.mark.parametrize('method', ['average', 'median', 'nearest', 'IDW'])
def test_random_against_numpy(method):
    smp, off, ln, sh, bs, nil, nxl, nt, w = random_case(1)
    got = _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w)
    want = np_bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w)
    if method in ('median', 'nearest'):
        np.testing.assert_array_equal(got, want)
    else:
        peak = np.abs(want).max(axis=0, keepdims=True)
        assert np.all(np.abs(got - want) <= 1e-6 * peak)
    empty = (bs[1:] == bs[:-1]).reshape(nil, nxl)
    assert not got[:, empty].any()


def test_idw_zero_distance():
    smp = np.float32([1, 1, 1, 1, 2, 2, 2, 2, 7, 7, 7, 7])
    off, ln, sh = np.array([0, 4, 8]), np.array([4, 4, 4]), np.array([0, 0, 0])
    w = B.idw_weights(np.array([0.0, 0.0, 3.0]), np.array([0, 0, 0]), 1.0)
    np.testing.assert_array_equal(w, [0.5, 0.5, 0.0])
    got = _ffi.bin_stack(smp, off, ln, sh, np.array([0, 3]), 1, 1, 4, method='IDW', weight=w)
    np.testing.assert_array_equal(got.ravel(), np.float32([1.5] * 4))


@pytest.mark.parametrize('method', ['average', 'median', 'IDW'])
def test_chunked_and_repeated_runs_bitwise(method):
    smp, off, ln, sh, bs, nil, nxl, nt, w = random_case(2, nil=9, nxl=40, nt=200, maxfold=60)
    full = _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w)
    again = _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w)
    one_inline = nt * nxl * 4 + 8 * (nxl + 1)
    per_il = [int(ln[bs[i * nxl]:bs[(i + 1) * nxl]].sum()) for i in range(nil)]
    cap = 2 * one_inline + 4 * max(per_il) * 2 + 24 * int(np.diff(bs[::nxl]).max()) * 2
    chunked = _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w, max_bytes=cap)
    assert full.tobytes() == again.tobytes() == chunked.tobytes()
    with pytest.raises(_ffi.UnsupportedError):
        _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=method, weight=w, max_bytes=1000)


def test_device_buffer_variant():
    smp, off, ln, sh, bs, nil, nxl, nt, w = random_case(3, nil=3, nxl=50, nt=150, maxfold=30)
    host = {m: _ffi.bin_stack(smp, off, ln, sh, bs, nil, nxl, nt, method=m, weight=w) for m in ('median', 'IDW')}
    bufs = [_ffi.DeviceArray(a.shape, a.dtype).upload(a) for a in (smp, off, ln.astype(np.int32), sh.astype(np.int32), w, bs)]
    out = _ffi.DeviceArray((nt, nil, nxl), np.float32)
    try:
        for m in ('median', 'IDW'):
            _ffi.bin_stack_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[5].ptr, out.ptr, nil, nxl, nt, method=m,
                               weight=bufs[4].ptr)
            assert out.download().tobytes() == host[m].tobytes()
    finally:
        for b in bufs + [out]:
            b.free()
