"""The step-3 / step-4 kernels (csrc/p3d_delrt.hip) on the GPU, bit for bit: the pad kernel against the reference's pad_trace_data (fixtures:
tests/golden/delrt.npz) and against the NumPy restatement (tests/helpers/delrt_numpy.py) on the smallest shapes at which it can go wrong; the
window kernel against what the reference saw on the section fixtures and against the restatement over window sizes, trace lengths around the
256-sample chunk, one and forty changes per launch, packed and resident."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import delrt_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import delrt as D  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'delrt.npz'))


def pad_input(ns, ntr):
    data = G['pad/section'][:ns, :ntr].copy()
    data[-1] = np.where(data[-1] == 0, 1 / 512, data[-1])
    return data


@pytest.mark.parametrize('name', [str(n) for n in G['pad/cases']])
def test_pad_trace_data_equals_the_reference(name):
    c = {k: G[f'pad/{name}/{k}'] for k in ('delays', 'ns', 'dt', 'data_padded', 'twt_padded', 'n_samples_padded', 'idx_delay', 'min_delay', 'max_delay')}
    ns, dt = int(c['ns']), float(c['dt'])
    data = pad_input(ns, c['delays'].size)
    twt = np.arange(ns) * dt + c['delays'][0]
    padded, twt_padded, n_padded, (idx_delay, dmin, dmax) = D.pad_trace_data(data, c['delays'], c['delays'].size, dt, twt)
    assert padded.dtype == np.float32 and padded.shape == c['data_padded'].shape and padded.tobytes() == c['data_padded'].tobytes()
    assert twt_padded.tobytes() == c['twt_padded'].tobytes() and n_padded == int(c['n_samples_padded'])
    assert np.array_equal(idx_delay, c['idx_delay']) and dmin == c['min_delay'] and dmax == c['max_delay']
    major, *_ = D.pad_trace_data(np.ascontiguousarray(data.T), c['delays'], c['delays'].size, dt, twt, trace_major=True)
    assert major.tobytes() == np.ascontiguousarray(c['data_padded'].T).tobytes()


# ntr x ns_in -> ns_out, top: one trace of one sample; sections whose length is no multiple of 4 (5, 21); every residue of top mod 4 with quads that
# straddle traces (397, 521 odd); no shift at all (aligned 16-byte loads throughout); more than one workgroup (7 x 521 = 3647 floats)
PAD_SHAPES = [
    (1, 1, 1, [0]),
    (1, 3, 5, [2]),
    (3, 5, 7, [0, 1, 2]),
    (7, 397, 521, [0, 1, 2, 3, 124, 60, 121]),
    (5, 256, 256, [0, 0, 0, 0, 0]),
    (4, 8, 12, [4, 3, 0, 1]),
]


@pytest.mark.parametrize('ntr,ns_in,ns_out,top', PAD_SHAPES)
def test_pad_kernel_equals_numpy(ntr, ns_in, ns_out, top):
    rng = np.random.default_rng(ntr * 1000 + ns_in)
    data = (rng.integers(1, 100, (ns_in, ntr)) / 64).astype(np.float32)        # no zero sample: every misplaced one shows
    want = np.ascontiguousarray(H.pad(data, top, ns_out).T)
    section = np.ascontiguousarray(data.T)
    assert {t % 4 for _, _, _, tt in PAD_SHAPES for t in tt} == {0, 1, 2, 3}
    got = _ffi.delrt_pad(section, top, ns_out)
    assert got.dtype == np.float32 and got.shape == (ntr, ns_out) and got.tobytes() == want.tobytes()
    din, dtop, dout = _ffi.DeviceArray((ntr, ns_in), np.float32), _ffi.DeviceArray((ntr,), np.int32), _ffi.DeviceArray((ntr, ns_out), np.float32)
    try:
        din.upload(section)
        dtop.upload(np.array(top, np.int32))
        dout.upload(np.full((ntr, ns_out), 7, np.float32))                    # every output sample is written, the zeros too
        _ffi.delrt_pad_dev(din.ptr, ntr, ns_in, ns_out, dtop.ptr, dout.ptr)
        assert dout.download().tobytes() == want.tobytes()
    finally:
        for buf in (din, dtop, dout):
            buf.free()


@pytest.mark.parametrize('top,text', [([0, -1, 0], 'trace 1: -1 samples of top padding'), ([0, 0, 3], 'trace 2: 3 samples of top padding and 5 samples do not fit')])
def test_pad_refuses_a_bad_top_before_any_launch(top, text):
    section = np.ones((3, 5), np.float32)
    with pytest.raises(_ffi.P3DError) as e:
        _ffi.delrt_pad(section, top, 7)
    assert e.value.code == _ffi.P3D_ERR_INVALID and text in str(e.value)
    assert text in _ffi.lib().p3d_last_error().decode()
    din, dtop, dout = _ffi.DeviceArray((3, 5), np.float32), _ffi.DeviceArray((3,), np.int32), _ffi.DeviceArray((3, 7), np.float32)
    try:
        din.upload(section)
        dtop.upload(np.array(top, np.int32))
        dout.upload(np.full((3, 7), 7, np.float32))
        with pytest.raises(_ffi.P3DError) as e:
            _ffi.delrt_pad_dev(din.ptr, 3, 5, 7, dtop.ptr, dout.ptr)
        assert e.value.code == _ffi.P3D_ERR_INVALID and text in str(e.value) and len(_ffi.lib().p3d_last_error()) > 0
        assert np.all(dout.download() == 7)                                   # nothing was launched
    finally:
        for buf in (din, dtop, dout):
            buf.free()
    with pytest.raises(_ffi.P3DError):
        _ffi.delrt_pad(section, [0, 0, 0], 4)                                 # an output trace shorter than the input trace


@pytest.mark.parametrize('name', [str(n) for n in G['section/cases']])
def test_window_kernel_and_full_path_equal_the_reference(name):
    data, delrt = G[f'section/{name}/data'], G[f'section/{name}/delrt']
    n_traces, n_samples = (int(v) for v in G[f'section/{name}/window'])
    c = {k: G[f'section/{name}/{k}'] for k in ('idx', 'width', 'peak_idx', 'peak_val', 'maxima', 'kind', 'delay', 'index')}
    section = np.ascontiguousarray(data.T)
    width = 2 * n_traces + 1
    for k, idx in enumerate(c['idx'].tolist()):
        lo, w = idx - n_traces, int(c['width'][k])
        rows = np.minimum(np.arange(lo, lo + width), lo + w - 1)              # a subset one trace short: filled up with its last trace
        peak_idx, peak_val, maxima = _ffi.delrt_windows(section[rows][None], n_samples)
        assert peak_idx.tolist() == [c['peak_idx'][k]] and peak_val.tobytes() == c['peak_val'][k:k + 1].tobytes()
        clipped = np.minimum(maxima[0], maxima[0, n_traces])[:w]
        assert clipped.tobytes() == c['maxima'][k, :w].tobytes()
        if w == width:                                                        # the reference's own signature
            got = D.correct_single_trace_DelayRecordingTime(idx, data[:, lo:lo + width], delrt[lo:lo + width], np.arange(width), n_traces, n_samples)
            assert got == ((None, None) if c['kind'][k] == 0 else (c['delay'][k], c['index'][k]))
    fixes = D.correct_delay_changes(section, delrt, n_traces, n_samples)
    want = [(int(i), int(i) - n_traces + int(x), int(delrt[int(i) - n_traces + int(x)]), int(d))
            for i, kind, d, x in zip(c['idx'], c['kind'], c['delay'], c['index']) if kind == 1]
    assert [tuple(int(v) for v in f) for f in fixes] == want


@pytest.mark.parametrize('ns', [5, 255, 256, 257, 1000])
def test_window_kernel_equals_numpy_packed_and_resident(ns):
    """Integer-valued samples from a small range: every trace holds its maximum several times, so the FIRST index has to win within a lane, across
    the lanes of a wave and across the waves."""
    rng = np.random.default_rng(ns)
    ntr = 64
    data = rng.integers(-6, 7, (ns, ntr)).astype(np.float32)
    data[:, 20] = -np.abs(data[:, 20]) - 1                                    # an all-negative trace, with 9 neighbours to either side as is 40
    data[:, 40] = 0                                                           # an all-zero one
    section = np.ascontiguousarray(data.T)
    dsec = _ffi.DeviceArray((ntr, ns), np.float32).upload(section)
    try:
        for n_traces in (1, 5, 9):
            for n_samples in (1, 7, 120):
                for m in (1, 40):
                    ref = rng.integers(n_traces, ntr - n_traces, m).astype(np.int32)
                    if m == 40:
                        ref[:4] = [n_traces, ntr - 1 - n_traces, 40, 20]      # both ends of the section; the zero and the negative trace as reference
                    want = H.windows(data, ref, n_traces, n_samples)
                    rows = (ref[:, None] + np.arange(-n_traces, n_traces + 1)[None, :])
                    packed = _ffi.delrt_windows(section[rows], n_samples)
                    dres = [_ffi.DeviceArray((m,), np.int32), _ffi.DeviceArray((m,), np.float32), _ffi.DeviceArray((m, 2 * n_traces + 1), np.float32)]
                    try:
                        _ffi.delrt_windows_dev(dsec.ptr, ntr, ns, ref, n_traces, n_samples, *(b.ptr for b in dres))
                        resident = [b.download() for b in dres]
                    finally:
                        for b in dres:
                            b.free()
                    for got in (packed, resident):
                        for g, w in zip(got, want):
                            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (n_traces, n_samples, m)
    finally:
        dsec.free()


def test_windows_refuses_a_reference_trace_without_neighbours():
    section = np.ones((8, 16), np.float32)
    dsec = _ffi.DeviceArray((8, 16), np.float32).upload(section)
    dres = [_ffi.DeviceArray((1,), np.int32), _ffi.DeviceArray((1,), np.float32), _ffi.DeviceArray((1, 5), np.float32)]
    try:
        for ref in (1, 6):
            with pytest.raises(_ffi.P3DError) as e:
                _ffi.delrt_windows_dev(dsec.ptr, 8, 16, [ref], 2, 4, *(b.ptr for b in dres))
            assert e.value.code == _ffi.P3D_ERR_INVALID and 'fewer than 2 neighbours' in str(e.value)
    finally:
        for b in [dsec] + dres:
            b.free()
    with pytest.raises(ValueError):
        _ffi.delrt_windows(np.ones((1, 4, 16), np.float32), 4)                # an even number of traces has no middle one
    empty = _ffi.delrt_windows(np.ones((0, 5, 16), np.float32), 4)
    assert [a.shape for a in empty] == [(0,), (0,), (0, 5)]
