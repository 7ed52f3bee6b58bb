"""Step 8: single-trace noise bursts of a 2-D section (mirror of the reference's despike_2D, despiking_2D_segy.py).

Detection and replacement run on the GPU (csrc/p3d_despike.hip) on the trace-major section, which is uploaded once and downloaded once; in
between only the packed candidate mask (1 / 32 of the data) and the per-trace counts come back, and the host finds the runs and orders the
spikes (`spikes_from_mask`, `assign_levels`).  DESIGN.md 3.8 has the algorithm and the departures from the reference."""
import warnings

import numpy as np

from .. import _ffi
from .utils import xprint

MODES = ['mean', 'rms', 'median']
REPLACE_AMP_MODES = ['scaled', 'mode', 'threshold', 'zeros', 'median']


def window_rows(ns, window, dt, overlap):
    """The time window of the reference in samples: ``M`` rows, step ``dy``, rows ``t < main_end`` of the main view and rows
    ``t >= add_start`` of the additional view (None when ``ns`` is a multiple of ``dy``: the tail is then never examined)."""
    M = int(window / dt)
    ov = np.around(overlap / 100 * M, 0)
    ov = ov if ov >= 1 else 1
    dy = int(M - ov)
    if M < 1 or dy < 1 or M > ns:
        raise ValueError(f'A time window of {M} samples (step {dy}) does not fit a section of {ns} samples.')
    main_end = ((ns - M) // dy) * dy + M
    add_start = ns - M if ns % dy != 0 else None
    return M, dy, main_end, add_start


def spikes_from_mask(mask, counts, ns, M, main_end, add_start, ntraces, bounds=None, chunk=1024):
    """Steps 3 and 4 on the detection kernel's output: the per-view count filter, then runs per trace.  Returns int32 records [n][8]
    (trace, lo, hi, first, last, c0, c1, 0) in the reference's order (trace, first sample); c0:c1 is the neighbour window clipped to
    the trace's split (``bounds``: ascending boundaries from 0 to ntr)."""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    ntr = mask.shape[0]
    bounds = np.asarray([0, ntr] if bounds is None else bounds, dtype=np.int64)
    keep_main = counts[0] > M * 0.1
    keep_add = counts[1] > M * 0.1 if add_start is not None else np.zeros(ntr, bool)
    rows = np.arange(ns)
    in_main = rows < main_end
    in_add = rows >= add_start if add_start is not None else np.zeros(ns, bool)
    h = ntraces // 2
    traces = np.nonzero(keep_main | keep_add)[0]
    records = []
    for c in range(0, traces.size, chunk):
        sel = traces[c:c + chunk]
        bits = np.unpackbits(mask[sel].view(np.uint8), axis=1, bitorder='little')[:, :ns].astype(bool)
        bits &= (keep_main[sel, None] & in_main[None, :]) | (keep_add[sel, None] & in_add[None, :])
        for x, row in zip(sel, bits):
            t = np.nonzero(row)[0]
            if t.size == 0:
                continue
            seg = np.searchsorted(bounds, x, side='right') - 1
            c0, c1 = max(int(bounds[seg]), int(x) - h), min(int(bounds[seg + 1]), int(x) + h + 1)
            for run in np.split(t, np.nonzero(np.diff(t) > M * 0.05)[0] + 1):
                if run.size > M * 0.05:
                    pad = int(run.size * 0.1)
                    first, last = int(run[0]), int(run[-1])
                    records.append((int(x), max(0, first - pad), min(ns, last + pad + 1), first, last, c0, c1, 0))
    return np.asarray(records, dtype=np.int32).reshape(-1, 8)


def assign_levels(records):
    """Level of every spike record (reference order): 0 if it neither reads what an earlier spike writes nor writes what an earlier
    spike reads, otherwise 1 + the highest level among those it interacts with.  Spikes of one level can be replaced in one launch,
    levels in ascending order reproduce the reference's sequential in-place replacement."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, 8)
    n = records.shape[0]
    levels = np.zeros(n, np.int32)
    x, lo, hi, c0, c1 = records[:, 0], records[:, 1], records[:, 2], records[:, 5], records[:, 6]
    reach = int((c1 - c0).max()) if n else 0
    start = np.searchsorted(x, x - reach, side='left')          # records are sorted by trace: earlier spikes that can interact
    for i in range(n):
        j = np.arange(start[i], i)
        if j.size == 0:
            continue
        touch = (lo[j] < hi[i]) & (lo[i] < hi[j]) & (((x[j] >= c0[i]) & (x[j] < c1[i])) | ((x[i] >= c0[j]) & (x[i] < c1[j])))
        if touch.any():
            levels[i] = levels[j][touch].max() + 1
    return levels


def order_by_level(records, levels):
    """Records sorted by level (stable) and the offsets ``level_start`` [nlevels + 1] of the levels."""
    records = np.asarray(records, dtype=np.int32).reshape(-1, 8)
    levels = np.asarray(levels, dtype=np.int64)
    order = np.argsort(levels, kind='stable')
    nlev = int(levels.max()) + 1 if levels.size else 0
    level_start = np.searchsorted(levels[order], np.arange(nlev + 1)).astype(np.int32)
    return np.ascontiguousarray(records[order]), level_start


def split_bounds(splits, ntr):
    """[0, s1, ..., ntr] from the trace indices where a new split starts."""
    inner = [] if splits is None else [int(s) for s in np.asarray(splits).ravel() if 0 < int(s) < ntr]
    return np.unique(np.asarray([0] + inner + [ntr], dtype=np.int32))


def despike_2D(array, window, dt, overlap=10, ntraces=5, mode='mean', threshold=2, out='scaled', verbosity=0, splits=None, device=0,
               trace_major=False):
    """
    Remove single-trace noise bursts from seismic data (signature, checks and results of the reference's ``despike_2D``).

    array : samples x traces (traces x samples with ``trace_major=True``, the SEG-Y layout: no transposes then), float32.
    window [ms], dt [ms], overlap [%], ntraces (odd), mode in mean / rms / median, threshold, out in scaled / mode / threshold /
    zeros / median: as in the reference.  ``splits``: trace indices where a new split starts (``--use_delay``); every split is
    despiked on its own, one narrower than ``ntraces`` passes through with a warning.  The input is never modified; it is returned
    as it is when nothing is detected.  The kernels compute in float32: an array of another dtype is converted, and the result is
    float32 (the reference computes in the array's own dtype).
    """
    refusals = [(not 0 <= overlap <= 100, 'Overlap must be integer between 0 and 100 [%].'),
                (threshold < 0, 'Theshold must be positive.'),
                (ntraces % 2 == 0, 'Number of traces must be odd integer.'),
                (mode not in MODES, f'Amplitude mode must be one of {MODES}.'),
                (out not in REPLACE_AMP_MODES, f'Output amplitude option must be one of {REPLACE_AMP_MODES}.')]
    for refused, message in refusals:                           # the reference's checks, in its order, with its messages
        if refused:
            raise ValueError(message)
    if ntraces > _ffi.DESPIKE_MAX_TRACES:
        raise _ffi.UnsupportedError(_ffi.P3D_ERR_UNSUPPORTED, f'trace windows of up to {_ffi.DESPIKE_MAX_TRACES} traces are supported, got {ntraces}')
    a = np.asarray(array)
    if a.ndim != 2:
        raise ValueError('Input array must be 2D (samples x traces).')
    section = np.ascontiguousarray(a if trace_major else a.T, dtype=np.float32)
    ntr, ns = section.shape
    M, dy, main_end, add_start = window_rows(ns, window, dt, overlap)
    xprint(f'win: {(M, ntraces)}', kind='debug', verbosity=verbosity)
    xprint(f'dy (twt): {dy},  dx (traces): 1', kind='debug', verbosity=verbosity)

    bounds = split_bounds(splits, ntr)
    narrow = [(int(b0), int(b1)) for b0, b1 in zip(bounds[:-1], bounds[1:]) if b1 - b0 < ntraces]
    if narrow:
        warnings.warn(f'{len(narrow)} split(s) with fewer than {ntraces} traces pass through unchanged: {narrow[:5]}', RuntimeWarning, stacklevel=2)

    dsec = _ffi.DeviceArray((ntr, ns), np.float32, device)
    dmask = _ffi.DeviceArray((ntr, (ns + 63) // 64), np.uint64, device)
    dcnt = _ffi.DeviceArray((2, ntr), np.int32, device)
    try:
        dsec.upload(section)
        _ffi.despike_detect_dev(dsec.ptr, ntr, ns, ntraces, mode, threshold, main_end, add_start, dmask.ptr, dcnt.ptr, splits=bounds, device=device)
        counts = dcnt.download()
        records = np.zeros((0, 8), np.int32)
        if (counts > M * 0.1).any():
            records = spikes_from_mask(dmask.download(), counts, ns, M, main_end, add_start, ntraces, bounds)
        xprint('spikes:', records.shape[0], kind='debug', verbosity=verbosity)
        if records.shape[0] == 0:
            xprint(f'No spikes detected ({ntr} traces). Consider adjusting the input parameters.', kind='info', verbosity=verbosity)
            return array
        ordered, level_start = order_by_level(records, assign_levels(records))
        _ffi.despike_replace_dev(dsec.ptr, ntr, ns, ordered, level_start, mode, out, threshold, device=device)
        result = dsec.download()
    finally:
        for buf in (dsec, dmask, dcnt):
            buf.free()
    return result if trace_major else np.ascontiguousarray(result.T)
