"""Step 7 -- misties of crossing 2-D lines, mirror of the functions of ``pseudo_3D_interpolation/mistie_correction_segy.py``.

The data-parallel parts run in HIP (``p3d_mistie``, include/p3d.h) and there is no CPU fallback: where the lines' shot-point segments
cross (the reference: shapely's STRtree and GEOS), which shot point of either line is nearest to every crossing (the reference: a Python
loop), and the windowed cross-correlation and Pearson coefficient of the two envelope traces at every crossing (the reference: one
crossing at a time with both SEG-Y files opened each time).  Reading the files, the windows, the quality mask and the least-squares
solve of Bishop & Nunns (1994) stay NumPy.  DESIGN.md 3.10 lists the departures; the ones a caller sees:

- `find_intersections` takes the lines' vertex arrays (``points_split``) and returns plain arrays, not shapely geometries;
- `nearest_intersection_vertices` returns ``(index int32 [k, 2], distance float64 [k, 2])`` (column 0: the first line of the pair),
  not two float32 ``(index, distance)`` tables; `compute_misties` accepts either form;
- `compute_misties` takes the file names from ``lookup_df`` -- a mapping ``{line name: file name}`` or a DataFrame indexed by line name
  with a ``'line'`` column -- and raises ``ValueError`` naming the crossing where the reference crashes (no sample left, windows of
  different lengths).
"""
import os
import re

import numpy as np

from .. import _ffi
from .segy import SegyFile
from .signal import envelope
from .utils import rescale, xprint

BAD_TRACE_MEAN = 0.4                  # load_trace: mean(rescale(trace)) above this marks a bad / noisy trace
XCORR_BATCH_BYTES = 512 << 20         # both trace stacks of one correlation launch


def line_key(filename):
    """The line name of a SEG-Y file: its base name up to ``_UTM`` (the reference's ``(.*)_UTM``, greedy), the whole base name without
    extension when there is no ``_UTM``."""
    base = os.path.basename(str(filename))
    hit = re.search(r'(.*)_UTM', base)
    return hit.group(1) if hit else os.path.splitext(base)[0]


def samples2twt(samples, dt):
    """Samples -> two-way time in the unit of ``dt``."""
    return samples * dt


def _lines(points_split):
    lines = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in points_split]
    if not lines:
        raise ValueError('no lines')
    off = np.concatenate(([0], np.cumsum([p.shape[0] for p in lines]))).astype(np.int64)
    return lines, np.concatenate(lines) if off[-1] else np.zeros((0, 2)), off


def candidate_pairs(points_split):
    """The line pairs (i, j), i < j, whose bounding boxes overlap or touch, int32 [npairs, 2] in lexicographic order."""
    lines, _, _ = _lines(points_split)
    live = np.array([p.shape[0] > 0 for p in lines])
    lo = np.array([p.min(axis=0) if p.size else (np.inf, np.inf) for p in lines])
    hi = np.array([p.max(axis=0) if p.size else (-np.inf, -np.inf) for p in lines])
    meet = np.all((lo[:, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[:, None, :]), axis=2) & live[:, None] & live[None, :]
    i, j = np.nonzero(np.triu(meet, 1))
    return np.stack([i, j], axis=1).astype(np.int32)


def find_intersections(points_split, return_segments=False, capacity=None):
    """All points at which two different lines meet: ``(xy float64 [k, 2], line_idx int [k, 2])``, ordered by line pair (i, j), i < j,
    then along line i.  Proper crossings, touches at an end point and shared vertices count (shapely's ``intersects``); collinear
    overlapping segments give the two ends of the overlap; a point is reported once per line pair.  ``return_segments``: also the
    segment numbers ``[k, 2]`` on line i and line j.  ``capacity``: size of the first output buffer (see `_ffi.mistie_cross`)."""
    lines, xy, off = _lines(points_split)
    pairs = candidate_pairs(lines)
    hits = _ffi.mistie_cross(xy, off, pairs, capacity=capacity)
    line_idx = pairs[hits['pair']].astype(np.int64).reshape(-1, 2)
    pts = np.stack([hits['x'], hits['y']], axis=1)
    # position along line i: segment number plus the point's parameter on it
    a0 = xy[off[line_idx[:, 0]] + hits['seg_i']] if hits.size else np.zeros((0, 2))
    a1 = xy[off[line_idx[:, 0]] + hits['seg_i'] + 1] if hits.size else np.zeros((0, 2))
    r = a1 - a0
    rr = np.einsum('ij,ij->i', r, r)
    t = np.divide(np.einsum('ij,ij->i', pts - a0, r), rr, out=np.zeros(hits.size), where=rr > 0)
    order = np.lexsort((hits['part'], hits['seg_j'], t, hits['seg_i'], hits['pair']))
    if return_segments:
        return pts[order], line_idx[order], np.stack([hits['seg_i'], hits['seg_j']], axis=1)[order]
    return pts[order], line_idx[order]


def nearest_intersection_vertices(points_split, intersections_xy, line_intersections_idx):
    """For every intersection point and both of its lines: ``(index int32 [k, 2], distance float64 [k, 2])`` of the nearest vertex (shot
    point), the first minimum over the WHOLE line as ``np.argmin`` gives it (a line that doubles back can come nearer elsewhere than
    at the segment that was hit)."""
    _, xy, off = _lines(points_split)
    return _ffi.mistie_nearest(xy, off, intersections_xy, line_intersections_idx)


def cross_correlation_shift(cc):
    """Shift (in samples) between two correlated signals from their 'same'-mode cross-correlation: ``len(cc) // 2 - k`` with k the first
    arg max when ``|max| >= |min|``, else the first arg min.  shift < 0: signal A later than signal B."""
    cc = np.asarray(cc)
    zero_idx = int(np.floor(len(cc) / 2))
    idx = np.argmax(cc) if np.abs(np.max(cc)) >= np.abs(np.min(cc)) else np.argmin(cc)
    return zero_idx - int(idx)


def sample_times(segy):
    """Two-way time of a file's samples [ms]: the first trace's delay recording time plus ``arange(ns) * dt`` (segyio's ``file.samples``)."""
    return np.arange(segy.ns) * segy.dt + float(segy.header('DelayRecordingTime')[0])


def load_raw_trace(segy, idx_tr, ntraces2mix=3):
    """The reference's ``load_trace`` up to the envelope, rule for rule: trace ``idx_tr``; when ``mean(rescale(trace)) > 0.4`` the slice
    ``[idx_tr - n // 2, idx_tr + n - n // 2)`` (n = ``ntraces2mix`` made odd) clipped to the file, row ``n // 2`` of it deleted and the rest
    averaged -- at trace 0 the clipped slice starts at the bad trace, so the trace that is dropped is its neighbour.  Returns
    ``(trace float32, mixed)``."""
    trace = segy.traces([idx_tr])[0]
    if not np.mean(rescale(trace)) > BAD_TRACE_MEAN:
        return trace, False
    n = ntraces2mix if ntraces2mix % 2 != 0 else ntraces2mix + 1
    left = n // 2
    first, last = max(idx_tr - left, 0), min(idx_tr + n - left, segy.ntraces)
    rows = segy.traces(np.arange(first, last))
    return np.delete(rows, left, axis=0).mean(axis=0), True


def window_range(twt, win_up, win_lo):
    """(first sample, number of samples) of ``(twt >= win_up) & (twt <= win_lo)`` for ascending ``twt``."""
    inside = np.flatnonzero((twt >= win_up) & (twt <= win_lo))
    return (int(inside[0]), int(inside.size)) if inside.size else (0, 0)


def correlation_window(twt_0, twt_1, win=(False, False), say=None):
    """The reference's window rules: the given ``(upper, lower)`` limits [ms] when BOTH are truthy (an upper limit of 0 counts as not given,
    as there), else the overlap of the two traces' sample times; limits outside the overlap are pulled to it with a warning."""
    win_up, win_lo = win
    top, bottom = max(twt_0.min(), twt_1.min()), min(twt_0.max(), twt_1.max())
    if not all([win_up, win_lo]):
        win_up, win_lo = top, bottom
    if top > win_up or bottom < win_lo:
        if say is not None:
            say(f'Adjust window range ({win_up}:{win_lo} ms) to valid data range ', f'({top}:{bottom} ms)', kind='warning')
        win_up, win_lo = max(win_up, top), min(win_lo, bottom)
    return win_up, win_lo


def _file_name(lookup_df, name, lookup_col):
    if lookup_df is not None and lookup_col is not None:
        return lookup_df.loc[name, 'line'] if hasattr(lookup_df, 'loc') else lookup_df[name]
    return name + '.sgy'


def _vertex_indices(nearest):
    nearest = np.asarray(nearest)
    return (nearest[:, 0] if nearest.ndim == 2 else nearest).astype(np.int64)


def intersection_traces(segy_dir, line_intersections_names, nearest_0, nearest_1, win=(False, False), lookup_df=None, lookup_col=None,
                        ntraces2mix=3, verbosity=1):
    """Everything `compute_misties` reads from the files: per crossing and side the (envelope) trace, zero-padded to the longest trace, and
    its window.  Returns ``dict(a, b float32 [k][nsmax], ranges int32 [k][4], dt [k][2], mixed bool [k][2], paths)``.  Traces of equal length go
    through the GPU envelope together (files with 'env' in their path hold envelopes already)."""
    names = np.asarray(line_intersections_names).reshape(-1, 2)
    rows = np.stack([_vertex_indices(nearest_0), _vertex_indices(nearest_1)], axis=1)
    k = names.shape[0]
    files, raw, paths = {}, [], []
    mixed, dts, ranges = np.zeros((k, 2), bool), np.zeros((k, 2)), np.zeros((k, 4), np.int32)

    def say(*args, **kwargs):
        xprint(*args, verbosity=verbosity, **kwargs)

    for c in range(k):
        pair = []
        for side in range(2):
            path = os.path.join(segy_dir, _file_name(lookup_df, names[c, side], lookup_col))
            if path not in files:
                files[path] = SegyFile(path)
            trace, mixed[c, side] = load_raw_trace(files[path], int(rows[c, side]), ntraces2mix)
            raw.append(trace)
            pair.append(path)
            dts[c, side] = files[path].dt
        paths.append(pair)
        if dts[c, 0] != dts[c, 1]:
            raise ValueError(f'Identical sample interval required: {dts[c, 0]} != {dts[c, 1]} ({names[c, 0]} != {names[c, 1]})')
        twt_0, twt_1 = sample_times(files[pair[0]]), sample_times(files[pair[1]])
        win_up, win_lo = correlation_window(twt_0, twt_1, win, say)
        ranges[c] = window_range(twt_0, win_up, win_lo) + window_range(twt_1, win_up, win_lo)
    nsmax = max((t.size for t in raw), default=1)
    stack = np.zeros((2 * k, nsmax), np.float32)
    flat_paths = [p for pair in paths for p in pair]
    for ns in sorted({t.size for t in raw}):
        plain = [n for n, t in enumerate(raw) if t.size == ns and 'env' in flat_paths[n]]
        todo = [n for n, t in enumerate(raw) if t.size == ns and 'env' not in flat_paths[n]]
        for n in plain:
            stack[n, :ns] = raw[n]
        if todo:
            stack[todo, :ns] = envelope(np.stack([raw[n] for n in todo]), axis=-1)
    return dict(a=stack[0::2], b=stack[1::2], ranges=ranges, dt=dts, mixed=mixed, paths=paths)


def correlate_intersections(a, b, ranges, names=None, path='auto'):
    """`_ffi.mistie_xcorr` in batches, with the per-crossing status turned into a ``ValueError`` that names the crossing.  Returns
    ``(shift int32, coeff float64, n int32)``."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    k = a.shape[0]
    shift, coeff, n = np.zeros(k, np.int32), np.zeros(k), np.zeros(k, np.int32)
    step = max(1, XCORR_BATCH_BYTES // max(8 * a.shape[1], 1))
    for c0 in range(0, k, step):
        part = slice(c0, min(c0 + step, k))
        shift[part], coeff[part], n[part], status = _ffi.mistie_xcorr(a[part], b[part], ranges[part], path=path)
        bad = np.flatnonzero(status)
        if bad.size:
            c = c0 + int(bad[0])
            what = {_ffi.MISTIE_EMPTY: 'no sample is left once the samples at which either trace is 0 are dropped',
                    _ffi.MISTIE_LENGTHS: f'the two windows differ in length ({ranges[c][1]} and {ranges[c][3]} samples)',
                    _ffi.MISTIE_RANGE: f'a window lies outside its trace (ranges {ranges[c].tolist()})'}[int(status[bad[0]])]
            label = f' ({names[c][0]} x {names[c][1]})' if names is not None else ''
            raise ValueError(f'intersection {c}{label}: {what}')
    return shift, coeff, n


def solve_offsets(misties, line_intersections_idx, nlines):
    """One offset per line from the misties at the crossings (Bishop & Nunns, 1994): least squares of ``A offsets = misties`` with
    ``A[c, i] = 1``, ``A[c, j] = -1`` for crossing c of lines (i, j).  Returns ``(offsets int16, residuals)``."""
    idx = np.asarray(line_intersections_idx).reshape(-1, 2)
    A = np.zeros((len(misties), nlines), dtype=np.int32)
    i = np.arange(len(misties))
    A[i, idx[:, 0]] = 1
    A[i, idx[:, 1]] = -1
    offsets, residuals, _, _ = np.linalg.lstsq(A, misties, rcond=None)
    return np.around(offsets, 0).astype('int16'), residuals


def compute_misties(segy_dir, line_intersections_names, line_intersections_idx, nearest_0, nearest_1, win=(False, False), quality=0,
                    lookup_df=None, lookup_col=None, check_bad_traces=False, ntraces2mix=3, return_ms=False, return_coeff=False, verbosity=1):
    """Mistie per line (in samples) from the crossings of the lines; the reference's arguments and return shapes:
    ``(offsets int16 [nlines], residuals)``, plus ``offsets_ms`` with ``return_ms`` and the kept crossings' ``coeffs`` (float32) with
    ``return_coeff``.  ``nearest_0`` / ``nearest_1``: vertex (trace) index per crossing on the first / second line, either as index arrays
    or as the reference's ``(index, distance)`` tables.  As in the reference bad traces are ALWAYS checked (``check_bad_traces`` is accepted
    and ignored), and ``nlines = len(lookup_df)``."""
    names = np.asarray(line_intersections_names).reshape(-1, 2)
    idx = np.asarray(line_intersections_idx).reshape(-1, 2)
    if names.shape[0] == 0:
        raise ValueError('no line intersections: nothing to compute misties from')
    if lookup_df is None:
        raise ValueError('`lookup_df` (line name -> file name) is required: its length is the number of lines')
    got = intersection_traces(segy_dir, names, nearest_0, nearest_1, win=win, lookup_df=lookup_df, lookup_col=lookup_col,
                              ntraces2mix=ntraces2mix, verbosity=verbosity)
    shift, coeff, _ = correlate_intersections(got['a'], got['b'], got['ranges'], names=names)
    intersections_misties = shift.astype(np.int16)
    intersections_coeffs = coeff.astype(np.float32)
    with np.errstate(invalid='ignore'):
        mask_quality = np.abs(intersections_coeffs) >= quality
    xprint(f'Filtered < {np.count_nonzero(~mask_quality)} > values below quality threshold ({quality})', kind='info', verbosity=verbosity)
    coeffs = intersections_coeffs[mask_quality]
    offsets, residuals = solve_offsets(intersections_misties[mask_quality], idx[mask_quality], len(lookup_df))
    dt = got['dt'][-1, 0]
    if return_ms and return_coeff:
        return (offsets, residuals), samples2twt(offsets, dt=dt), coeffs
    if return_ms:
        return (offsets, residuals), samples2twt(offsets, dt=dt)
    if return_coeff:
        return (offsets, residuals), coeffs
    return (offsets, residuals)


def compensate_mistie(data, mistie, verbosity=1, trace_major=False):
    """Shift all traces of a section ``data`` [nsamples][ntraces] (``trace_major``: [ntraces][nsamples]) by ``mistie`` samples on the GPU
    (``p3d_static_shift`` with one shift for all traces): negative moves the traces up, zeros fill the end.  Returns a new float32 array."""
    mistie_samples = int(np.around(mistie, 0))
    data = np.asarray(data, dtype=np.float32)
    if data.ndim != 2:
        raise ValueError('data is a 2D section')
    section = np.ascontiguousarray(data if trace_major else data.T)
    shifted = _ffi.static_shift(section, np.full(section.shape[0], np.clip(mistie_samples, -2**31, 2**31 - 1), dtype=np.int32))
    if mistie_samples != 0:
        xprint(f'#samples:{mistie_samples:>5}   ->   {"up" if mistie_samples < 0 else "down"}: {data.shape}', kind='debug', verbosity=verbosity)
    return shifted if trace_major else np.ascontiguousarray(shifted.T)
