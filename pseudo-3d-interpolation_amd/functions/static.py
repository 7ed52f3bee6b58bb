"""Step 5: seafloor detection and static correction of a 2-D section (mirror of the reference's ``detect_seafloor_reflection``,
``get_static``, ``compensate_static`` and of the 1-D filters they use).

Everything that touches the section runs on the GPU (csrc/p3d_static.hip) on the trace-major layout of the SEG-Y file: the trace scan, the
two STA/LTA passes, the peak pick and the shift.  The section is uploaded once; only one integer (or one double) per trace comes back
between the kernels.  The chain in between works on one value per trace and is NumPy on the host (no scipy): moving double-MAD outlier
detection, a not-a-knot cubic spline through the samples that are kept, a moving median, a Savitzky-Golay line fit, a polynomial
detrend.  DESIGN.md 3.9 has the algorithm, the kernels and the departures from the reference."""
import numpy as np

from .. import _ffi

CHUNK_ROWS = 4096     # windows of the moving filters that are materialised at a time


# ---- conversions (the reference's functions/utils.py) -----------------------------------------------------------

def depth2samples(depth, dt, v=1500, units='s'):
    """Depth (m) -> two-way travel time -> samples of ``dt`` (``units`` 's', 'ms'; 'ns' divides by 1e-6 as the reference does)."""
    return twt2samples(depth / (v / 2), _seconds(dt, units))


def twt2samples(twt, dt, units='s'):
    return twt / _seconds(dt, units)


def samples2twt(samples, dt):
    return samples * dt


def _seconds(dt, units):
    if units == 'ms':
        return dt / 1000
    if units == 'ns':
        return dt / 1e-6
    return dt


# ---- 1-D filters ------------------------------------------------------------------------------------------------

def pad_array(a, n, zeros=False):
    """``n`` more values on either side of a 1-D array: zeros, or the neighbouring values mirrored about the end sample and folded to
    its lower side (end - |mirror - end|)."""
    a = np.asarray(a)
    if zeros:
        return np.concatenate((np.zeros(n), a, np.zeros(n)))
    front = a[0] - np.abs(a[1:n + 1][::-1] - a[0])
    back = a[-1] - np.abs(a[-n - 1:-1][::-1] - a[-1])
    return np.concatenate((front, a, back))


def _windows(a, win):
    return np.lib.stride_tricks.sliding_window_view(a, win)


def moving_median(a, win=3, padded=False):
    """Median of every window of ``win`` values; ``padded``: on the array extended by (win - 1) // 2 values (`pad_array`)."""
    a = np.asarray(a)
    if padded:
        a = pad_array(a, (win - 1) // 2)
    w = _windows(a, win)
    return np.concatenate([np.median(w[r:r + CHUNK_ROWS], axis=-1) for r in range(0, w.shape[0], CHUNK_ROWS)])


def _double_mad_windows(w):
    """The reference's two-sided MAD of every window (rows of ``w``), with its conventions: the deviation is taken over the WHOLE window,
    a window whose centre lies at or below the median gets the 'left' value, at or above it the 'right' one (the latter wins on the
    median), zeros become 1, and the result has the dtype of the data (deviations of integers are truncated)."""
    med = np.median(w, axis=-1)
    dev = np.abs(w - med[:, None])
    centre = w[:, w.shape[-1] // 2]
    mad = np.ones(w.shape[0], dtype=w.dtype)
    for side in (centre <= med, centre >= med):
        part = np.median(dev[side], axis=-1) if side.any() else np.zeros(0)
        part[part == 0] = 1
        mad[side] = part
    return med, mad


def moving_mad_filter(a, win, threshold=3, mad_mode='double'):
    """Indices of the outliers of a moving two-sided median-absolute-deviation filter of ``win`` (odd) values."""
    if type(win) is not int or win % 2 != 1:
        raise ValueError('window length must be odd integer')
    if mad_mode != 'double':
        raise NotImplementedError("only mad_mode='double' is implemented")
    a = np.asarray(a)
    w = _windows(pad_array(a, (win - 1) // 2), win)
    flagged = []
    for r in range(0, w.shape[0], CHUNK_ROWS):
        med, mad = _double_mad_windows(w[r:r + CHUNK_ROWS])
        mad[mad == 0] = 1
        flagged.append(r + np.nonzero(np.abs(a[r:r + CHUNK_ROWS] - med) / mad > threshold)[0])
    return np.concatenate(flagged)


def median_abs_deviation_double(x):
    """Two-sided MAD of a 1-D array: per sample the median deviation of the values at or below the median (samples up to the median)
    or at or above it (samples beyond).  Raises when one side is 0."""
    x = np.asarray(x)
    med = np.median(x)
    dev = np.abs(x - med)
    left, right = np.median(dev[x <= med]), np.median(dev[x >= med])
    if left == 0 or right == 0:
        raise ValueError('one side of median absolute deviation is zero')
    mad = np.repeat(left, len(x))
    mad[x > med] = right
    return mad.astype(x.dtype)


def mad_filter(a, threshold=3, mad_mode='double'):
    """Indices of the values further than ``threshold`` two-sided MADs from the median."""
    if mad_mode != 'double':
        raise NotImplementedError("only mad_mode='double' is implemented")
    a = np.asarray(a)
    return np.nonzero(np.abs(a - np.median(a)) / median_abs_deviation_double(a) > threshold)[0]


def polynominal_filter(data, order=3, kind='high'):
    """``data`` minus its least-squares polynomial of ``order`` ('high'), or the polynomial itself ('low')."""
    data = np.array(data, dtype=float)
    x = np.arange(len(data))
    fit = np.polyval(np.polyfit(x, data, deg=order), x)
    if kind == 'high':
        return data - fit
    if kind == 'low':
        return data - (data - fit)
    raise ValueError(f'filter kind `{kind}` is not available')


def not_a_knot_spline(x, y, xq):
    """Values at ``xq`` (inside [x[0], x[-1]]) of the cubic spline through (x, y), x ascending, with not-a-knot ends: the third derivative
    is continuous across x[1] and x[-2] (what ``scipy.interpolate.interp1d(kind='cubic')`` evaluates).  The second derivatives come from one
    tridiagonal solve (the end conditions are substituted into the first and the last interior equation), so the cost is linear in
    the number of points."""
    x, y, xq = np.asarray(x, dtype=float), np.asarray(y, dtype=float), np.asarray(xq, dtype=float)
    n = x.size
    if n < 4:
        raise ValueError(f'a cubic spline needs at least 4 samples, got {n}')
    h = np.diff(x)
    if np.any(h <= 0):
        raise ValueError('x must ascend')
    slope = np.diff(y) / h
    diag = 2.0 * (h[:-1] + h[1:])
    lower, upper = h[:-1].copy(), h[1:].copy()          # coefficients of M[i - 1] and M[i + 1] in the equation of point i = 1 ... n - 2
    rhs = 6.0 * np.diff(slope)
    # M[0] = (1 + h0 / h1) M[1] - (h0 / h1) M[2], and the mirror image at the other end
    r0, r1 = h[0] / h[1], h[-1] / h[-2]
    diag[0] += h[0] * (1.0 + r0)
    upper[0] -= h[0] * r0
    diag[-1] += h[-1] * (1.0 + r1)
    lower[-1] -= h[-1] * r1
    m = diag.size
    cp, dp = np.empty(m), np.empty(m)
    cp[0], dp[0] = upper[0] / diag[0], rhs[0] / diag[0]
    for i in range(1, m):
        den = diag[i] - lower[i] * cp[i - 1]
        cp[i] = upper[i] / den
        dp[i] = (rhs[i] - lower[i] * dp[i - 1]) / den
    M = np.empty(n)
    M[m] = dp[m - 1]
    for i in range(m - 2, -1, -1):
        M[i + 1] = dp[i] - cp[i] * M[i + 2]
    M[0] = (1.0 + r0) * M[1] - r0 * M[2]
    M[-1] = (1.0 + r1) * M[-2] - r1 * M[-3]
    k = np.clip(np.searchsorted(x, xq, side='right') - 1, 0, n - 2)
    hk, a, b = h[k], x[k + 1] - xq, xq - x[k]
    return (M[k] * a**3 + M[k + 1] * b**3) / (6.0 * hk) + (y[k] / hk - M[k] * hk / 6.0) * a + (y[k + 1] / hk - M[k + 1] * hk / 6.0) * b


def filter_interp_1d(data, method='r_doubleMAD', kind='cubic', win=11, threshold=3.0, filter_boundaries=True):
    """Remove the outliers of a moving two-sided MAD filter and interpolate across them (``kind`` 'cubic': not-a-knot spline, 'linear').
    Flagged runs that touch the first or the last sample are kept, by the reference's counting rule.  Returns float64; samples that are
    kept are returned as they are (the reference returns spline values there, equal up to rounding)."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError('data must be 1D array!')
    if kind not in ('cubic', 'linear'):
        raise NotImplementedError(f"interpolation kind {kind!r} is not implemented (use 'cubic' or 'linear')")
    if method == 'r_doubleMAD':
        idx = moving_mad_filter(data, win=win, threshold=threshold, mad_mode='double')
    elif method == 'doubleMAD':
        idx = mad_filter(data, threshold=threshold, mad_mode='double')
    else:
        raise NotImplementedError(f"outlier method {method!r} is not implemented (use 'r_doubleMAD' or 'doubleMAD')")
    if filter_boundaries:
        steps = np.diff(idx)
        pieces = np.split(steps, np.nonzero(steps > 1)[0])
        if np.isin(0, idx):
            idx = idx[pieces[0].size + 1:]
        if np.isin(data.size - 1, idx):
            idx = idx[:-pieces[-1].size]
    keep = np.ones(data.size, dtype=bool)
    keep[idx] = False
    x = np.arange(data.size)
    out = data.astype(np.float64)
    if not keep.all():
        gaps = x[~keep]
        if gaps[0] < x[keep][0] or gaps[-1] > x[keep][-1]:
            raise ValueError('A value to interpolate lies outside the samples that were kept.')
        if kind == 'cubic':
            out[~keep] = not_a_knot_spline(x[keep], data[keep], gaps)
        else:
            out[~keep] = np.interp(gaps, x[keep], data[keep])
    return out


def savgol_line(y, win):
    """Savitzky-Golay filter of polynomial order 1 without derivative, edges in mode 'interp': the moving mean of ``win`` (odd) values, and
    on the first and the last ``win // 2`` samples the least-squares line through the first / last ``win`` values."""
    y = np.asarray(y, dtype=float)
    if win % 2 != 1:
        raise NotImplementedError('the Savitzky-Golay window must be an odd number of traces')
    if win > y.size:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    if win < 3:
        raise ValueError('polyorder must be less than window_length.')
    half = win // 2
    out = np.empty_like(y)
    out[half:y.size - half] = np.convolve(y, np.full(win, 1.0 / win), mode='valid')
    t = np.arange(win) - half                           # centred abscissa: slope and mean decouple
    for seg, dst, at in ((y[:win], slice(0, half), t[:half]), (y[-win:], slice(y.size - half, y.size), t[win - half:])):
        out[dst] = seg.mean() + (t @ seg) / (t @ t) * at
    return out


# ---- the static ---------------------------------------------------------------------------------------------------

def get_static(data, kind='diff', interp_kind='cubic', win_mad=None, win_sg=7, limit_perc=99, limit_samples=10, limit_by_MAD=False,
               limit_depressions=False):
    """Static of every trace as the deviation of ``data`` (one value per trace: seafloor sample or water depth) from its smooth trend:
    outliers removed (`filter_interp_1d`, window ``win_mad``: 5 % of the traces, odd, at least 7), then Savitzky-Golay low-pass minus
    the data.  Clipping as in the reference and in its order: inside and around seafloor depressions (``limit_depressions`` = (pad,
    limit at the outer edge, limit in the depression); found as runs of at least 3 traces below the order-11 polynomial trend by more
    than 3 two-sided MADs; when none is found the static is returned WITHOUT the clips below), by percentile, by ``limit_samples``, by
    ``limit_by_MAD`` x median |static| (note that, as there, ``False`` is a number: 0)."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError(f'Input array must have only one dimension not {data.ndim}.')
    if kind not in ['diff', 'deriv']:
        raise ValueError(f'Kind < {kind} > is not supported')
    if kind == 'deriv':
        raise NotImplementedError("kind='deriv' is not implemented")
    if interp_kind not in ('cubic', 'linear'):
        raise NotImplementedError(f"interpolation kind {interp_kind!r} is not implemented (use 'cubic' or 'linear')")
    if win_mad is None:
        win_mad = int(data.size * 0.05)
    win_mad += 1 - win_mad % 2
    win_mad = max(win_mad, 7)

    cleaned = filter_interp_1d(data, method='r_doubleMAD', kind=interp_kind, threshold=3, win=win_mad)
    lowpass = savgol_line(cleaned, win_sg)
    static = lowpass - cleaned                          # < 0: samples are added at the top of the trace, > 0: at the bottom

    def clip(values, limit):
        return np.where(np.abs(values) > limit, limit * np.sign(values), values)

    if limit_depressions:
        detrended = -polynominal_filter(lowpass, order=11)
        flagged = mad_filter(detrended, threshold=3, mad_mode='double')
        below = flagged[detrended[flagged] < 0]
        runs = [r for r in np.split(below, np.nonzero(np.diff(below) > 1)[0] + 1) if r.size >= 3]
        if not runs:
            return static
        npad, outer, centre = limit_depressions
        where = np.concatenate([np.arange(r[0] - npad, r[-1] + npad + 1, dtype='int') for r in runs])
        limits = np.concatenate([np.concatenate((np.linspace(outer, centre + 1, npad), np.full(r.size, centre),
                                                 np.linspace(centre + 1, outer, npad))).astype('int') for r in runs])
        inside = (where >= 0) & (where < detrended.size)
        where, limits = where[inside], limits[inside]
        static[where] = clip(static[where], limits)
    if limit_perc is not None and limit_perc is not False:
        static = clip(static, np.percentile(np.abs(static), limit_perc))
    if isinstance(limit_samples, (float, int)):
        static = clip(static, limit_samples)
    if limit_by_MAD is True or isinstance(limit_by_MAD, (int, float)):
        factor = limit_by_MAD if isinstance(limit_by_MAD, (int, float)) else 3
        static = clip(static, int(np.ceil(np.median(np.abs(static)) * factor)))
    return static


# ---- the section: GPU ---------------------------------------------------------------------------------------------

def _section(data, trace_major):
    a = np.asarray(data)
    if a.ndim != 2 or a.size == 0:
        raise ValueError('Input array must be 2D (samples x traces).')
    return np.ascontiguousarray(a if trace_major else a.T, dtype=np.float32)


def _truncate(values):
    return np.asarray(values).astype('int')


def seafloor_stages(data, idx_slice_start=None, nsta=None, nlta=None, win=30, threshold=None, win_mad=None, win_mad_post=None, win_median=11,
                    n=5, post_detection_filter=True, trace_major=False, device=0, nso=None):
    """`detect_seafloor_reflection` with its intermediate results: a dict with ``live`` (bool per trace: not a zero trace), ``start``
    (first sample of the valid slice per trace), ``nsta``, ``nlta``, ``threshold``, ``raw`` (first crossings, live traces), ``baseline``
    (after the MAD / spline and the median filter, live traces), ``peak`` (picked rows, live traces), ``idx`` (the result, all traces)."""
    section = _section(data, trace_major)
    ntr, ns = section.shape
    nsamples = ns if nso is None else int(nso)
    if not 1 <= nsamples <= ns:
        raise ValueError(f'{nsamples} original samples do not fit traces of {ns} samples')
    if nsta is None:
        nsta = int(np.around(nsamples * 0.001))
    if nlta is None:
        nlta = int(np.around(nsamples * 0.05))
    if nsta < 3:
        nsta, nlta = 3, 50
        print(f'[WARNING]    Changed nsta={nsta} and nlta={nlta}!')
    if nlta >= nsamples:
        raise ValueError(f'No sample beyond the long window: nlta={nlta} for traces of {nsamples} samples.')
    nvalid = None if nso is None else nsamples
    bufs = [_ffi.DeviceArray((ntr, ns), np.float32, device), _ffi.DeviceArray((ntr,), np.int32, device), _ffi.DeviceArray((ntr,), np.float64, device),
            _ffi.DeviceArray((ntr,), np.int32, device), _ffi.DeviceArray((ntr,), np.int32, device)]
    dsec, dfirst, dpeak, dint, dout = bufs
    try:
        dsec.upload(section)
        _ffi.static_scan_dev(dsec.ptr, ntr, ns, dfirst.ptr, device=device)
        first = dfirst.download()
        live = first >= 0
        if not live.any():
            raise ValueError('The section holds only zero traces.')
        start = np.maximum(first, 0) if nso is not None else np.zeros(ntr, np.int32)
        if nso is not None and np.any(start[live] + nsamples > ns):
            raise IndexError(f'{int(np.sum(start[live] + nsamples > ns))} trace(s) hold fewer than {nsamples} samples after their first non-zero one.')
        if threshold is None:
            _ffi.static_stalta_max_dev(dsec.ptr, ntr, ns, dfirst.ptr, nsta, nlta, dpeak.ptr, nvalid=nvalid, device=device)
            threshold = float(dpeak.download()[live].max())
        _ffi.static_stalta_cross_dev(dsec.ptr, ntr, ns, dfirst.ptr, nsta, nlta, threshold, dint.ptr, nvalid=nvalid, device=device)
        raw = dint.download()[live].astype('int')
        stages = dict(live=live, start=start, nsta=nsta, nlta=nlta, threshold=threshold, raw=raw.copy())

        idx = raw
        if idx_slice_start is not None:
            offset = np.asarray(idx_slice_start)
            offset = offset[live] if offset.shape == (ntr,) else offset
            idx = idx + offset
            idx = np.where(np.logical_or(idx > nsamples - offset, idx < offset), np.median(idx), idx)
        if win_mad is None:
            win_mad = int(idx.size * 0.02)
            win_mad += 1 - win_mad % 2
            win_mad = max(win_mad, 7)
        idx = _truncate(filter_interp_1d(idx, method='r_doubleMAD', kind='cubic', threshold=3, win=win_mad))
        win_median = int(0.3 * ntr) if win_median > ntr else win_median
        idx = _truncate(moving_median(idx, win_median, padded=True))
        if idx.size != raw.size:
            raise ValueError(f'A median window of {win_median} traces does not keep the number of traces; use an odd window.')
        stages['baseline'] = idx.copy()

        if win > 0:
            if np.any(idx + win < 0) or np.any(idx - win >= nsamples):
                raise ValueError('A search window lies outside its trace.')
            base = np.zeros(ntr, np.int32)
            base[live] = idx
            dint.upload(base)
            _ffi.static_peak_dev(dsec.ptr, ntr, ns, dfirst.ptr, dint.ptr, win, n, dout.ptr, nvalid=nvalid, device=device)
            peak = dout.download()[live].astype('int')
        else:
            peak = idx
        stages['peak'] = peak.copy()
    finally:
        for buf in bufs:
            buf.free()

    if not live.all():                                   # zero traces get the linearly interpolated pick of their neighbours
        x = np.arange(ntr)
        if not (live[0] and live[-1]):
            raise ValueError('A zero trace at the start or the end of the section cannot be interpolated.')
        peak = _truncate(np.interp(x, x[live], peak))
    if post_detection_filter:
        if win_mad_post is None:
            win_mad_post = int(raw.size * 0.01)
            win_mad_post += 1 - win_mad_post % 2
            win_mad_post = max(win_mad_post, 7)
        peak = _truncate(filter_interp_1d(peak, method='r_doubleMAD', kind='cubic', threshold=3, win=win_mad_post))
    stages['idx'] = _truncate(peak)
    return stages


def detect_seafloor_reflection(data, idx_slice_start=None, nsta=None, nlta=None, win=30, threshold=None, win_mad=None, win_mad_post=None,
                               win_median=11, n=5, post_detection_filter=True, trace_major=False, device=0, nso=None):
    """
    Sample index of the seafloor reflection of every trace (parameters, defaults and rules of the reference's function).

    data : samples x traces (traces x samples with ``trace_major=True``, the SEG-Y layout: no transpose then).
    The STA/LTA ratio (``nsta`` / ``nlta`` samples, default 0.1 % / 5 % of the samples; 3 / 50 when ``nsta`` would be below 3) is
    thresholded at its largest value within rows nlta ... 2 nlta - 1 (the water column) unless ``threshold`` is given; the first
    crossings are cleaned along the profile (moving double MAD of ``win_mad`` traces with spline interpolation, moving median of
    ``win_median`` traces), and in the window of +- ``win`` samples around them the first group among the ``n`` largest amplitudes is
    picked (``win=0``: the cleaned crossings are returned).  Zero traces are left out and interpolated linearly afterwards;
    ``post_detection_filter`` cleans the picks once more (``win_mad_post`` traces).
    ``nso`` (not in the reference, which is given the sliced array instead): the traces are zero-padded and their valid part is the
    ``nso`` samples from the first non-zero one; the result then counts from there.
    """
    return seafloor_stages(data, idx_slice_start, nsta, nlta, win, threshold, win_mad, win_mad_post, win_median, n, post_detection_filter,
                           trace_major, device, nso)['idx']


def compensate_static(data, static, dt=None, units='ms', cnv_d2s=False, v=1500, trace_major=False, device=0):
    """
    Shift every trace by its static: ``static`` in samples, or a depth in m with ``cnv_d2s`` (converted with ``dt`` [``units``] and the
    sound velocity ``v``), rounded with ``np.around`` to int32.  Negative: the trace moves up and zeros fill its end; positive: down,
    zeros at its top.  Returns ``(shifted, static_samples)``; the input is not modified and the result is float32.
    """
    if cnv_d2s:
        if dt is None:
            print('[ERROR]   `dt` is required when converting depth to samples')
            return None
        static = depth2samples(np.asarray(static), dt=_seconds(dt, units), v=v, units='s')
    static_samples = np.around(static, 0).astype(np.int32)
    section = _section(data, trace_major)
    ntr, ns = section.shape
    if static_samples.shape != (ntr,):
        raise ValueError(f'{ntr} traces but {static_samples.shape} statics')
    bufs = [_ffi.DeviceArray((ntr, ns), np.float32, device), _ffi.DeviceArray((ntr, ns), np.float32, device), _ffi.DeviceArray((ntr,), np.int32, device)]
    try:
        bufs[0].upload(section)
        bufs[2].upload(static_samples)
        _ffi.static_shift_dev(bufs[0].ptr, ntr, ns, bufs[2].ptr, bufs[1].ptr, device=device)
        shifted = bufs[1].download()
    finally:
        for buf in bufs:
            buf.free()
    return (shifted if trace_major else np.ascontiguousarray(shifted.T)), static_samples
