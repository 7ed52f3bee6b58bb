"""Signal functions of steps 11 and 15, mirrored from pseudo_3D_interpolation/functions/signal.py: automatic gain control
(``get_AGC_samples`` :302-322, ``AGC`` :325-409), the time-variant ``gain`` (:96-299), ``programmed_gain_control``, ``rms``,
``rms_normalization``, ``calc_reference_amplitude``, ``envelope`` and ``get_resampled_twt``, plus scipy's ``resample_poly`` and
``resample`` along the time axis.  The data work runs in HIP (``p3d_agc``, ``p3d_pre_*_dev``, include/p3d.h); only small tables
(gain curves, FIR taps, spectral factors) are built here in NumPy.  Only the reference's default AGC zero padding is implemented."""
import math
import warnings

import numpy as np

from .. import _ffi


def get_AGC_samples(win: float, dt: float):
    """AGC window length in seconds -> number of samples (``int(win / dt)``, made odd by adding one)."""
    samples = int(win / dt)
    samples = samples + 1 if samples % 2 == 0 else samples
    return samples


def AGC(x, win: int, kind: str = 'rms', pad: bool = True, pad_mode: str = 'constant', squared: bool = False,
        return_gain_func: bool = False, axis: int = -1):
    """Automatic gain control of a trace (1-D), profile (2-D) or cube (3-D) along ``axis``, on the GPU.

    Same arguments and defaults as the reference.  ``win`` (samples, an ``int``) is made odd; the time axis is zero-padded by
    ``win // 2`` samples at both ends and the gain ``g`` is the rms / mean / median of the ``win`` samples centred on each sample,
    pads included; ``g == 0`` becomes 1 and the result is ``x * (1 / g)`` (``sign(y) * y**2`` when ``squared``).

    Differences from the reference: the result is a NEW float32 array (the reference scales its argument in place); the input is
    read as float32.  A time axis that is not the slowest (``axis != 0``, e.g. the default -1 of a 2-D profile) is moved to the
    front with ``np.moveaxis`` on the host and back afterwards: the kernel runs on time-slow ``[nt][ntraces]`` data, the
    slice-major ``(twt, iline, xline)`` cube as it is.  Only ``pad=True, pad_mode='constant'`` is implemented; anything else raises
    ``NotImplementedError``.
    """
    if not isinstance(win, int):
        raise TypeError(f'`win` must be integer not {type(win)}')
    if kind not in _ffi.AGC_KIND:
        raise ValueError(f'Unknown AGC kind "{kind}"')
    if not pad:
        raise NotImplementedError('AGC without padding (pad=False) is not implemented')
    if pad_mode != 'constant':
        raise NotImplementedError(f"AGC pad_mode {pad_mode!r}: only 'constant' (zero padding) is implemented")
    win = win + 1 if win % 2 == 0 else win
    x = np.asarray(x, dtype=np.float32)
    if x.ndim not in (1, 2, 3):
        raise ValueError(f'expected a trace, profile or cube (1-3 axes), got {x.ndim} axes')
    axis = axis % x.ndim
    xt = np.moveaxis(x, axis, 0) if axis != 0 else x
    res = _ffi.agc(xt, win, kind=kind, squared=squared, return_gain=return_gain_func)
    y, g = res if return_gain_func else (res, None)
    if axis != 0:
        y = np.moveaxis(y, 0, axis)
        g = None if g is None else np.moveaxis(g, 0, axis)
    if return_gain_func:
        return y, g
    return y


# ---- step 11 ---------------------------------------------------------------------------------------------------------------------
def _time_first(x, axis):
    x = np.asarray(x, dtype=np.float32)
    axis = axis % x.ndim
    return (np.moveaxis(x, axis, 0) if axis != 0 else x), axis


def _time_back(y, axis):
    return np.moveaxis(y, 0, axis) if axis != 0 else y


def programmed_gain_control(twt: np.ndarray, twt_gain: dict):
    """Programmed gain control curve (float32) over the samples of ``twt``.

    Each ``{twt: gain}`` node is pinned to the sample nearest to its time (when two nodes land on one sample, the later time wins);
    the first and last sample take the gain of the earliest / latest node unless a node already sits there; the samples in between
    are interpolated linearly in sample index."""
    t = np.asarray(twt)
    times = sorted(twt_gain)
    pinned = {}
    for tk in times:
        pinned[int(np.argmin(np.abs(t - tk)))] = twt_gain[tk]
    pinned.setdefault(0, twt_gain[times[0]])
    pinned.setdefault(t.size - 1, twt_gain[times[-1]])
    at = np.array(sorted(pinned))
    val = np.array([pinned[i] for i in at], dtype=np.float32)
    return np.interp(np.arange(t.size), at, val).astype(np.float32)


def gain_tables(nsamples, twt, tpow=0.0, epow=0.0, etpow=1.0, ebase=None, gpow=0.0, agc=False, agc_win=0.05, agc_kind='rms',
                agc_sqrt=False, clip=None, pclip=None, nclip=None, qclip=None, linear=None, pgc=None, bias=None, scale=1.0, norm=False,
                norm_rms=False):
    """Parameter vector and curves of ``p3d_pre_gain_dev`` (include/p3d.h) for the reference's ``gain`` arguments: ``(prm, curves)``,
    curves [4][nsamples] (tpow, epow, linear, pgc) or None."""
    scalars = dict(tpow=tpow, epow=epow, etpow=etpow, gpow=gpow, clip=clip, pclip=pclip, nclip=nclip, qclip=qclip, bias=bias, scale=scale)
    for name, value in scalars.items():
        if value is not None and not isinstance(value, (int, float)):
            raise ValueError(f'`{name}` must be either int or float')
    twt = np.asarray(twt)
    if twt.size != nsamples:
        raise ValueError(f'twt has {twt.size} samples, the traces {nsamples}')
    from .. import _ffi
    flag, idx = _ffi.GAIN_FLAG, _ffi.GAIN_PRM
    prm = np.zeros(_ffi.GAIN_NPRM)
    curves = np.ones((4, nsamples))
    flags = 0
    if (bias is not None) and (bias != 0.0):
        flags |= flag['bias']
        prm[idx['bias']] = bias
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        if (tpow is not None) and (tpow != 0.0):
            curves[0] = np.power(twt, tpow)
            # the first sample: t^tpow, except that a trace starting at t = 0 gets 0 there (also for tpow < 0)
            curves[0][0] = np.power(twt[0], tpow) if twt[0] != 0.0 else 0.0
            flags |= flag['tpow']
        if epow is not None and epow != 0.0:
            etpow_fact = np.power(twt, etpow)
            curves[1] = np.power(ebase, epow * etpow_fact) if ebase is not None else np.exp(epow * etpow_fact)
            flags |= flag['epow']
    if (gpow is not None) and (gpow != 0.0):
        flags |= flag['gpow']
        prm[idx['gpow']] = gpow
    if agc:
        dt = round(float(np.mean(np.diff(twt))) * 1e9) / 1e9    # the sampling interval, rounded to whole nanoseconds
        if agc_kind not in _ffi.AGC_KIND:
            raise ValueError(f'Unknown AGC kind "{agc_kind}"')
        win = get_AGC_samples(agc_win, dt)
        flags |= flag['agc']
        prm[idx['agc_win']] = win + 1 if win % 2 == 0 else win
        prm[idx['agc_kind']] = _ffi.AGC_KIND[agc_kind]
        prm[idx['agc_sqrt']] = bool(agc_sqrt)
    for name, val in (('clip', clip), ('pclip', pclip), ('nclip', nclip), ('qclip', qclip)):
        if val is not None:
            flags |= flag[name]
            prm[idx[name]] = val
    if linear is not None:
        curves[2] = np.linspace(min(linear), max(linear), twt.size, endpoint=True)
        flags |= flag['linear']
    if isinstance(pgc, dict):
        curves[3] = programmed_gain_control(twt, pgc)
        flags |= flag['pgc']
    if norm_rms:
        flags |= flag['norm_rms']
    if (scale is not None) and (scale != 1.0):
        flags |= flag['scale'] | (flag['norm'] if norm else 0)
        prm[idx['scale']] = scale
    prm[idx['flags']] = flags
    use_curves = flags & (flag['tpow'] | flag['epow'] | flag['linear'] | flag['pgc'])
    return prm, (curves if use_curves else None)


def gain(data, twt, tpow=0.0, epow=0.0, etpow=1.0, ebase=None, gpow=0.0, agc: bool = False, agc_win=0.05, agc_kind: str = 'rms',
         agc_sqrt: bool = False, clip=None, pclip=None, nclip=None, qclip=None, linear=None, pgc=None, bias=None, scale=1.0,
         norm: bool = False, norm_rms: bool = False, copy: bool = True, axis=-1):
    """Time-variant gain of a trace (1-D), section (2-D) or cube (3-D) along ``axis``, on the GPU (a Python restatement of the
    reference's port of Seismic Unix ``sugain``, see LICENSE_SeismicUnix of the reference).

    Same arguments, defaults and order of operations as the reference: bias; tpow (t^tpow, the first sample 0 when twt[0] == 0);
    epow / etpow / ebase; signed gpow; AGC (``agc_win`` seconds); clip, pclip, nclip; qclip (quantile of |x| per trace); linear;
    pgc; norm_rms (rms per trace); scale (or ``1 / scale`` with ``norm``).  The result is a new float32 array (``copy`` is
    accepted and the input is never modified).  Departure: qclip and norm_rms work per trace on 2-D and 3-D data as well (the
    reference broadcasts them only for a single trace)."""
    prm, curves = gain_tables(np.asarray(data).shape[axis], twt, tpow=tpow, epow=epow, etpow=etpow, ebase=ebase, gpow=gpow, agc=agc,
                              agc_win=agc_win, agc_kind=agc_kind, agc_sqrt=agc_sqrt, clip=clip, pclip=pclip, nclip=nclip, qclip=qclip,
                              linear=linear, pgc=pgc, bias=bias, scale=scale, norm=norm, norm_rms=norm_rms)
    from .. import _ffi
    return _ffi.apply_trace_op(data, axis, ('gain', prm, curves))


def rms(array, axis=None):
    """Root mean square amplitude(s) sqrt(sum(a^2) / N) over ``axis`` (None: the whole array, a scalar).  An integer axis runs on the
    GPU (one value per trace)."""
    from .. import _ffi
    if axis is None or isinstance(axis, (tuple, list)):
        a = np.asarray(array)
        n = a.size if axis is None else int(np.prod([a.shape[ax] for ax in axis]))
        return np.sqrt(np.sum(a ** 2, axis=None if axis is None else tuple(axis)) / n)
    _, refs = _ffi.apply_trace_op(array, axis, ('reduce', 2))
    return refs[0]


def rms_normalization(signal, axis=None):
    """``signal / rms(signal, axis)`` with a zero rms replaced by 1; an integer axis runs on the GPU."""
    if axis is None:
        signal = np.asarray(signal)
        r = rms(signal)
        return signal / (1.0 if r == 0.0 else r)
    from .. import _ffi
    prm = np.zeros(_ffi.GAIN_NPRM)
    prm[_ffi.GAIN_PRM['flags']] = _ffi.GAIN_FLAG['norm_rms']
    return _ffi.apply_trace_op(signal, axis, ('gain', prm, None))


def calc_reference_amplitude(traces, axis: int = None, scale: str = 'rms'):
    """Reference amplitude per trace: ``rms`` or ``max`` (``peak``) of |x| along ``axis``, 0 replaced by 1 (GPU for an integer axis)."""
    if scale not in ('rms', 'peak', 'max'):
        raise ValueError(f'unknown scale {scale!r}')
    if axis is None:
        a = np.asarray(traces)
        amp = rms(a) if scale == 'rms' else np.max(np.abs(a))
        return np.where(amp == 0.0, 1.0, amp)
    from .. import _ffi
    _, refs = _ffi.apply_trace_op(traces, axis, ('reduce', 0 if scale == 'rms' else 1))
    return refs[0]


def envelope(signal, axis=-1):
    """Envelope |hilbert(x)| along ``axis`` on the GPU (float32)."""
    from .. import _ffi
    x, ax = _time_first(signal, axis)
    return _time_back(_ffi.trace_ops(x, [envelope_op(x.shape[0])])[0], ax)


def get_resampled_twt(twt, n_resamples, n_samples):
    """TWT of ``n_resamples`` samples spanning the ``n_samples`` of ``twt``."""
    return np.arange(0, n_resamples) * (twt[1] - twt[0]) * n_samples / float(n_resamples) + twt[0]


def envelope_op(n):
    """``trace_ops`` operation of the analytic-signal modulus at length n: scipy.signal.hilbert's h (1, 2 ... 2, 1 at Nyquist, 0)."""
    h = np.zeros(n, np.float32)
    if n % 2 == 0:
        h[0] = h[n // 2] = 1
        h[1:n // 2] = 2
    else:
        h[0] = 1
        h[1:(n + 1) // 2] = 2
    return ('spectral', n, np.arange(n, dtype=np.int32) * 4, h, True, 1.0 / n, 1.0)


def resample_poly_op(n_in, up, down, window='hann'):
    """``trace_ops`` operation of ``scipy.signal.resample_poly(x, up, down, window=window)`` (integer up / down, constant padding)."""
    from .filter import firwin
    if up != int(up):
        raise ValueError('up must be an integer')
    if down != int(down):
        raise ValueError('down must be an integer')
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError('up and down must be >= 1')
    g = math.gcd(up, down)
    up //= g
    down //= g
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    if up == down == 1:
        return ('upfirdn', np.ones(1), 1, 1, 0, n_in)
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1. / max_rate, window=window) * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    h = np.concatenate((np.zeros(n_pre_pad), h))
    return ('upfirdn', h, up, down, n_pre_remove, n_out)


def resample_op(n_in, num, window=None):
    """``trace_ops`` operation of ``scipy.signal.resample(x, num, window=window)`` for real traces: the rfft bins kept (the periodic
    window applied in ifftshift order and folded), the Nyquist bin doubled (down) or halved (up), the inverse at length num,
    scaled by num / n_in."""
    from .filter import get_window
    nx, num = int(n_in), int(num)
    if num < 1:
        raise ValueError('num must be positive')
    wr = np.ones(nx // 2 + 1)
    if window is not None:
        w = np.fft.ifftshift(get_window(window, nx))
        wreal = w.copy()
        wreal[1:] += wreal[-1:0:-1]
        wreal[1:] *= 0.5
        wr = wreal[:nx // 2 + 1]
    n = min(num, nx)
    nyq = n // 2 + 1
    yfac = np.zeros(num // 2 + 1)
    ysrc = np.full(num // 2 + 1, -1, np.int64)
    keep = min(nyq, num // 2 + 1)
    yfac[:keep] = wr[:keep]
    ysrc[:keep] = np.arange(keep)
    if n % 2 == 0:
        if num < nx:
            yfac[n // 2] *= 2.0
        elif nx < num:
            yfac[n // 2] *= 0.5
    # the full spectrum of irfft(Y, num): Z[k] = Y[k] (k <= num // 2), conj(Y[num - k]) above; Im Y[0] and Im Y[num / 2] ignored
    src = np.full(num, -1, np.int32)
    fac = np.zeros(num, np.float32)
    for k in range(num):
        kk, op = (k, 0) if k <= num // 2 else (num - k, 1)
        if k == 0 or 2 * k == num:
            op = 2
        if ysrc[kk] >= 0:
            src[k] = ysrc[kk] * 4 + op
            fac[k] = yfac[kk]
    return ('spectral', num, src, fac, False, 1.0 / num, float(num) / float(nx))


def resample_poly(x, up, down, axis=0, window='hann'):
    """``scipy.signal.resample_poly(x, up, down, axis, window)`` on the GPU (float32; windows of ``functions.filter.WINDOWS``)."""
    xt, ax = _time_first(x, axis)
    return _time_back(_ffi.trace_ops(xt, [resample_poly_op(xt.shape[0], up, down, window)])[0], ax)


def resample(x, num, t=None, axis=0, window=None):
    """``scipy.signal.resample(x, num, axis=axis, window=window)`` of real data on the GPU (float32)."""
    if t is not None:
        raise NotImplementedError('resample with sample positions (t) is not implemented')
    xt, ax = _time_first(x, axis)
    return _time_back(_ffi.trace_ops(xt, [resample_op(xt.shape[0], num, window)])[0], ax)
