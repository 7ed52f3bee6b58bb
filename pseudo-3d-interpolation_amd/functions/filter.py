"""Frequency filters of step 11, mirrored from pseudo_3D_interpolation/functions/filter.py (``filter_frequency`` :809-873 and its
partials), plus the small filter designs of ``scipy.signal`` that step 11 needs, restated in NumPy: Butterworth order selection
(``buttord``, including its band-stop branch with a bounded Brent minimisation), ``butter`` as second-order sections, ``sosfilt_zi``,
``firwin`` and the windows without parameters.  Only these tables are built on the host; the filtering runs in HIP
(``p3d_pre_sosfiltfilt_dev``, include/p3d.h).

The reference's ``bandpass`` maps ``[f1, f2, f3, f4]`` to ``wp = [f1, f4]`` and ``ws = [f2, f3]``: ``buttord`` reads that as a
BAND-STOP specification and moves the passband edges by its minimiser before ``butter(btype='bandpass')`` designs on the result.
That is kept, so ``Wn`` (and the output) match the reference.
"""
import math
from functools import partial

import numpy as np

from .. import _ffi

WINDOWS = ('hann', 'hamming', 'blackman', 'bartlett', 'boxcar')


# ---- windows ------------------------------------------------------------------------------------------------------------------
def get_window(window, nx, fftbins=True):
    """``scipy.signal.get_window`` for the windows without parameters (``WINDOWS``); periodic when ``fftbins`` (the default),
    symmetric otherwise."""
    name = window.lower() if isinstance(window, str) else window
    aliases = {'hanning': 'hann', 'han': 'hann', 'hamm': 'hamming', 'ham': 'hamming', 'black': 'blackman', 'blk': 'blackman',
               'bart': 'bartlett', 'brt': 'bartlett', 'box': 'boxcar', 'ones': 'boxcar', 'rect': 'boxcar', 'rectangular': 'boxcar'}
    name = aliases.get(name, name) if isinstance(name, str) else name
    if name not in WINDOWS:
        raise NotImplementedError(f'window {window!r} is not supported; supported windows: {", ".join(WINDOWS)}')
    m = int(nx)
    if m <= 1:
        return np.ones(max(m, 0))
    sym = not fftbins
    mm = m if sym else m + 1
    if name == 'boxcar':
        w = np.ones(mm)
    elif name == 'bartlett':
        n = np.arange(0, mm)
        w = np.where(np.less_equal(n, (mm - 1) / 2.0), 2.0 * n / (mm - 1), 2.0 - 2.0 * n / (mm - 1))
    else:
        a = {'hann': [0.5, 0.5], 'hamming': [0.54, 0.46], 'blackman': [0.42, 0.50, 0.08]}[name]
        fac = np.linspace(-np.pi, np.pi, mm)
        w = np.zeros(mm)
        for k in range(len(a)):
            w += a[k] * np.cos(k * fac)
    return w if sym else w[:-1]


def firwin(numtaps, cutoff, window='hamming'):
    """``scipy.signal.firwin(numtaps, cutoff, window=window)`` for a single low-pass cutoff (relative to Nyquist), scaled to unit
    gain at DC."""
    cutoff = float(cutoff)
    if not 0 < cutoff < 1:
        raise ValueError('Invalid cutoff frequency: frequencies must be greater than 0 and less than fs/2.')
    alpha = 0.5 * (numtaps - 1)
    m = np.arange(0, numtaps) - alpha
    h = cutoff * np.sinc(cutoff * m)
    h = h * get_window(window, numtaps, fftbins=False)
    return h / np.sum(h * np.cos(np.pi * m * 0.0))


# ---- Butterworth design ---------------------------------------------------------------------------------------------------------
def _fminbound(func, x1, x2, xatol=1e-5, maxfun=500):
    """Bounded scalar minimisation (Brent's method with golden sections), the stopping rule and step logic of
    ``scipy.optimize.fminbound``."""
    sqrt_eps = math.sqrt(2.2e-16)
    golden_mean = 0.5 * (3.0 - math.sqrt(5.0))
    a, b = x1, x2
    fulc = a + golden_mean * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    fx = func(x)
    num = 1
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = sqrt_eps * abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    while abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        golden = True
        if abs(e) > tol1:
            golden = False
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r = e
            e = rat
            if (abs(p) < abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = np.sign(xm - xf) + ((xm - xf) == 0)
                    rat = tol1 * si
            else:
                golden = True
        if golden:
            e = (a - xf) if xf >= xm else (b - xf)
            rat = golden_mean * e
        si = np.sign(rat) + (rat == 0)
        x = xf + si * max(abs(rat), tol1)
        fu = func(x)
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = sqrt_eps * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxfun:
            break
    return xf


def _band_stop_order(wp, ind, passb, stopb, gpass, gstop):
    """Butterworth order (not rounded) of a band-stop filter when passband edge ``ind`` is moved to ``wp``."""
    passb_c = passb.copy()
    passb_c[ind] = wp
    nat = stopb * (passb_c[0] - passb_c[1]) / (stopb ** 2 - passb_c[0] * passb_c[1])
    nat = min(abs(nat))
    gs = 10 ** (0.1 * abs(gstop))
    gp = 10 ** (0.1 * abs(gpass))
    return np.log10((gs - 1.0) / (gp - 1.0)) / (2 * np.log10(nat))


def buttord(wp, ws, gpass, gstop, fs):
    """``scipy.signal.buttord(wp, ws, gpass, gstop, analog=False, fs=fs)``: lowest Butterworth order and natural frequency."""
    if gpass <= 0.0:
        raise ValueError('gpass should be larger than 0.0')
    if gstop <= 0.0:
        raise ValueError('gstop should be larger than 0.0')
    if gpass > gstop:
        raise ValueError('gpass should be smaller than gstop')
    wp = 2 * np.atleast_1d(np.asarray(wp, dtype=float)) / fs
    ws = 2 * np.atleast_1d(np.asarray(ws, dtype=float)) / fs
    ftype = 2 * (len(wp) - 1) + 1
    if wp[0] >= ws[0]:
        ftype += 1
    passb = np.tan(np.pi * wp / 2.0)
    stopb = np.tan(np.pi * ws / 2.0)
    if ftype == 1:            # low
        nat = stopb / passb
    elif ftype == 2:          # high
        nat = passb / stopb
    elif ftype == 3:          # stop
        passb[0] = _fminbound(lambda w: _band_stop_order(w, 0, passb, stopb, gpass, gstop), passb[0], stopb[0] - 1e-12)
        passb[1] = _fminbound(lambda w: _band_stop_order(w, 1, passb, stopb, gpass, gstop), stopb[1] + 1e-12, passb[1])
        nat = (stopb * (passb[0] - passb[1])) / (stopb ** 2 - passb[0] * passb[1])
    else:                     # pass
        nat = (stopb ** 2 - passb[0] * passb[1]) / (stopb * (passb[0] - passb[1]))
    nat = min(abs(nat))
    gs = 10 ** (0.1 * abs(gstop))
    gp = 10 ** (0.1 * abs(gpass))
    order = int(math.ceil(np.log10((gs - 1.0) / (gp - 1.0)) / (2 * np.log10(nat))))
    try:
        w0 = (gp - 1.0) ** (-1.0 / (2.0 * order))
    except ZeroDivisionError:
        w0 = 1.0
    if ftype == 1:
        wn = w0 * passb
    elif ftype == 2:
        wn = passb / w0
    elif ftype == 3:
        wn = np.empty(2, float)
        discr = np.sqrt((passb[1] - passb[0]) ** 2 + 4 * w0 ** 2 * passb[0] * passb[1])
        wn[0] = ((passb[1] - passb[0]) + discr) / (2 * w0)
        wn[1] = ((passb[1] - passb[0]) - discr) / (2 * w0)
        wn = np.sort(abs(wn))
    else:
        w0 = np.array([-w0, w0], float)
        wn = -w0 * (passb[1] - passb[0]) / 2.0 + np.sqrt(w0 ** 2 / 4.0 * (passb[1] - passb[0]) ** 2 + passb[0] * passb[1])
        wn = np.sort(abs(wn))
    wn = (2.0 / np.pi) * np.arctan(wn)
    if len(wn) == 1:
        wn = wn[0]
    return order, wn * fs / 2


def _cplxreal(z):
    """Split into complex values with positive imaginary part (one per conjugate pair) and real values, in scipy's order."""
    z = np.atleast_1d(z)
    if z.size == 0:
        return z, z
    tol = 100 * np.finfo((1.0 * z).dtype).eps
    z = z[np.lexsort((abs(z.imag), z.real))]
    real_idx = abs(z.imag) <= tol * abs(z)
    zr = z[real_idx].real
    if len(zr) == len(z):
        return np.array([]), zr
    z = z[~real_idx]
    zp = z[z.imag > 0]
    zn = z[z.imag < 0]
    if len(zp) != len(zn):
        raise ValueError('Array contains complex value with no matching conjugate.')
    same_real = np.diff(zp.real) <= tol * abs(zp[:-1])
    diffs = np.diff(np.concatenate(([0], same_real, [0])))
    starts, stops = np.nonzero(diffs > 0)[0], np.nonzero(diffs < 0)[0]
    for i in range(len(starts)):
        s, e = starts[i], stops[i] + 1
        for chunk in (zp[s:e], zn[s:e]):
            chunk[...] = chunk[np.lexsort([abs(chunk.imag)])]
    if any(abs(zp - zn.conj()) > tol * abs(zn)):
        raise ValueError('Array contains complex value with no matching conjugate.')
    return (zp + zn.conj()) / 2, zr


def _nearest_idx(fro, to, which):
    order = np.argsort(np.abs(fro - to))
    mask = np.isreal(fro[order])
    if which == 'complex':
        mask = ~mask
    return order[np.nonzero(mask)[0][0]]


def _poly2(r, k):
    """k * poly([r1, r2]) as NumPy's ``poly`` forms it; real when the roots are real or a conjugate pair."""
    a = np.ones(1, complex)
    for root in r:
        a = np.convolve(a, np.array([1, -root]))
    return (k * a).real


def zpk2sos(z, p, k):
    """``scipy.signal.zpk2sos(z, p, k)`` with the default ('nearest') pairing."""
    z = np.asarray(z, complex)
    p = np.asarray(p, complex)
    if len(z) == len(p) == 0:
        return np.array([[k, 0., 0., 1., 0., 0.]])
    p = np.concatenate((p, np.zeros(max(len(z) - len(p), 0))))
    z = np.concatenate((z, np.zeros(max(len(p) - len(z), 0))))
    nsec = (max(len(p), len(z)) + 1) // 2
    if len(p) % 2 == 1:
        p = np.concatenate((p, [0.]))
        z = np.concatenate((z, [0.]))
    z = np.concatenate(_cplxreal(z))
    p = np.concatenate(_cplxreal(p))
    p_sos = np.zeros((nsec, 2), np.complex128)
    z_sos = np.zeros_like(p_sos)
    for si in range(nsec):
        p1_idx = np.argmin(np.abs(1 - np.abs(p)))
        p1 = p[p1_idx]
        p = np.delete(p, p1_idx)
        if np.isreal(p1) and np.isreal(p).sum() == 0:
            z1_idx = _nearest_idx(z, p1, 'real')
            z1 = z[z1_idx]
            z = np.delete(z, z1_idx)
            p2 = z2 = 0
        else:
            if not np.isreal(p1) and np.isreal(z).sum() == 1:
                z1_idx = _nearest_idx(z, p1, 'complex')
            else:
                z1_idx = np.argmin(np.abs(p1 - z))
            z1 = z[z1_idx]
            z = np.delete(z, z1_idx)
            if not np.isreal(p1):
                if not np.isreal(z1):
                    p2, z2 = p1.conj(), z1.conj()
                else:
                    p2 = p1.conj()
                    z2_idx = _nearest_idx(z, p1, 'real')
                    z2 = z[z2_idx]
                    z = np.delete(z, z2_idx)
            else:
                if not np.isreal(z1):
                    z2 = z1.conj()
                    p2_idx = _nearest_idx(p, z1, 'real')
                    p2 = p[p2_idx]
                else:
                    idx = np.nonzero(np.isreal(p))[0]
                    p2_idx = idx[np.argmin(np.abs(np.abs(p[idx]) - 1))]
                    p2 = p[p2_idx]
                    z2_idx = _nearest_idx(z, p2, 'real')
                    z2 = z[z2_idx]
                    z = np.delete(z, z2_idx)
                p = np.delete(p, p2_idx)
        p_sos[si] = [p1, p2]
        z_sos[si] = [z1, z2]
    p_sos = p_sos[::-1]
    z_sos = z_sos[::-1]
    sos = np.zeros((nsec, 6))
    for si in range(nsec):
        sos[si, :3] = _poly2(z_sos[si], k if si == 0 else 1.0)
        sos[si, 3:] = _poly2(p_sos[si], 1.0)
    return sos


def butter(N, Wn, btype, fs):
    """``scipy.signal.butter(N, Wn, btype=btype, output='sos', fs=fs)`` of a digital filter."""
    Wn = 2 * np.asarray(Wn, dtype=float) / fs
    if np.any(Wn <= 0) or np.any(Wn >= 1):
        raise ValueError(f'Digital filter critical frequencies must be 0 < Wn < fs/2 (fs={fs} -> fs/2={fs / 2})')
    m = np.arange(-N + 1, N, 2)
    p = -np.exp(1j * np.pi * m / (2 * N))
    z = np.array([])
    k = 1
    fs2 = 2.0
    warped = 2 * fs2 * np.tan(np.pi * Wn / fs2)
    degree = len(p) - len(z)
    if btype == 'lowpass':
        wo = float(warped)
        z, p, k = wo * z, wo * p, k * wo ** degree
    elif btype == 'highpass':
        wo = float(warped)
        k = k * np.real(np.prod(-z) / np.prod(-p))
        z, p = np.append(wo / z, np.zeros(degree)), wo / p
    elif btype == 'bandpass':
        bw = float(warped[1] - warped[0])
        wo = float(np.sqrt(warped[0] * warped[1]))
        z_lp = (z * bw / 2).astype(complex)
        p_lp = (p * bw / 2).astype(complex)
        z = np.concatenate((z_lp + np.sqrt(z_lp ** 2 - wo ** 2), z_lp - np.sqrt(z_lp ** 2 - wo ** 2)))
        p = np.concatenate((p_lp + np.sqrt(p_lp ** 2 - wo ** 2), p_lp - np.sqrt(p_lp ** 2 - wo ** 2)))
        z = np.append(z, np.zeros(degree))
        k = k * bw ** degree
    else:
        raise ValueError(f'unsupported btype {btype!r}')
    # bilinear transform (fs = 2 after the prewarp)
    degree = len(p) - len(z)
    fs4 = 2.0 * fs2
    z_z = (fs4 + z) / (fs4 - z)
    p_z = (fs4 + p) / (fs4 - p)
    z_z = np.append(z_z, -np.ones(degree))
    k_z = k * np.real(np.prod(fs4 - z) / np.prod(fs4 - p))
    return zpk2sos(z_z, p_z, k_z)


def lfilter_zi(b, a):
    """``scipy.signal.lfilter_zi`` of one section (a[0] == 1)."""
    b = np.asarray(b, float)
    a = np.asarray(a, float)
    if a[0] != 1.0:
        b, a = b / a[0], a / a[0]
    n = max(len(a), len(b))
    companion = np.zeros((n - 1, n - 1))
    companion[0, :] = -a[1:] / a[0]
    companion[list(range(1, n - 1)), list(range(0, n - 2))] = 1
    i_minus_a = np.eye(n - 1) - companion.T
    return np.linalg.solve(i_minus_a, b[1:] - a[1:] * b[0])


def sosfilt_zi(sos):
    """``scipy.signal.sosfilt_zi``: steady-state initial states of the cascade for a unit step."""
    sos = np.asarray(sos, float)
    zi = np.empty((sos.shape[0], 2))
    scale = 1.0
    for s in range(sos.shape[0]):
        b, a = sos[s, :3], sos[s, 3:]
        zi[s] = scale * lfilter_zi(b, a)
        scale *= b.sum() / a.sum()
    return zi


def sos_padlen(sos):
    """sosfiltfilt's default pad length: 3 * (2 * nsec + 1 - min(#(b2 == 0), #(a2 == 0)))."""
    sos = np.asarray(sos)
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    return 3 * int(ntaps)


def design_filter(freqs, fs, filter_type, gpass=1, gstop=10):
    """The reference's filter design (``filter_frequency`` without the data): ``(N, Wn, sos)``."""
    corners = list(freqs)
    bad = ValueError('Invalid filter frequencies!')
    if filter_type == 'bandpass':
        # passband edges: the outer corners; stopband edges: the inner ones (buttord reads this as a band stop, see the module doc)
        if corners != sorted(corners):
            raise bad
        wp, ws = [corners[0], corners[-1]], [corners[1], corners[2]]
    elif filter_type in ('lowpass', 'highpass'):
        wp, ws = corners
        # a low-pass keeps what lies below its stopband edge, a high-pass what lies above it
        inverted = wp > ws if filter_type == 'lowpass' else wp < ws
        if inverted:
            raise bad
    else:
        raise ValueError(f'unknown filter type {filter_type!r}')
    N, Wn = buttord(wp, ws, gpass, gstop, fs=fs)
    sos = butter(N, Wn, btype=filter_type, fs=fs)
    return N, Wn, sos


def sosfiltfilt(sos, x, axis=-1, device=0):
    """``scipy.signal.sosfiltfilt(sos, x, axis)`` (odd padding, default pad length) on the GPU; float32 result."""
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    padlen = sos_padlen(sos)
    n = np.asarray(x).shape[axis]
    if n <= padlen:
        raise ValueError(f'The length of the input vector x must be greater than padlen, which is {padlen}.')
    return _ffi.apply_trace_op(x, axis, ('filter', sos, sosfilt_zi(sos), padlen), device=device)


def filter_frequency(data: np.ndarray, freqs: list, fs: float, filter_type: str, gpass: int = 1, gstop: int = 10, axis: int = -1):
    """Zero-phase Butterworth filter of ``data`` along ``axis`` from passband / stopband corner frequencies (same unit as ``fs``):

      - ``bandpass``: freqs = [f1, f2, f3, f4]
      - ``lowpass``:  freqs = [f_stopband, f_cutoff]
      - ``highpass``: freqs = [f_cutoff, f_stopband]

    Same signature, errors and design as the reference; the filtering runs on the GPU and returns float32 (the reference returns
    scipy's float64)."""
    _, _, sos = design_filter(freqs, fs, filter_type, gpass, gstop)
    return sosfiltfilt(sos, data, axis=axis)


bandpass_filter = partial(filter_frequency, filter_type='bandpass')
lowpass_filter = partial(filter_frequency, filter_type='lowpass')
highpass_filter = partial(filter_frequency, filter_type='highpass')


def moving_window_2D(a, w, dx=1, dy=1, writeable=False):
    """All windows of shape ``w`` = (rows, columns) over the last two axes of ``a`` with steps ``dy`` (rows) and ``dx`` (columns), as a
    strided view of shape (..., (rows - w[0]) // dy + 1, (columns - w[1]) // dx + 1, w[0], w[1]) (reference: functions/filter.py,
    ``moving_window_2D``; NumPy only -- step 8 itself runs on the GPU, functions/despike.py)."""
    a = np.asarray(a)
    w = tuple(w)
    nrow, ncol = (a.shape[-2] - w[-2]) // dy + 1, (a.shape[-1] - w[-1]) // dx + 1
    return np.lib.stride_tricks.as_strided(a, shape=a.shape[:-2] + (nrow, ncol) + w,
                                           strides=a.strides[:-2] + (a.strides[-2] * dy, a.strides[-1] * dx) + a.strides[-2:], writeable=writeable)


# ---- step 2: smoothing of a coordinate profile ----------------------------------------------------------------------------------
SMOOTH_WINDOWS = {'flat': np.ones, 'hanning': np.hanning, 'hamming': np.hamming, 'bartlett': np.bartlett, 'blackman': np.blackman}


def _line_fit(values):
    """Slope and intercept of the least-squares line through ``values`` at 0, 1, ... (the minimum-norm solution for a single value)."""
    design = np.column_stack([np.arange(values.size), np.ones(values.size)])
    return np.linalg.lstsq(design, values, rcond=None)[0]


def smooth_padded(data, window_len, window='hanning'):
    """Host half of :func:`smooth` for an odd ``window_len`` >= 3: the signal with ``window_len // 2`` samples added at each end on the
    least-squares lines through its first and its last ``window_len // 2`` samples, and the window normalised to a sum of 1."""
    half = window_len // 2
    m0, c0 = _line_fit(data[:half])
    m1, c1 = _line_fit(data[-half:])
    padded = np.r_[np.arange(-half, 0, 1) * m0 + c0, data, np.arange(half, 2 * half) * m1 + c1]
    w = np.asarray(SMOOTH_WINDOWS[window](window_len), dtype=np.float64)
    return padded, w / w.sum()


def smooth(data, window_len=11, window='hanning', device=0):
    """Smooth a 1-D array with a normalised window of ``window_len`` samples (reference: functions/filter.py ``smooth``, the SciPy cookbook's
    recipe with linearly extrapolated ends).  An even length becomes the next odd one; below 3 the input is returned as it is.  The padded signal
    and the window are built on the host (`smooth_padded`), the convolution runs on the GPU in double (``p3d_proj_smooth_dev``).  The order of
    the checks, and so which ``ValueError`` an input meets, is the reference's."""
    if data.ndim != 1:
        raise ValueError('smooth only accepts 1 dimension arrays.')
    if data.size < window_len:
        raise ValueError(f'Input data should be longer ({data.size}) than the window length ({window_len}).')
    if window_len < 3:
        return data
    window_len += 1 - window_len % 2
    if window not in SMOOTH_WINDOWS:
        raise ValueError("Window is one of 'flat', 'hanning', 'hamming', 'bartlett', 'blackman'")
    padded, w = smooth_padded(np.asarray(data, dtype=np.float64), window_len, window)
    return _ffi.proj_smooth(padded, w, device=device)
