"""Float64 references of the step-11 trace operations, computed at test time from the float32 input with SciPy / NumPy
(tests/test_gpu_preproc_edges.py, tests/test_preproc_reference_host.py).  Time is on axis 0 ([nt][traces], the layout of
``_ffi.trace_ops``).  Nothing here imports the package: the filter designs, window tables and stage order are SciPy's / restated."""
import numpy as np
import scipy.fft
import scipy.signal as ss

from helpers import agc_numpy

# ---- the filter cases of the edge tests: (name, design arguments, expected sections, expected padlen) ---------------------------
# butter(N, 0.3): ceil(N / 2) sections; bandpass doubles the order: N sections; padlen = 3 * (2 * sections + 1 - zeros at the origin)
FILTER_DESIGNS = (
    [(f'low{n}', (2 * n - 1, 0.3, 'lowpass'), n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)]
    + [(f'band{n}', (n, [0.1, 0.4], 'bandpass'), n) for n in (1, 4, 7, 8, 9, 16, 17)]
    + [(f'high{n}', (2 * n, 0.2, 'highpass'), n) for n in (1, 8, 9)])


def design(args):
    """``(sos, zi, padlen)`` of ``butter(*args, output='sos')`` as scipy.signal.sosfiltfilt computes them."""
    sos = ss.butter(args[0], args[1], args[2], output='sos')
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    return sos, ss.sosfilt_zi(sos), 3 * int(ntaps)


def rel_l2(got, want):
    """Per-trace relative L2 error along axis 0 (an all-zero reference trace: the absolute error)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.linalg.norm(want, axis=0)
    return np.linalg.norm(got - want, axis=0) / np.where(den == 0.0, 1.0, den)


def traces(nt, ntr, seed):
    """float32 test traces [nt][ntr]: white noise plus a slow sinusoid and an offset (so the filter edges and the DC bin matter)."""
    rng = np.random.default_rng(seed)
    t = np.arange(nt)[:, None]
    x = rng.standard_normal((nt, ntr)) + 0.5 * np.sin(2 * np.pi * t * (0.01 + 0.002 * np.arange(ntr)[None, :])) + 0.25
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- sosfiltfilt ------------------------------------------------------------------------------------------------------------------
def sosfiltfilt(sos, x):
    return ss.sosfiltfilt(sos, np.asarray(x, np.float64), axis=0)


def odd_ext(x, n):
    """sosfiltfilt's padtype='odd' along axis 0: ``n`` samples mirrored through each end point, in the dtype of ``x``."""
    if n < 1:
        return x
    assert n < x.shape[0]
    return np.concatenate((2 * x[:1] - x[n:0:-1], x, 2 * x[-1:] - x[-2:-(n + 2):-1]), axis=0)


def sosfiltfilt_f32_storage(sos, x, padlen, group=8):
    """The float64 cascade with the signal rounded to float32 where the documented design stores it: after each group of ``group``
    sections, forward and backward (the last forward group's output is the end of the forward pass, the last backward group's the
    float32 result).  The odd extension is formed in float32 (``odd_ext`` below); every group starts from ``zi * ext[0]``, the
    backward groups from ``zi`` times the UNROUNDED last forward sample."""
    x = np.asarray(x, np.float32)
    sos = np.asarray(sos, np.float64)
    zi = ss.sosfilt_zi(sos)
    ext = odd_ext(x, padlen)
    assert ext.dtype == np.float32
    cuts = list(range(0, sos.shape[0], group))

    def cascade(sig, start):
        last = None
        for k in cuts:
            s = slice(k, k + group)
            y, _ = ss.sosfilt(sos[s], sig.astype(np.float64), axis=0, zi=zi[s][:, :, None] * start[None, None, :])
            last = y[-1].copy()
            sig = y.astype(np.float32)
        return sig, last

    fwd, y0 = cascade(ext, ext[0].astype(np.float64))
    bwd, _ = cascade(fwd[::-1], y0)
    out = bwd[::-1]
    return out[padlen:out.shape[0] - padlen] if padlen > 0 else out


# ---- resampling and envelope --------------------------------------------------------------------------------------------------
def resample_poly(x, up, down, window='hann'):
    return ss.resample_poly(np.asarray(x, np.float64), up, down, axis=0, window=window)


def resample(x, num, window=None):
    return ss.resample(np.asarray(x, np.float64), num, axis=0, window=window)


def envelope(x):
    return np.abs(ss.hilbert(np.asarray(x, np.float64), axis=0))


def _hilbert_h(n):
    h = np.zeros(n)
    if n % 2 == 0:
        h[0] = h[n // 2] = 1
        h[1:n // 2] = 2
    else:
        h[0] = 1
        h[1:(n + 1) // 2] = 2
    return h


def envelope_c64(x):
    """The envelope as scipy.fft computes it on float32 input (complex64 transforms): the single-precision yardstick."""
    x = np.asarray(x, np.float32)
    X = scipy.fft.fft(x, axis=0)
    assert X.dtype == np.complex64
    z = scipy.fft.ifft(X * _hilbert_h(x.shape[0]).astype(np.float32)[:, None], axis=0)
    assert z.dtype == np.complex64
    return np.abs(z)


def resample_c64(x, num, window=None):
    """scipy.signal.resample's arithmetic for real input, restated on scipy.fft's single-precision transforms."""
    x = np.asarray(x, np.float32)
    nx = x.shape[0]
    X = scipy.fft.rfft(x, axis=0)
    assert X.dtype == np.complex64
    if window is not None:
        w = scipy.fft.ifftshift(ss.get_window(window, nx))
        wr = w.copy()
        wr[1:] += wr[-1:0:-1]
        wr[1:] *= 0.5
        X = X * wr[:nx // 2 + 1].astype(np.float32)[:, None]
    n = min(num, nx)
    nyq = n // 2 + 1
    Y = np.zeros((num // 2 + 1, x.shape[1]), np.complex64)
    Y[:nyq] = X[:nyq]
    if n % 2 == 0:
        if num < nx:
            Y[n // 2] *= np.float32(2.0)
        elif nx < num:
            Y[n // 2] *= np.float32(0.5)
    y = scipy.fft.irfft(Y, num, axis=0)
    assert y.dtype == np.float32
    return y * np.float32(float(num) / float(nx))


# ---- gain stages (the reference's order: bias, tpow, epow, gpow | AGC | clip, pclip, nclip | qclip, linear, pgc | norm_rms, scale)
def quantile_abs(x, q):
    """np.quantile of |x| per trace in float64 (a trace with a NaN gives NaN)."""
    return np.quantile(np.abs(np.asarray(x, np.float64)), q, axis=0)


def qclip(x, q):
    """The qclip stage: |x| above the trace's quantile of |x| becomes quantile * sign(x), rounded to float32."""
    x = np.asarray(x, np.float32)
    thr = quantile_abs(x, q)[None, :]
    with np.errstate(invalid='ignore'):
        return np.where(np.abs(x).astype(np.float64) > thr, (thr * np.sign(x)).astype(np.float32), x)


def rms(x):
    """sqrt(sum(x^2) / nt) per trace: float32 squares (NumPy squares a float32 array in float32), summed in float64."""
    x = np.asarray(x, np.float32)
    return np.sqrt((x * x).astype(np.float64).sum(axis=0) / x.shape[0]).astype(np.float32)


def reference_amplitude(x, kind):
    """rms (kind 0), max |x| (kind 1) with 0 -> 1, or the plain rms (kind 2)."""
    x = np.asarray(x, np.float32)
    r = np.max(np.abs(x), axis=0) if kind == 1 else rms(x)
    return r if kind == 2 else np.where(r == 0.0, np.float32(1.0), r).astype(np.float32)


def balance(x, kind):
    x = np.asarray(x, np.float32)
    ref = reference_amplitude(x, kind)
    return x / ref[None, :], ref


def tpow_curve(twt, tpow):
    c = np.power(np.asarray(twt, np.float64), tpow)
    if twt[0] == 0.0:
        c[0] = 0.0
    return c


def pgc_curve(nt, nodes):
    """{sample index: gain}: linear interpolation in sample index, float32 (the reference's programmed gain control with the
    nodes already on samples)."""
    at = np.array(sorted(nodes))
    return np.interp(np.arange(nt), at, np.array([nodes[i] for i in at], np.float32)).astype(np.float32)


def gain_stages(x, tpow=None, agc_win=None, pclip=None, qclip_q=None, linear=None, pgc=None, norm_rms=False, scale=None):
    """The elementwise stages the edge tests use, in the reference's order, float32 as NumPy computes on a float32 array (the
    float64 curves multiply in float64 and round)."""
    v = np.asarray(x, np.float32).copy()
    if tpow is not None:
        v = (v.astype(np.float64) * tpow[:, None]).astype(np.float32)
    if agc_win is not None:
        v = agc_numpy.agc(v, agc_win, 'rms', axis=0)     # the step-15 AGC (rms, window in samples)
    if pclip is not None:
        v = np.where(v > np.float32(pclip), np.float32(pclip), v)
    if qclip_q is not None:
        v = qclip(v, qclip_q)
    if linear is not None:
        v = (v.astype(np.float64) * linear[:, None]).astype(np.float32)
    if pgc is not None:
        v = v * pgc[:, None]
    if norm_rms:
        v = v / reference_amplitude(v, 0)[None, :]
    if scale is not None:
        v = v * np.float32(scale)
    return v
