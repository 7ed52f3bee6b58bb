"""NumPy restatements of the step-15 AGC and iline / xline upsampling, the yardsticks of the GPU tests
(tests/test_gpu_postproc_agc.py, tests/test_gpu_postproc_upsample.py, tests/test_gpu_postproc_cli.py)."""
import numpy as np


def agc(x, win, kind='rms', squared=False, axis=0, return_gain=False):
    """AGC with zero padding along ``axis``: float32 squares, window sums in float64, float32 gain, ``x * (1 / g)``."""
    x = np.asarray(x, np.float32)
    win = win + 1 if win % 2 == 0 else win
    h = win // 2
    xt = np.moveaxis(x, axis, -1)
    pad = [(0, 0)] * (xt.ndim - 1) + [(h, h)]
    xp = np.pad(xt, pad)
    w = np.lib.stride_tricks.sliding_window_view(xp, win, axis=-1)
    if kind == 'rms':
        g = np.sqrt((w * w).astype(np.float64).mean(axis=-1)).astype(np.float32)
    elif kind == 'mean':
        g = w.astype(np.float64).mean(axis=-1).astype(np.float32)
    elif kind == 'median':
        g = np.median(w, axis=-1).astype(np.float32)
    else:
        raise ValueError(kind)
    g[g == 0] = 1
    y = xt * (np.float32(1) / g)
    if squared:
        y = np.sign(y) * y * y
    y, g = np.moveaxis(y, -1, axis), np.moveaxis(g, -1, axis)
    return (y, g) if return_gain else y


def interp_table(src, dst, method):
    """Per output coordinate: the source line and the weight towards the next one (linear / slinear), or the nearer source line
    with the lower one on an exact tie (nearest, weight 0)."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    i0 = np.clip(np.searchsorted(src, dst, side='right') - 1, 0, src.size - 1)
    nxt = np.minimum(i0 + 1, src.size - 1)
    span = src[nxt] - src[i0]
    w = np.where(span > 0, (dst - src[i0]) / np.where(span > 0, span, 1), 0.0)
    if method == 'nearest':
        i0 = np.where(w > 0.5, nxt, i0)
        w = np.zeros_like(w)
    return i0, w


def upsample(x, il_src, il_dst, xl_src, xl_dst, method='linear'):
    """Separable upsampling of a stack (n, nil, nxl) in float64: along iline, then along xline."""
    x = np.asarray(x)
    out = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    for axis, (src, dst) in ((1, (il_src, il_dst)), (2, (xl_src, xl_dst))):
        i0, w = interp_table(src, dst, method)
        i1 = np.minimum(i0 + 1, len(src) - 1)
        shape = [1, 1, 1]
        shape[axis] = -1
        w = w.reshape(shape)
        out = (1 - w) * np.take(out, i0, axis=axis) + w * np.take(out, i1, axis=axis)
    return out
