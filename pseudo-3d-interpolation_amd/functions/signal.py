"""Automatic gain control of step 15, mirrored from pseudo_3D_interpolation/functions/signal.py (``get_AGC_samples`` :302-322,
``AGC`` :325-409).  The gain runs in HIP (``p3d_agc``, include/p3d.h); only the reference's default zero padding is implemented."""
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
