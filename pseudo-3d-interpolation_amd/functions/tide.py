"""Step 6: tide prediction along a track and the tide compensation of a section (mirror of ``tpxo_tide_prediction.tide_predict`` in its
``track`` mode and of the reference's ``compensate_tide``).

The prediction runs on the GPU (csrc/p3d_tide.hip): `tide_model.load_subset` cuts the bounding box of the points out of the model files on the
host, the kernel interpolates the harmonic constants to every point and sums the nodal-corrected constituents at the point's time, in double
precision.  The compensation is the per-trace integer shift of step 5 (``p3d_static_shift``).  DESIGN.md 3.13 has the formulas and the departures."""
import numpy as np

from .. import _ffi
from .tide_model import CONSTITUENTS, load_subset
from .utils import depth2samples, dt_seconds, twt2samples, xprint

DEFAULT_CONSTITUENTS = ('m2', 's2', 'n2', 'k2', 'k1', 'o1', 'p1', 'q1')
EPOCH = np.datetime64('1992-01-01T00:00:00', 'us')
MSG_MINOR = ('the correction for minor constituents (`correct_minor`) is not implemented: it infers 18 constituents from tables of OTPS that this '
             'package does not hold')
MSG_FULL = "mode='full' (every time at every position) is not implemented; only mode='track' (one time per position) is"


def seconds_since_1992(times):
    """``datetime64`` values or ISO strings -> float64 seconds since 1992-01-01T00:00:00, taken as UTC without leap seconds; NaT gives NaN."""
    times = np.asarray(times)
    if times.dtype.kind != 'M':
        times = times.astype('datetime64[us]')
    delta = times.astype('datetime64[us]') - EPOCH
    out = delta.astype(np.int64) / 1e6
    return np.where(np.isnat(delta), np.nan, out)


def header_times(year, day, hour, minute, second):
    """The five trace-header words of the recording time -> ``datetime64[s]``.  The reference parses them with ``%Y-%j %H:%M:%S``: a four-digit
    year, day 1 ... 365 (366 in a leap year), hour 0 ... 23, minute and second 0 ... 59.  Anything else raises ``ValueError`` naming the first
    such trace."""
    year, day, hour, minute, second = (np.asarray(v, dtype=np.int64) for v in (year, day, hour, minute, second))
    leap = (year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0))
    bad = (year < 1000) | (year > 9999) | (day < 1) | (day > 365 + leap) | (hour < 0) | (hour > 23) | (minute < 0) | (minute > 59) | (second < 0) | (second > 59)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f'trace #{k} holds no valid recording time: year {year[k]}, day of year {day[k]}, {hour[k]}:{minute[k]}:{second[k]} '
                         f'({int(bad.sum())} such traces)')
    days = (year - 1970).astype('datetime64[Y]').astype('datetime64[D]') + (day - 1).astype('timedelta64[D]')
    return days.astype('datetime64[s]') + (hour * 3600 + minute * 60 + second).astype('timedelta64[s]')


def tide_predict(model_dir, lat, lon, times, constituents=DEFAULT_CONSTITUENTS, correct_minor=False, mode='track', device=0):
    """Tidal elevation (m) at the positions ``lat`` / ``lon`` (degrees) and the ``times`` (``datetime64`` or ISO strings, UTC), one time per
    position, from the model files in ``model_dir`` -- the call of ``tpxo_tide_prediction.tide_predict``.  A position whose four surrounding
    model nodes are dry gets NaN.  Non-finite input raises ``ValueError``; ``correct_minor`` and ``mode='full'`` raise ``NotImplementedError``
    before any file is touched."""
    if correct_minor:
        raise NotImplementedError(MSG_MINOR)
    if mode == 'full':
        raise NotImplementedError(MSG_FULL)
    if mode != 'track':
        raise ValueError(f"mode {mode!r} is neither 'track' nor 'full'")
    lat, lon = np.atleast_1d(np.asarray(lat, dtype=np.float64)), np.atleast_1d(np.asarray(lon, dtype=np.float64))
    t = np.atleast_1d(seconds_since_1992(times))
    if lat.ndim != 1 or not lat.shape == lon.shape == t.shape:
        raise ValueError(f"mode 'track' takes one time per position: lat {lat.shape}, lon {lon.shape}, times {t.shape}")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all() and np.isfinite(t).all()):
        raise ValueError('non-finite latitude, longitude or time')
    constituents = [constituents] if isinstance(constituents, str) else list(constituents)
    if lat.size == 0:
        return np.empty(0, np.float64)
    sub = load_subset(model_dir, constituents, lon, lat)
    return _ffi.tide_predict(sub.lon, lat, t, sub.hre, sub.him, sub.wet, sub.grid, sub.ids, device=device)


def compensate_tide(data, tide, dt, tide_units='meter', units='ms', v=1500, verbosity=1, device=0):
    """
    Apply the predicted tide to the traces of ``data`` (samples x traces): trace i moves up by ``offset[i]`` samples (down for a negative one),
    zeros fill the gap -- out[t] = in[t + offset].  ``tide`` is an elevation (``tide_units`` 'meter', converted with the sound velocity ``v``), a
    two-way travel time ('s' or 'ms', both taken as seconds as in the reference) or 'samples'; ``dt`` is the sample interval in ``units`` ('s',
    'ms'; 'ns' divides by 1e-6 as the reference does).  Offsets are ``np.around`` to int32 on the host, the shift is ``p3d_static_shift`` on the
    GPU.  A trace with |offset| >= the number of samples becomes zeros.  Returns float32 (samples x traces); the input is not modified.
    """
    dt = dt_seconds(dt, units)
    tide = np.asarray(tide)
    if tide_units == 'meter':
        tide_samples = depth2samples(tide, dt, v=v, units='s')
    elif tide_units in ['s', 'ms']:
        tide_samples = twt2samples(tide, dt, units='s')
    elif tide_units == 'samples':
        tide_samples = tide
    else:
        raise ValueError(f'Provided unknown unit < {tide_units} > for tide values.')
    if not np.isfinite(tide_samples).all():
        raise ValueError('non-finite tide values')
    data = np.asarray(data)
    if data.ndim != 2 or tide_samples.shape != (data.shape[1],):
        raise ValueError(f'a section of shape {data.shape} (samples x traces) and tide values of shape {tide_samples.shape}')
    ns = data.shape[0]
    offset = np.around(np.clip(tide_samples, -ns, ns), 0).astype('int32')        # beyond +-ns the trace is zeros either way
    for i in (np.flatnonzero(offset) if verbosity >= 2 else ()):
        xprint(f'trace #{i}:{offset[i]:>5}   ->   {"up" if offset[i] > 0 else "down"}: ({ns},)', kind='debug', verbosity=verbosity)
    section = np.ascontiguousarray(data.T, dtype=np.float32)
    if section.size == 0:
        return section.T.copy()
    return np.ascontiguousarray(_ffi.static_shift(section, -offset, device=device).T)


__all__ = ['CONSTITUENTS', 'DEFAULT_CONSTITUENTS', 'compensate_tide', 'header_times', 'seconds_since_1992', 'tide_predict']
