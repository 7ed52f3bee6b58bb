"""Small utilities mirrored from pseudo_3D_interpolation/functions/utils.py (only what the steps of this package use)."""
from functools import partial

import numpy as np

# shortest positional representation of a float (trailing zeros and point trimmed)
ffloat = partial(np.format_float_positional, trim='-')


def xprint(*args, kind: str = 'info', verbosity: int = 0, **kwargs) -> None:
    """print() with a coloured prefix, gated by verbosity (reference: functions/utils.py:57-76)."""
    verbosity = 1 if verbosity is True else verbosity
    table = {
        'info': ('\033[39m', '[INFO]  ', 1),
        'warning': ('\033[33m\033[1m', '[WARN]  ', 0),
        'error': ('\033[31m\033[1m', '[ERROR]  ', 0),
        'success': ('\033[32m', '[SUCCESS]  ', 1),
        'debug': ('\033[36m', '[DEBUG]  ', 2),
    }
    entry = table.get(kind)
    level = 1
    if entry is not None:
        color, label, level = entry
        args = [f'{color}{label}'] + [f'{a}' for a in args] + ['\033[0m']
    if level <= verbosity:
        print(*args, **kwargs)


def rescale(a, vmin=0, vmax=1):
    """Rescale to [vmin, vmax] using the array's own extrema (functions/utils.py:413-441)."""
    a = np.asarray(a)
    return rescale_dask(a, vmin=np.nanmin(a) if vmin is None else vmin, vmax=np.nanmax(a) if vmax is None else vmax)


def rescale_dask(a, vmin=0, vmax=1, amin=None, amax=None):
    """Rescale to [vmin, vmax] with given (global) extrema (functions/utils.py:444-473)."""
    a = np.asarray(a)
    amin = np.nanmin(a) if amin is None else amin
    amax = np.nanmax(a) if amax is None else amax
    if amin == amax:
        return a
    return vmin + (a - amin) * ((vmax - vmin) / (amax - amin))


def convert_twt(twt, unit_in: str, unit_out: str):
    """Convert TWT value(s) between 's', 'ms', 'us' and 'ns' (functions/utils.py:366-400, with its conversion factor)."""
    units = {'s': 1, 'ms': 1e-3, 'us': 1e-6, 'ns': 1e-9}
    if unit_in not in units:
        raise ValueError(f'Input unit `{unit_in}` is not supported. Choose one of {units.keys()}')
    if unit_out not in units:
        raise ValueError(f'Output unit `{unit_out}` is not supported. Choose one of {units.keys()}')
    fact_in, fact_out = units[unit_in], units[unit_out]
    factor = fact_in / fact_out if fact_in > fact_out else fact_in * fact_out
    return twt * factor


def dt_seconds(dt, units):
    """``dt`` in seconds; 'ns' divides by 1e-6 as the reference does."""
    if units == 'ms':
        return dt / 1000
    if units == 'ns':
        return dt / 1e-6
    return dt


def depth2twt(depth, v=1500):
    """Depth (m) -> two-way travel time (s) at sound velocity ``v`` (functions/utils.py:304-306)."""
    return depth / (v / 2)


def twt2samples(twt, dt, units='s'):
    """Two-way travel time (s) -> samples of ``dt`` [``units``] (functions/utils.py:319-328)."""
    return twt / dt_seconds(dt, units)


def depth2samples(depth, dt, v=1500, units='s'):
    """Depth (m) -> samples of ``dt`` [``units``] (functions/utils.py:336-347)."""
    return twt2samples(depth2twt(depth, v=v), dt_seconds(dt, units))
