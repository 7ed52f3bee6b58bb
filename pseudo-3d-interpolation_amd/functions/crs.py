"""Coordinate reference systems of step 2 without third-party packages: a small parser and the transformation between geographic
coordinates and transverse Mercator grids on the GPU (HIP unit ``p3d_proj``).

There is no EPSG database and there are no datum shifts.  What is understood (case-insensitive):

  * ``EPSG:4326`` (WGS84) and ``EPSG:4258`` (ETRS89, GRS80): geographic, degrees;
  * ``EPSG:32601`` ... ``32660`` / ``EPSG:32701`` ... ``32760``: WGS84 / UTM north / south;
  * ``EPSG:25828`` ... ``25838``: ETRS89 / UTM north (GRS80);
  * PROJ.4 strings ``+proj=longlat``, ``+proj=utm +zone=Z [+south]`` and ``+proj=tmerc +lat_0= +lon_0= +k= | +k_0= +x_0= +y_0=``, each with
    ``+datum=WGS84`` or ``+ellps=WGS84 | GRS80`` (WGS84 when neither is given; ``+units=m``, ``+no_defs``, ``+type=crs`` and ``+towgs84=0,...``
    are accepted and ignored).

Anything else, and a transformation between different ellipsoids, raises ``NotImplementedError`` with this list."""
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .. import _ffi

ELLIPSOIDS = {'WGS84': (6378137.0, 1 / 298.257223563), 'GRS80': (6378137.0, 1 / 298.257222101)}
UTM_K0, UTM_X0, UTM_Y0_SOUTH = 0.9996, 500000.0, 10000000.0
ACCEPTED = ('accepted: EPSG:4326, EPSG:4258, EPSG:32601-32660, EPSG:32701-32760, EPSG:25828-25838, and the PROJ.4 strings "+proj=longlat", '
            '"+proj=utm +zone=Z [+south]", "+proj=tmerc +lat_0 +lon_0 +k|+k_0 +x_0 +y_0" with +datum=WGS84 or +ellps=WGS84|GRS80 '
            '(no EPSG database, no datum shifts, no projection other than transverse Mercator)')


@dataclass(frozen=True)
class CRS:
    kind: str                       # 'geographic' or 'tmerc'
    a: float
    f: float
    lon0: float = 0.0               # degrees
    lat0: float = 0.0               # degrees
    k0: float = 1.0
    x0: float = 0.0
    y0: float = 0.0
    epsg: Optional[int] = None

    @property
    def is_projected(self):
        return self.kind == 'tmerc'

    @property
    def is_geographic(self):
        return self.kind == 'geographic'

    def to_epsg(self):
        return self.epsg

    @property
    def prm(self):
        """(a, f, lon0_deg, lat0_deg, k0, x0, y0): the parameter block of ``p3d_proj_tmerc``."""
        return np.array([self.a, self.f, self.lon0, self.lat0, self.k0, self.x0, self.y0], np.float64)


def _utm(zone, south, ellps, epsg):
    if not 1 <= zone <= 60:
        raise NotImplementedError(f'UTM zone {zone} does not exist; {ACCEPTED}')
    a, f = ELLIPSOIDS[ellps]
    return CRS('tmerc', a, f, lon0=6.0 * zone - 183.0, lat0=0.0, k0=UTM_K0, x0=UTM_X0, y0=UTM_Y0_SOUTH if south else 0.0, epsg=epsg)


def _from_epsg(code, text):
    if code == 4326:
        return CRS('geographic', *ELLIPSOIDS['WGS84'], epsg=code)
    if code == 4258:
        return CRS('geographic', *ELLIPSOIDS['GRS80'], epsg=code)
    if 32601 <= code <= 32660:
        return _utm(code - 32600, False, 'WGS84', code)
    if 32701 <= code <= 32760:
        return _utm(code - 32700, True, 'WGS84', code)
    if 25828 <= code <= 25838:
        return _utm(code - 25800, False, 'GRS80', code)
    raise NotImplementedError(f'CRS {text!r}: EPSG code {code} is not known here; {ACCEPTED}')


IGNORED = {'units': {'m'}, 'no_defs': {None}, 'type': {'crs'}, 'wktext': {None}, 'towgs84': None}


def _from_proj4(text):
    words = {}
    for token in text.split():
        if not token.startswith('+'):
            raise NotImplementedError(f'CRS {text!r}: cannot read {token!r}; {ACCEPTED}')
        key, _, value = token[1:].partition('=')
        words[key.lower()] = value if value else None

    def number(key, default):
        value = words.pop(key, None)
        if value is None:
            return default
        try:
            return float(value)
        except ValueError:
            raise NotImplementedError(f'CRS {text!r}: +{key}={value} is not a number; {ACCEPTED}') from None

    proj = (words.pop('proj', None) or '').lower()
    datum, ellps = words.pop('datum', None), words.pop('ellps', None)
    if datum is not None and datum.upper() != 'WGS84':
        raise NotImplementedError(f'CRS {text!r}: datum {datum}; {ACCEPTED}')
    name = (ellps or datum or 'WGS84').upper()
    if name not in ELLIPSOIDS or (datum is not None and ellps is not None and ellps.upper() != 'WGS84'):
        raise NotImplementedError(f'CRS {text!r}: ellipsoid {ellps}; {ACCEPTED}')
    a, f = ELLIPSOIDS[name]
    if proj in ('longlat', 'latlong', 'lonlat', 'latlon'):
        crs = CRS('geographic', a, f)
    elif proj == 'utm':
        zone = number('zone', None)
        if zone is None or zone != int(zone):
            raise NotImplementedError(f'CRS {text!r}: +proj=utm needs +zone=1...60; {ACCEPTED}')
        south = 'south' in words
        words.pop('south', None)
        zone = int(zone)
        crs = _utm(zone, south, name, ((32700 if south else 32600) + zone) if name == 'WGS84' and 1 <= zone <= 60 else None)
    elif proj == 'tmerc':
        if 'k' in words and 'k_0' in words:
            raise NotImplementedError(f'CRS {text!r}: both +k and +k_0; {ACCEPTED}')
        k0 = number('k', None) if 'k' in words else number('k_0', 1.0)
        crs = CRS('tmerc', a, f, lon0=number('lon_0', 0.0), lat0=number('lat_0', 0.0), k0=k0, x0=number('x_0', 0.0), y0=number('y_0', 0.0))
        if not (crs.k0 > 0 and abs(crs.lat0) <= 90 and abs(crs.lon0) <= 360 and np.isfinite(crs.prm).all()):
            raise NotImplementedError(f'CRS {text!r}: scale, origin or offsets out of range; {ACCEPTED}')
    else:
        raise NotImplementedError(f'CRS {text!r}: projection {proj or None}; {ACCEPTED}')
    for key, value in words.items():
        if key not in IGNORED or (IGNORED[key] is not None and (value.lower() if value else None) not in IGNORED[key]):
            raise NotImplementedError(f'CRS {text!r}: parameter +{key} is not supported; {ACCEPTED}')
    return crs


def parse_crs(text):
    """The :class:`CRS` of an EPSG code (``'EPSG:32760'``, ``'epsg:4326'``, a bare integer) or a PROJ.4 string; ``NotImplementedError`` with the
    list of accepted forms for anything else."""
    if isinstance(text, CRS):
        return text
    if isinstance(text, (int, np.integer)):
        return _from_epsg(int(text), f'EPSG:{int(text)}')
    if not isinstance(text, str):
        raise NotImplementedError(f'CRS {text!r}; {ACCEPTED}')
    stripped = text.strip()
    match = re.fullmatch(r'(?:epsg\s*:\s*)?(\d+)', stripped, re.IGNORECASE)
    if match:
        return _from_epsg(int(match.group(1)), stripped)
    if stripped.startswith('+'):
        return _from_proj4(stripped)
    raise NotImplementedError(f'CRS {text!r} is neither an EPSG code nor a PROJ.4 string; {ACCEPTED}')


def _same(a, b):
    return (a.kind, a.a, a.f, a.lon0, a.lat0, a.k0, a.x0, a.y0) == (b.kind, b.a, b.f, b.lon0, b.lat0, b.k0, b.x0, b.y0)


def transform(crs_src, crs_dst, x, y, device=0):
    """Coordinates ``x`` (longitude or easting), ``y`` (latitude or northing) of ``crs_src`` in ``crs_dst``, in this order for both
    (``always_xy``); geographic coordinates are degrees.  Returns two float64 arrays.  Geographic -> grid is the forward projection, grid ->
    geographic the inverse, grid -> grid the inverse followed by the forward one on the device (the intermediate degrees stay there); an
    identical pair, and two geographic systems of one ellipsoid, are a copy.  Any non-finite result raises ``ValueError``."""
    crs_src, crs_dst = parse_crs(crs_src), parse_crs(crs_dst)
    if (crs_src.a, crs_src.f) != (crs_dst.a, crs_dst.f):
        raise NotImplementedError(f'source and destination CRS are on different ellipsoids (a datum shift); {ACCEPTED}')
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError(f'x {x.shape} and y {y.shape} differ in shape')
    if _same(crs_src, crs_dst) or (crs_src.is_geographic and crs_dst.is_geographic) or x.size == 0:
        ox, oy = x.copy(), y.copy()
    elif crs_src.is_geographic:
        ox, oy = _ffi.proj_tmerc(x, y, crs_dst.prm, inverse=False, device=device)
    elif crs_dst.is_geographic:
        ox, oy = _ffi.proj_tmerc(x, y, crs_src.prm, inverse=True, device=device)
    else:
        ox, oy = _grid_to_grid(crs_src, crs_dst, x, y, device)
    if not (np.isfinite(ox).all() and np.isfinite(oy).all()):
        raise ValueError('the transformation gave non-finite coordinates (non-finite input, or a point the projection cannot hold)')
    return ox, oy


def _grid_to_grid(crs_src, crs_dst, x, y, device):
    shape, n = x.shape, x.size
    dx, dy = _ffi.DeviceArray((n,), np.float64, device), _ffi.DeviceArray((n,), np.float64, device)
    try:
        dx.upload(np.ascontiguousarray(x).ravel())
        dy.upload(np.ascontiguousarray(y).ravel())
        _ffi.proj_tmerc_dev(dx.ptr, dy.ptr, n, crs_src.prm, True, dx.ptr, dy.ptr, device)
        _ffi.proj_tmerc_dev(dx.ptr, dy.ptr, n, crs_dst.prm, False, dx.ptr, dy.ptr, device)
        return dx.download().reshape(shape), dy.download().reshape(shape)
    finally:
        dx.free()
        dy.free()
