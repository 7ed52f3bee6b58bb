"""Reader of a TPXO9-atlas style tide model for step 6, NumPy only: a parser of the netCDF classic header and the subset of the elevation
constants around a set of points.

Layout assumed (unpinned, no model file was at hand): the model directory holds one elevation file per constituent,
``h_<con>_*.nc``, and optionally one grid file ``grid_*.nc``.  Dimensions ``nx``, ``ny``; ``lon_z(nx)`` and ``lat_z(ny)`` doubles in degrees, both
rising uniformly, the longitudes covering the circle (``nx * dlon`` = 360); ``hRe(nx, ny)`` and ``hIm(nx, ny)`` int32 in millimetres with the
longitude as the slow axis; the grid file holds the depth ``hz(nx, ny)``, a node is wet where ``hz > 0``; without a grid file every node is wet.

The files are netCDF classic (magic ``CDF\\x01``, or ``CDF\\x02`` with 64-bit offsets).  Only the header is parsed; the fixed-size variables are
handed out as big-endian ``np.memmap`` views, so a file of half a gigabyte is never read whole: `load_subset` slices the rows of the bounding box
and copies those.  A netCDF-4 (HDF5) file goes through h5py where that is installed."""
import glob
import os
import struct
from dataclasses import dataclass

import numpy as np

from .backends import h5py_enabled

CONSTITUENTS = ('m2', 's2', 'n2', 'k2', 'k1', 'o1', 'p1', 'q1', 'm4', 'mf', '2n2', 'mm', 'mn4', 'ms4')     # id = position (include/p3d.h)
HDF5_MAGIC = b'\x89HDF\r\n\x1a\n'
NC_DIMENSION, NC_VARIABLE, NC_ATTRIBUTE = 10, 11, 12
NC_TYPES = {1: '>i1', 2: 'S1', 3: '>i2', 4: '>i4', 5: '>f4', 6: '>f8'}
UNIFORM = 1e-9          # of the spacing


class _Cursor:
    def __init__(self, fh, path):
        self.fh, self.path = fh, path

    def take(self, n):
        raw = self.fh.read(n)
        if len(raw) != n:
            raise ValueError(f'{self.path}: the netCDF header ends early')
        return raw

    def int32(self):
        return struct.unpack('>i', self.take(4))[0]

    def int64(self):
        return struct.unpack('>q', self.take(8))[0]

    def count(self):
        n = self.int32()
        if n < 0:
            raise ValueError(f'{self.path}: negative count in the netCDF header')
        return n

    def name(self):
        n = self.count()
        return self.take(n + (-n) % 4)[:n].decode('utf-8')

    def values(self, nc_type, n):
        if nc_type not in NC_TYPES:
            raise ValueError(f'{self.path}: netCDF type {nc_type} is not one of the classic format')
        dt = np.dtype(NC_TYPES[nc_type])
        nbytes = n * dt.itemsize
        raw = self.take(nbytes + (-nbytes) % 4)[:nbytes]
        if nc_type == 2:
            return raw.rstrip(b'\x00').decode('utf-8', 'replace')
        return np.frombuffer(raw, dt).astype(dt.newbyteorder('='))

    def tagged(self, tag, what):
        """Number of entries of a header list: the tag and the count, or two zeros for an absent list."""
        got, n = self.int32(), self.count()
        if got == 0 and n == 0:
            return 0
        if got != tag:
            raise ValueError(f'{self.path}: expected the {what} list in the netCDF header, found tag {got}')
        return n

    def attributes(self):
        out = {}
        for _ in range(self.tagged(NC_ATTRIBUTE, 'attribute')):
            name = self.name()
            nc_type = self.int32()
            out[name] = self.values(nc_type, self.count())
        return out


class ClassicFile:
    """The header of a netCDF classic file: ``dims`` (name -> length), ``attrs`` and ``variables`` (name -> dict of dtype, shape, dims, begin,
    attrs, record).  ``var(name)`` is a read-only big-endian memory map of a fixed-size variable."""

    def __init__(self, path):
        self.path = path
        with open(path, 'rb') as fh:
            magic = fh.read(4)
            if magic[:3] != b'CDF' or magic[3:] not in (b'\x01', b'\x02'):
                raise ValueError(f'{path}: not a netCDF classic file (magic {magic!r})')
            wide = magic[3:] == b'\x02'
            cur = _Cursor(fh, path)
            self.numrecs = cur.int32()
            names, lengths = [], []
            for _ in range(cur.tagged(NC_DIMENSION, 'dimension')):
                names.append(cur.name())
                lengths.append(cur.count())
            self.dims = dict(zip(names, lengths))
            self.attrs = cur.attributes()
            self.variables = {}
            for _ in range(cur.tagged(NC_VARIABLE, 'variable')):
                name = cur.name()
                dimids = [cur.int32() for _ in range(cur.count())]
                if any(not 0 <= d < len(names) for d in dimids):
                    raise ValueError(f'{path}: variable {name} names a dimension that does not exist')
                attrs = cur.attributes()
                nc_type = cur.int32()
                if nc_type not in NC_TYPES:
                    raise ValueError(f'{path}: variable {name} has netCDF type {nc_type}')
                cur.int32()                                                 # vsize: redundant with the shape
                begin = cur.int64() if wide else cur.int32()
                self.variables[name] = dict(dtype=np.dtype(NC_TYPES[nc_type]), shape=tuple(lengths[d] for d in dimids),
                                            dims=tuple(names[d] for d in dimids), begin=begin, attrs=attrs,
                                            record=bool(dimids) and lengths[dimids[0]] == 0)
        self.size = os.path.getsize(path)

    def var(self, name):
        if name not in self.variables:
            raise ValueError(f'{self.path}: holds no variable {name!r} (has {sorted(self.variables)})')
        v = self.variables[name]
        if v['record']:
            raise ValueError(f'{self.path}: {name} is a record variable; only fixed-size variables are read')
        nbytes = int(np.prod(v['shape'], dtype=np.int64)) * v['dtype'].itemsize
        if v['begin'] < 0 or v['begin'] + nbytes > self.size:
            raise ValueError(f'{self.path}: {name} ({nbytes} bytes at {v["begin"]}) lies outside the file of {self.size} bytes')
        return np.memmap(self.path, v['dtype'], 'r', offset=v['begin'], shape=v['shape'])

    def close(self):
        """Nothing is held open: the header was read in the constructor and every memory map owns its own mapping."""


class _Hdf5File:
    """The same two calls on a netCDF-4 file through h5py; the datasets are sliced lazily like the memory maps."""

    def __init__(self, path):
        import h5py
        self.path, self._f = path, h5py.File(path, 'r')

    def var(self, name):
        if name not in self._f:
            raise ValueError(f'{self.path}: holds no variable {name!r}')
        return self._f[name]

    def close(self):
        self._f.close()


def open_model_file(path):
    with open(path, 'rb') as fh:
        magic = fh.read(8)
    if magic == HDF5_MAGIC:
        if not h5py_enabled:
            raise ImportError('reading netCDF needs xarray + h5netcdf, or h5py; convert the cube to .npz in this environment')
        return _Hdf5File(path)
    return ClassicFile(path)


def uniform_axis(values, path, name):
    """(first, spacing) of an axis that rises uniformly (to 1e-9 of the spacing); ``ValueError`` naming the file otherwise."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 1 or values.size < 2:
        raise ValueError(f'{path}: axis {name} needs at least two nodes')
    step = (values[-1] - values[0]) / (values.size - 1)
    if not step > 0 or np.abs(values - (values[0] + step * np.arange(values.size))).max() > UNIFORM * step:
        raise ValueError(f'{path}: axis {name} does not rise uniformly')
    return float(values[0]), float(step)


@dataclass
class Subset:
    """The part of a model around a set of points: ``hre`` / ``him`` int32 [nc][nxs][nys] (mm), ``wet`` uint8 [nxs][nys], node (i, j) at
    (lon0 + i dlon, lat0 + j dlat), ``lon`` the points' longitudes unwrapped onto that axis, ``constituents`` the names of the planes."""
    hre: np.ndarray
    him: np.ndarray
    wet: np.ndarray
    lon0: float
    dlon: float
    lat0: float
    dlat: float
    lon: np.ndarray
    constituents: tuple

    @property
    def grid(self):
        return np.array([self.lon0, self.dlon, self.lat0, self.dlat], np.float64)

    @property
    def ids(self):
        return np.array([CONSTITUENTS.index(c) for c in self.constituents], np.int32)


def _one_file(model_dir, pattern, required=True):
    found = sorted(glob.glob(os.path.join(model_dir, pattern)))
    if not found:
        if required:
            raise FileNotFoundError(f'no file {pattern} in the model directory {model_dir}')
        return None
    return found[0]


def _rows(var, first, count, nx, j0, j1):
    """Rows first ... first + count - 1 modulo nx of a [nx][ny] variable, columns j0 ... j1 - 1: at most two contiguous blocks."""
    first %= nx
    if first + count <= nx:
        return np.asarray(var[first:first + count, j0:j1])
    return np.concatenate([np.asarray(var[first:, j0:j1]), np.asarray(var[:first + count - nx, j0:j1])], axis=0)


def load_subset(model_dir, constituents, lon, lat):
    """The model's constants on the bounding box of the points (``lon``, ``lat`` in degrees), grown by one node on each side.

    Longitudes are brought to [0, 360); the box is the shortest arc that holds them all, so a profile across the 0 / 360 degree seam gives one
    monotone longitude axis that runs past 360 (or starts below the first node), and the points' longitudes are unwrapped onto it
    (``lon0 + ((lon - lon0) mod 360)``).  The latitude range is clamped to the grid; there is no wrap over a pole."""
    constituents = tuple(str(c).lower() for c in constituents)
    for c in constituents:
        if c not in CONSTITUENTS:
            raise ValueError(f'constituent {c!r} is not one of {CONSTITUENTS}')
    if not constituents:
        raise ValueError('no constituent given')
    lon, lat = np.asarray(lon, dtype=np.float64).ravel(), np.asarray(lat, dtype=np.float64).ravel()
    if lon.size == 0 or lon.shape != lat.shape:
        raise ValueError(f'{lon.size} longitudes and {lat.size} latitudes')
    if not (np.isfinite(lon).all() and np.isfinite(lat).all()):
        raise ValueError('non-finite coordinates')
    paths = [_one_file(model_dir, f'h_{c}_*.nc') for c in constituents]
    grid_path = _one_file(model_dir, 'grid_*.nc', required=False)

    opened = []                                                              # closed below: the subset holds copies

    def opening(path):
        opened.append(open_model_file(path))
        return opened[-1]

    try:
        first = opening(paths[0])
        lon_z, lat_z = np.asarray(first.var('lon_z'), dtype=np.float64), np.asarray(first.var('lat_z'), dtype=np.float64)
        nx, ny = lon_z.size, lat_z.size
        x0, dlon = uniform_axis(lon_z, paths[0], 'lon_z')
        y0, dlat = uniform_axis(lat_z, paths[0], 'lat_z')
        if abs(nx * dlon - 360.0) > UNIFORM * dlon * nx:
            raise ValueError(f'{paths[0]}: the longitudes do not cover the circle ({nx} nodes of {dlon} degrees)')
        if lat.min() < y0 or lat.max() > y0 + (ny - 1) * dlat:
            raise ValueError(f'latitudes {lat.min()} ... {lat.max()} outside the grid {y0} ... {y0 + (ny - 1) * dlat}')

        # the shortest arc that holds every longitude: it starts behind the widest gap between neighbours on the circle
        lon = np.mod(lon, 360.0)
        lon[lon >= 360.0] = 0.0                                              # -1e-17 mod 360 rounds to 360
        ordered = np.sort(lon)
        gaps = np.diff(np.r_[ordered, ordered[0] + 360.0])
        k = int(np.argmax(gaps))
        west, width = float(ordered[(k + 1) % ordered.size]), 360.0 - float(gaps[k])
        if width > 180.0:
            raise ValueError(f'the points span {width:.3f} degrees of longitude; a profile spans less than 180')
        ia = int(np.floor((west - x0) / dlon)) - 1                            # one node west of the first cell
        ib = int(np.floor((west + width - x0) / dlon)) + 2                    # one node east of the last cell
        ja = max(int(np.floor((lat.min() - y0) / dlat)) - 1, 0)
        jb = min(int(np.floor((lat.max() - y0) / dlat)) + 2, ny - 1)
        if jb - ja < 1:
            ja, jb = (ja - 1, jb) if ja > 0 else (ja, jb + 1)
        nxs, nys = ib - ia + 1, jb - ja + 1
        if nxs > nx or nys < 2 or ny < 2:
            raise ValueError(f'{paths[0]}: a grid of {nx} x {ny} nodes is too small for the points')
        lon0, lat0 = x0 + ia * dlon, y0 + ja * dlat

        hre, him = np.empty((len(paths), nxs, nys), np.int32), np.empty((len(paths), nxs, nys), np.int32)
        for c, path in enumerate(paths):
            f = first if c == 0 else opening(path)
            for name, dst in (('hRe', hre), ('hIm', him)):
                var = f.var(name)
                if tuple(var.shape) != (nx, ny):
                    raise ValueError(f'{path}: {name} has shape {tuple(var.shape)}, the axes of {paths[0]} have ({nx}, {ny})')
                dst[c] = _rows(var, ia, nxs, nx, ja, jb + 1)
        if grid_path is None:
            wet = np.ones((nxs, nys), np.uint8)
        else:
            hz = opening(grid_path).var('hz')
            if tuple(hz.shape) != (nx, ny):
                raise ValueError(f'{grid_path}: hz has shape {tuple(hz.shape)}, the elevation files have ({nx}, {ny})')
            wet = (_rows(hz, ia, nxs, nx, ja, jb + 1) > 0).astype(np.uint8)
        return Subset(hre, him, wet, lon0, dlon, lat0, dlat, lon0 + np.mod(lon - lon0, 360.0), constituents)
    finally:
        for f in opened:
            f.close()
