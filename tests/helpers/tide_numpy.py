"""Float64 NumPy statement of the step-6 tide prediction (include/p3d.h), written from the formulas and vectorised over the points; a
minimal writer of netCDF classic files; and a synthetic TPXO9-atlas style model for the tests.

The prediction works on the tables the kernel gets (a subset, ``periodic=False``) or on a whole model whose longitudes cover the circle
(``periodic=True``: node indices are taken modulo ``nx``), so it does not depend on ``functions/tide_model.load_subset``."""
import os
import struct

import numpy as np

CONSTITUENTS = ('m2', 's2', 'n2', 'k2', 'k1', 'o1', 'p1', 'q1', 'm4', 'mf', '2n2', 'mm', 'mn4', 'ms4')
OMEGA = {'m2': 1.405189e-4, 's2': 1.454441e-4, 'n2': 1.378797e-4, 'k2': 1.458423e-4, 'k1': 7.292117e-5, 'o1': 6.759774e-5, 'p1': 7.252295e-5,
         'q1': 6.495854e-5, 'm4': 2.810377e-4, 'mf': 0.053234e-4, '2n2': 1.352405e-4, 'mm': 0.026392e-4, 'mn4': 2.783984e-4, 'ms4': 2.859630e-4}
PHASE = {'m2': 1.731557546, 's2': 0.0, 'n2': 6.050721243, 'k2': 3.487600001, 'k1': 0.173003674, 'o1': 1.558553872, 'p1': 6.110181633,
         'q1': 5.877717569, 'm4': 3.463115091, 'mf': 1.756042456, '2n2': 4.086699633, 'mm': 1.964021610, 'mn4': 1.499093481, 'ms4': 1.731557546}


def nodal(name, t):
    """(f, u) of constituent ``name`` at ``t`` seconds since 1992-01-01 (OTPS ``nodal``)."""
    atan, rad = np.arctan, np.pi / 180
    T = t / 86400 + 48622 - 51544.4993
    N = (125.0445 - 0.05295377 * T) % 360 * rad
    s1, c1, s2, c2, s3 = np.sin(N), np.cos(N), np.sin(2 * N), np.cos(2 * N), np.sin(3 * N)
    if name == 'mm':
        return 1 - 0.130 * c1, 0 * c1
    if name == 'mf':
        return 1.043 + 0.414 * c1, (-23.7 * s1 + 2.7 * s2 - 0.4 * s3) * rad
    if name == 'q1':
        return np.sqrt((1 + 0.188 * c1) ** 2 + (0.188 * s1) ** 2), atan(0.189 * s1 / (1 + 0.189 * c1))
    if name == 'o1':
        return np.sqrt((1 + 0.189 * c1 - 0.0058 * c2) ** 2 + (0.189 * s1 - 0.0058 * s2) ** 2), (10.8 * s1 - 1.3 * s2 + 0.2 * s3) * rad
    if name in ('p1', 's2'):
        return 1 + 0 * c1, 0 * c1
    if name == 'k1':
        t1, t2 = 1 + 0.1158 * c1 - 0.0029 * c2, 0.1554 * s1 - 0.0029 * s2
    elif name in ('m2', 'n2', '2n2', 'ms4', 'm4', 'mn4'):
        t1, t2 = 1 - 0.03731 * c1 + 0.00052 * c2, 0.03731 * s1 - 0.00052 * s2
    elif name == 'k2':
        t1, t2 = 1 + 0.2852 * c1 + 0.0324 * c2, 0.3108 * s1 + 0.0324 * s2
    else:
        raise ValueError(name)
    f, u = np.sqrt(t1 ** 2 + t2 ** 2), atan(-t2 / t1)
    if name in ('m4', 'mn4'):
        return f ** 2, 2 * u
    return f, u


def cell_weights(lon, lat, wet, lon0, dlon, lat0, dlat, periodic=False):
    """Node indices (ix, ix + 1, iy, iy + 1) and the four renormalised weights [4][n] (order 00, 01, 10, 11; NaN where they sum to 0)."""
    nxs, nys = wet.shape
    fx, fy = (np.asarray(lon, float) - lon0) / dlon, (np.asarray(lat, float) - lat0) / dlat
    ix = np.floor(fx).astype(np.int64)
    if not periodic:
        ix = np.clip(ix, 0, nxs - 2)
    iy = np.clip(np.floor(fy).astype(np.int64), 0, nys - 2)
    wx, wy = fx - ix, fy - iy
    i0, i1 = (ix % nxs, (ix + 1) % nxs) if periodic else (ix, ix + 1)
    w = np.array([(1 - wx) * (1 - wy), (1 - wx) * wy, wx * (1 - wy), wx * wy])
    w = w * np.array([wet[i0, iy], wet[i0, iy + 1], wet[i1, iy], wet[i1, iy + 1]]).astype(bool)
    total = w.sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.where(total > 0, w / total, np.nan)
    return (i0, i1, iy, iy + 1), w


def predict(lon, lat, t, hre, him, wet, lon0, dlon, lat0, dlat, names, periodic=False, parts=False):
    """Tide (m) at the points; ``hre`` / ``him`` [nc][nxs][nys] in mm, ``names`` the constituent of each plane.  ``parts``: the [n][nc] terms."""
    t = np.asarray(t, float)
    (i0, i1, j0, j1), w = cell_weights(lon, lat, wet, lon0, dlon, lat0, dlat, periodic)
    terms = np.empty((t.size, len(names)))
    for c, name in enumerate(names):
        zr = (w[0] * hre[c][i0, j0] + w[1] * hre[c][i0, j1] + w[2] * hre[c][i1, j0] + w[3] * hre[c][i1, j1]) / 1000
        zi = (w[0] * him[c][i0, j0] + w[1] * him[c][i0, j1] + w[2] * him[c][i1, j0] + w[3] * him[c][i1, j1]) / 1000
        f, u = nodal(name, t)
        theta = OMEGA[name] * t + PHASE[name] + u
        terms[:, c] = f * (zr * np.cos(theta) - zi * np.sin(theta))
    return terms if parts else terms.sum(axis=1)


def shift_section(data, offset):
    """out[t][x] = data[t + offset[x]][x] or 0 on a (samples x traces) section: the compensation by integer offsets."""
    data = np.asarray(data)
    out = np.zeros_like(data)
    ns = data.shape[0]
    for x, k in enumerate(np.asarray(offset, dtype=np.int64)):
        if abs(k) < ns:
            out[max(-k, 0):ns - max(k, 0), x] = data[max(k, 0):ns - max(-k, 0), x]
    return out


# ---- netCDF classic writer -------------------------------------------------------------------------------------------------------
NC_TYPE = {'int8': 1, 'int16': 3, 'int32': 4, 'float32': 5, 'float64': 6}


def _name(text):
    raw = text.encode()
    return struct.pack('>i', len(raw)) + raw + b'\x00' * (-len(raw) % 4)


def write_classic(path, dims, variables, version=1, attrs=None, sparse=()):
    """Write ``variables`` [(name, (dimension names), array)] as a netCDF classic file (``version`` 1, or 2 for 64-bit offsets) with fixed-size
    dimensions ``dims`` {name: length} and global text attributes ``attrs``.  Variables named in ``sparse`` get their space but no data (a hole
    in the file); their array may be ``None``."""
    names = list(dims)
    variables = [(n, d, None if a is None else np.asarray(a)) for n, d, a in variables]

    def att_list(items):
        if not items:
            return struct.pack('>ii', 0, 0)
        out = struct.pack('>ii', 12, len(items))
        for key, text in items.items():
            raw = text.encode()
            out += _name(key) + struct.pack('>ii', 2, len(raw)) + raw + b'\x00' * (-len(raw) % 4)
        return out

    def header(begins):
        out = b'CDF' + bytes([version]) + struct.pack('>i', 0)
        out += struct.pack('>ii', 10, len(names)) + b''.join(_name(n) + struct.pack('>i', dims[n]) for n in names)
        out += att_list(attrs)
        out += struct.pack('>ii', 11, len(variables))
        for (name, vdims, arr), begin, (dtype, nbytes) in zip(variables, begins, kinds):
            out += _name(name) + struct.pack('>i', len(vdims)) + b''.join(struct.pack('>i', names.index(d)) for d in vdims)
            out += att_list(None) + struct.pack('>ii', NC_TYPE[dtype], min(nbytes + (-nbytes) % 4, 2**31 - 1))
            out += struct.pack('>q' if version == 2 else '>i', begin)
        return out

    kinds = []
    for name, vdims, arr in variables:
        dtype = 'int32' if arr is None else arr.dtype.name
        shape = tuple(dims[d] for d in vdims)
        assert arr is None or arr.shape == shape, (name, arr.shape, shape)
        kinds.append((dtype, int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize))
    start = len(header([0] * len(variables)))
    begins, pos = [], start
    for _, nbytes in kinds:
        begins.append(pos)
        pos += nbytes + (-nbytes) % 4
    with open(path, 'wb') as fh:
        fh.write(header(begins))
        for (name, _, arr), begin, (dtype, nbytes) in zip(variables, begins, kinds):
            if name not in sparse:
                fh.seek(begin)
                fh.write(arr.astype(np.dtype(dtype).newbyteorder('>')).tobytes())
        fh.truncate(pos)
    return path


# ---- a synthetic model --------------------------------------------------------------------------------------------------------------
DRY_NODES = [(i, j) for i in (0, 1, 2) for j in (31, 32, 33)] + [(3, 32)]       # a 3 x 3 block and one node beside it: cells with 1, 2, 3 and 4 dry corners


def model_fields(nx=72, ny=37, constituents=CONSTITUENTS, seed=0):
    """Axes, smooth complex constants in integer millimetres (|z| <= 1.5 m, the amplitudes of 14 constituents sum to less than 10 m) and depths."""
    rng = np.random.default_rng(seed)
    dlon, dlat = 360.0 / nx, 180.0 / (ny - 1)
    lon_z, lat_z = dlon * np.arange(1, nx + 1), -90.0 + dlat * np.arange(ny)
    lam, phi = np.radians(lon_z)[:, None], np.radians(lat_z)[None, :]
    fields = {}
    for name in CONSTITUENTS:                                                   # every constituent draws its numbers, whichever are asked for
        a, p, q, r = rng.uniform(0.2, 0.7), rng.uniform(0, 2 * np.pi, 3)[0], rng.uniform(0, 2 * np.pi), rng.integers(1, 4)
        amp = a * (0.6 + 0.4 * np.cos(2 * lam + p) * np.cos(phi))
        z = amp * np.exp(1j * (r * lam + 2 * phi + q))
        fields[name] = (np.rint(z.real * 1000).astype(np.int32), np.rint(z.imag * 1000).astype(np.int32))
    hz = 100.0 + 50.0 * np.cos(lam) * np.cos(phi)
    for i, j in DRY_NODES:
        if i < nx and j < ny:
            hz[i, j] = 0.0
    return lon_z, lat_z, {c: fields[c] for c in constituents}, hz


def make_model(folder, nx=72, ny=37, constituents=CONSTITUENTS, seed=0, version=1, grid=True):
    """Write the model of `model_fields` into ``folder`` (one ``h_<con>_synthetic.nc`` per constituent and ``grid_synthetic.nc``); returns
    (lon_z, lat_z, fields, hz)."""
    lon_z, lat_z, fields, hz = model_fields(nx, ny, constituents, seed)
    os.makedirs(folder, exist_ok=True)
    dims = {'nx': nx, 'ny': ny}
    for name, (re, im) in fields.items():
        write_classic(os.path.join(folder, f'h_{name}_synthetic.nc'), dims,
                      [('lon_z', ('nx',), lon_z), ('lat_z', ('ny',), lat_z), ('hRe', ('nx', 'ny'), re), ('hIm', ('nx', 'ny'), im)],
                      version=version, attrs={'title': f'synthetic elevation constants of {name}'})
    if grid:
        write_classic(os.path.join(folder, 'grid_synthetic.nc'), dims,
                      [('lon_z', ('nx',), lon_z), ('lat_z', ('ny',), lat_z), ('hz', ('nx', 'ny'), hz.astype(np.float32))], version=version)
    return lon_z, lat_z, fields, hz
