"""Fixtures of step 2 (tests/golden/reproject.npz).

    python tests/golden/make_golden_reproject.py /path/to/reference

The projection values do NOT come from the reference (it takes them from pyproj) and not from the series under test: they are the exact
Gauss-Krueger projection evaluated with mpmath at 50 digits,

    N + i E = k0 * integral_0^Phi M(phi) dphi  along the straight path,   M(phi) = a (1 - e^2) / (1 - e^2 sin^2 phi)^(3/2),

where the complex latitude Phi solves psi(Phi) = psi(lat) + i lam by Newton's iteration (start: the sphere's solution asin(tanh(.))) and
psi(phi) = atanh(sin phi) - e atanh(e sin phi) is the isometric latitude; a latitude of origin is the same integral up to lat0 subtracted.

Recorded:
  * ``proj/<setting>/...``: 9 latitudes x 7 offsets from the central meridian, lon / lat / E / N as float64, for WGS84 UTM 60S (EPSG:32760), WGS84
    UTM 32N, ETRS89 UTM 32N (GRS80) and a ``+proj=tmerc`` string with lat_0 != 0, k = 1 and offsets;
  * ``z2z/...``: points of UTM 32N in UTM 33N, the oracle evaluated for both zones on the same geographic points;
  * ``hdr/...``: a profile of 300 traces in thousandths of arc-seconds (CoordinateUnits 2) and the exact header integers of EPSG:32760 for the scalars
    -1000, -100, 0 and 10, plus those after the reference's ``smooth(., 11)`` for scalar -100.  The script ASSERTS that no exact value is closer
    than 1e-6 m on the ground (1e-6 * |scalar| header units for a negative scalar) to a rounding tie, and takes the first seed for which that holds;
  * ``smooth/...``: inputs and outputs of the reference's own ``functions.filter.smooth`` (lengths 11, 12, 64, 257; windows 3, 10, 11, 51), the
    pass-through below 3 and the messages of both ``ValueError``s;
  * ``cli_flags``: the flags of the reference's parser.

The reference's modules import segyio, pyproj, tqdm (and its utils dask / xarray) at module level; empty stand-ins go into ``sys.modules`` first."""
import json
import os
import sys
import types

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, '..', 'helpers'))
for name in ('segyio', 'pyproj', 'tqdm', 'dask', 'dask.array', 'xarray'):
    mod = types.ModuleType(name)
    mod.tqdm = lambda it, **kw: it
    sys.modules[name] = mod

import reproject_numpy as H  # noqa: E402
from pseudo_3D_interpolation import reproject_segy as ref_cli  # noqa: E402
from pseudo_3D_interpolation.functions.filter import smooth as ref_smooth  # noqa: E402

mp.mp.dps = 50
WGS84 = (mp.mpf(6378137), mp.mpf(1 / 298.257223563))          # the float64 flattening the package holds: the oracle gets the parameters of the code
GRS80 = (mp.mpf(6378137), mp.mpf(1 / 298.257222101))
RAD = mp.pi / 180


def oracle(lon, lat, a, f, lon0, lat0, k0, x0, y0):
    """(E, N) as mpf of one point; lon / lat / lon0 / lat0 in degrees (mpf or exactly representable numbers)."""
    e2 = f * (2 - f)
    e = mp.sqrt(e2)

    def psi(phi):
        s = mp.sin(phi)
        return mp.atanh(s) - e * mp.atanh(e * s)

    def dpsi(phi):
        return (1 - e2) / ((1 - e2 * mp.sin(phi) ** 2) * mp.cos(phi))

    def meridian(phi):
        return a * (1 - e2) / (1 - e2 * mp.sin(phi) ** 2) ** mp.mpf('1.5')

    target = psi(mp.mpf(lat) * RAD) + 1j * (mp.mpf(lon) - mp.mpf(lon0)) * RAD
    Phi = mp.asin(mp.tanh(target))
    for _ in range(60):
        step = (psi(Phi) - target) / dpsi(Phi)
        Phi -= step
        if abs(step) < mp.mpf(10) ** -45:
            break
    else:
        raise AssertionError('Newton did not converge')
    z = mp.quad(lambda t: meridian(t * Phi) * Phi, [0, 1])
    m0 = mp.quad(meridian, [0, mp.mpf(lat0) * RAD]) if lat0 != 0 else 0
    return x0 + k0 * z.imag, y0 + k0 * (z.real - m0)


def as_prm(a, f, lon0, lat0, k0, x0, y0):
    return np.array([float(a), float(f), float(lon0), float(lat0), float(k0), float(x0), float(y0)])


out = {}
K_UTM = mp.mpf('0.9996')
SETTINGS = {
    'utm60s_wgs84': (*WGS84, 177, 0, K_UTM, 500000, 10000000),
    'utm32n_wgs84': (*WGS84, 9, 0, K_UTM, 500000, 0),
    'utm32n_grs80': (*GRS80, 9, 0, K_UTM, 500000, 0),
    'tmerc_lat0': (*WGS84, mp.mpf('173'), mp.mpf('-41.5'), mp.mpf(1), 1600000, 250000.5),
}
out['proj/strings'] = np.array(json.dumps({
    'utm60s_wgs84': 'EPSG:32760', 'utm32n_wgs84': 'EPSG:32632', 'utm32n_grs80': 'EPSG:25832',
    'tmerc_lat0': '+proj=tmerc +lat_0=-41.5 +lon_0=173 +k=1 +x_0=1600000 +y_0=250000.5 +ellps=WGS84 +units=m +no_defs'}))
LATS = ['-80', '-45.3', '-36.8', '-0.5', '0', '12.25', '52', '71', '84']
DLAMS = ['-6', '-3.2', '-1', '0', '0.5', '3', '4']
worst = 0.0
for name, s in SETTINGS.items():
    lon = [mp.mpf(s[2]) + mp.mpf(d) for d in DLAMS for _ in LATS]
    lat = [mp.mpf(v) for _ in DLAMS for v in LATS]
    lon64, lat64 = np.array([float(v) for v in lon]), np.array([float(v) for v in lat])
    # the oracle is evaluated at the float64 inputs the tests hand to the code, not at the decimal strings
    en = [oracle(mp.mpf(float(lo)), mp.mpf(float(la)), *s) for lo, la in zip(lon64, lat64)]
    E, N = np.array([float(v[0]) for v in en]), np.array([float(v[1]) for v in en])
    prm = as_prm(*s)
    gE, gN = H.tm_forward(lon64, lat64, prm)
    worst = max(worst, np.abs(gE - E).max(), np.abs(gN - N).max())
    for key, val in (('prm', prm), ('lon', lon64), ('lat', lat64), ('E', E), ('N', N)):
        out[f'proj/{name}/{key}'] = val
    assert lon64.size == 63 and np.any(lon64 == float(s[2])) and np.any(lat64 == 0)
out['proj/settings'] = np.array(list(SETTINGS))
print(f'float64 series against the oracle, forward: {worst:.2e} m')
assert worst < 1e-7

# ---- zone to zone: 32N -> 33N ---------------------------------------------------------------------------------------------------
s32, s33 = SETTINGS['utm32n_wgs84'], (*WGS84, 15, 0, K_UTM, 500000, 0)
zlon = np.array([float(lo) for lo in ('9.5', '11', '12', '13', '14.2') for _ in LATS])
zlat = np.array([float(la) for _ in range(5) for la in LATS])
src = [oracle(mp.mpf(lo), mp.mpf(la), *s32) for lo, la in zip(zlon, zlat)]
dst = [oracle(mp.mpf(lo), mp.mpf(la), *s33) for lo, la in zip(zlon, zlat)]
out['z2z/prm_src'], out['z2z/prm_dst'] = as_prm(*s32), as_prm(*s33)
out['z2z/E_src'], out['z2z/N_src'] = (np.array([float(v[k]) for v in src]) for k in (0, 1))
out['z2z/E_dst'], out['z2z/N_dst'] = (np.array([float(v[k]) for v in dst]) for k in (0, 1))

# ---- header integers of an arc-second profile --------------------------------------------------------------------------------------
NTR, SCALARS, GROUND = 300, (-1000, -100, 0, 10), 1e-6
s60 = SETTINGS['utm60s_wgs84']
prm60 = as_prm(*s60)


def multiplier(scalar):
    return mp.mpf(abs(scalar)) if scalar < 0 else (1 / mp.mpf(scalar) if scalar > 0 else mp.mpf(1))


def tie_distance(values, scalar):
    """Smallest distance, in header units, of the exact scaled values to a value halfway between two integers."""
    m = multiplier(scalar)
    return min(abs(abs(v * m - mp.floor(v * m)) - mp.mpf('0.5')) for v in values)


def profile(seed):
    rng = np.random.default_rng(seed)
    lon = 174.7 * 3600000 + np.cumsum(rng.normal(9000, 1500, NTR))          # thousandths of arc-seconds (about 3 cm), traces some 250 m apart
    lat = -72.5 * 3600000 + np.cumsum(rng.normal(-4000, 1500, NTR))         # far enough south for the northing in millimetres to fit 32 bits
    return np.rint(lon).astype(np.int64), np.rint(lat).astype(np.int64)


for seed in range(1000):
    lon_i, lat_i = profile(seed)
    E, N = H.tm_forward(lon_i / 3600000, lat_i / 3600000, prm60)            # screening with the float64 series (nanometres) at twice the margin, the oracle decides below
    smoothed = np.r_[ref_smooth(E, 11), ref_smooth(N, 11)]
    if all(tie_distance([mp.mpf(v) for v in np.r_[E, N]], sc) > 2 * GROUND * multiplier(sc) for sc in SCALARS) \
            and tie_distance([mp.mpf(v) for v in smoothed], -100) > 2 * GROUND * 100:
        break
else:
    raise AssertionError('no seed without a near tie')
exact = [oracle(mp.mpf(int(lo)) / 3600000, mp.mpf(int(la)) / 3600000, *s60) for lo, la in zip(lon_i, lat_i)]
exE, exN = [v[0] for v in exact], [v[1] for v in exact]
out['hdr/seed'], out['hdr/lon_mas'], out['hdr/lat_mas'], out['hdr/scalars'] = np.array(seed), lon_i, lat_i, np.array(SCALARS)
out['hdr/E'], out['hdr/N'] = np.array([float(v) for v in exE]), np.array([float(v) for v in exN])
assert np.abs(lon_i).max() < 2**31 and np.abs(lat_i).max() < 2**31
for sc in SCALARS:
    m = multiplier(sc)
    margin = tie_distance(exE + exN, sc)
    assert margin > GROUND * m, (sc, margin)                                  # the cap on excluded points is zero: every trace is kept
    out[f'hdr/{sc}/x'] = np.array([int(mp.nint(v * m)) for v in exE], np.int64)
    out[f'hdr/{sc}/y'] = np.array([int(mp.nint(v * m)) for v in exN], np.int64)
    assert np.abs(out[f'hdr/{sc}/x']).max() < 2**31 and np.abs(out[f'hdr/{sc}/y']).max() < 2**31
    print(f'scalar {sc}: nearest rounding tie {float(margin / m):.2e} m away')
sm = [ref_smooth(out[f'hdr/{k}'], 11) for k in ('E', 'N')]
assert min(np.abs(np.abs(v * 100 - np.floor(v * 100)) - 0.5).min() for v in sm) > 1e-4      # 1e-6 m * 100
out['hdr/smooth11/x'], out['hdr/smooth11/y'] = (np.around(v * 100).astype(np.int64) for v in sm)

# ---- smooth: the reference's own function --------------------------------------------------------------------------------------------
rng = np.random.default_rng(2)
cases, errors = [], {}
for length in (11, 12, 64, 257):
    base = rng.uniform(1e5, 1e7) + np.arange(length) * rng.uniform(-40, 40) + np.cumsum(rng.normal(0, 3, length))
    out[f'smooth/in/{length}'] = base
    for wl in (3, 10, 11, 51):
        try:
            got = ref_smooth(base, wl)
        except ValueError as exc:
            errors[f'{length}/{wl}'] = str(exc)
            continue
        assert got.shape == base.shape
        out[f'smooth/out/{length}/{wl}'] = got
        cases.append([length, wl])
    assert ref_smooth(base, 2) is base
assert [64, 51] in cases and [11, 11] in cases and [12, 11] in cases and [11, 10] in cases and errors
try:
    ref_smooth(np.zeros((4, 4)), 3)
except ValueError as exc:
    errors['ndim'] = str(exc)
try:
    ref_smooth(np.arange(20.0), 5, window='kaiser')
except ValueError as exc:
    errors['window'] = str(exc)
for window in ('flat', 'hamming', 'bartlett', 'blackman'):
    out[f'smooth/window/{window}'] = ref_smooth(out['smooth/in/64'], 7, window=window)
out['smooth/cases'], out['smooth/errors'] = np.array(cases), np.array(json.dumps(errors))

# ---- the reference's flags ---------------------------------------------------------------------------------------------------------
flags = []
for action in ref_cli.define_input_args()._actions:
    if action.dest != 'help':
        flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default, required=action.required,
                          choices=None if action.choices is None else list(action.choices), nargs=action.nargs, const=action.const,
                          type=None if action.type is None else action.type.__name__, help=action.help))
out['cli_flags'] = np.array(json.dumps(flags))
out['cli_description'] = np.array(ref_cli.define_input_args().description)

path = os.path.join(HERE, 'reproject.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
