"""Fixtures of step 6 (tests/golden/tide.npz).

    python tests/golden/make_golden_tide.py /path/to/reference

Recorded:
  * ``comp/...``: the reference's own ``compensate_tide`` on sections of ns in {1, 7, 300} samples x ntr in {1, 5, 70} traces whose sample (t, x)
    holds 1 + t + 1000 x, for ``tide_units`` meter / s / ms / samples and ``units`` s / ms, with offsets that include 0, +-1, +-(ns - 1) and +-ns;
  * ``conv/...``: values of the reference's ``depth2twt``, ``depth2samples`` and ``twt2samples``;
  * ``cli_flags`` / ``cli_description``: the reference's parser;
  * ``pred/...``: the tide prediction of DESIGN.md 3.13 evaluated with mpmath at 50 digits on the synthetic model of tests/helpers/tide_numpy.py
    (72 x 37 nodes, 14 constituents): about 300 points with times from 1985 to 2035 -- on nodes, on the last row (90 N), across the 0 / 360 degree
    seam and in cells with 1, 2, 3 and 4 dry corners -- as the [n][14] terms of the constituents (their sum over any selection is the tide).  The
    prediction does NOT come from the reference, which takes it from tpxo-tide-prediction; the mpmath statement below is written on its own and
    the float64 helper must agree with it to 1e-8 m;
  * ``cli/...``: a profile of 40 traces across the seam in thousandths of arc-seconds (CoordinateUnits 2) with recording times, the last four at
    the positions of traces 5 ... 8 at later times; the exact tides under the rule that traces sharing a position get the tide at the time of the
    first, and the rounded sample offsets for a sample interval of 50 microseconds.  The script ASSERTS that no exact offset lies within 1e-4 samples
    of a rounding tie (the cap on excluded traces is zero) and takes the first seed for which that holds.

The reference's module imports segyio, pyproj, tqdm (and its utils dask / xarray) and leaves with ``sys.exit`` when tpxo_tide_prediction is
missing; stand-ins go into ``sys.modules`` first (the one for tpxo_tide_prediction with a ``__spec__``, which ``find_spec`` asks for)."""
import importlib.machinery
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
for name in ('segyio', 'pyproj', 'tqdm', 'dask', 'dask.array', 'xarray', 'tpxo_tide_prediction'):
    mod = types.ModuleType(name)
    mod.tqdm = lambda it, **kw: it
    mod.tide_predict = None
    mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
    sys.modules[name] = mod

import tide_numpy as H  # noqa: E402
from pseudo_3D_interpolation import tide_compensation_segy as ref_cli  # noqa: E402
from pseudo_3D_interpolation.functions import utils as ref_utils  # noqa: E402

out = {}

# ---- (a) the reference's compensate_tide --------------------------------------------------------------------------------------------
rng = np.random.default_rng(11)
cases = []
for ns in (1, 7, 300):
    for ntr in (1, 5, 70):
        data = (1 + np.arange(ns)[:, None] + 1000 * np.arange(ntr)[None, :]).astype(np.float32)
        special = [0, 1, -1, ns - 1, -(ns - 1), ns, -ns]
        for tide_units in ('meter', 's', 'ms', 'samples'):
            for units in ('s', 'ms'):
                k = len(cases)
                want = np.array(([special[k % 7]] if ntr == 1 else special[:ntr] if ntr == 5 else special + list(rng.integers(-ns, ns + 1, ntr - 7))),
                                dtype=np.int64)
                want = np.roll(want, k)
                dt = 0.05 if units == 'ms' else 5e-5                      # 50 microseconds
                if tide_units == 'meter':
                    tide = want * 5e-5 * 750.0
                elif tide_units == 'samples':
                    tide = want.astype(np.float64)
                else:
                    tide = want * 5e-5                                       # 's' and 'ms' are both taken as seconds by the reference
                got = ref_cli.compensate_tide(data, tide, dt, tide_units=tide_units, units=units, verbosity=0)
                offset = np.around(tide / 5e-5 / (750.0 if tide_units == 'meter' else 1.0) if tide_units != 'samples' else tide).astype(np.int64)
                assert np.array_equal(offset, want), (ns, ntr, tide_units, units)
                assert got.shape == data.shape and got.dtype == np.float32 and np.array_equal(got, H.shift_section(data, want))
                out[f'comp/{k}/tide'], out[f'comp/{k}/out'] = tide, got
                cases.append(dict(ns=ns, ntr=ntr, tide_units=tide_units, units=units, dt=dt))
seen = {(c['ns'], c['ntr']) for c in cases}
assert len(cases) == 72 and len(seen) == 9
out['comp/cases'] = np.array(json.dumps(cases))

# ---- (b) the reference's conversions ------------------------------------------------------------------------------------------------
depth = np.r_[0.0, -1.5, 0.8317, rng.uniform(-3, 3, 13)]
out['conv/depth'] = depth
out['conv/depth2twt'] = ref_utils.depth2twt(depth)
out['conv/depth2twt_v1480'] = ref_utils.depth2twt(depth, v=1480)
for units, dt in (('s', 5e-5), ('ms', 0.05), ('ns', 5e-11)):
    out[f'conv/depth2samples/{units}'] = ref_utils.depth2samples(depth, dt, units=units)
    out[f'conv/depth2samples_v1480/{units}'] = ref_utils.depth2samples(depth, dt, v=1480, units=units)
    out[f'conv/twt2samples/{units}'] = ref_utils.twt2samples(depth / 700, dt, units=units)
    out[f'conv/dt/{units}'] = np.array(dt)

# ---- (c) the reference's flags ------------------------------------------------------------------------------------------------------
flags = []
for action in ref_cli.define_input_args()._actions:
    if action.dest != 'help':
        flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default, required=action.required,
                          choices=None if action.choices is None else list(action.choices), nargs=action.nargs, const=action.const,
                          type=None if action.type is None else action.type.__name__, help=action.help))
out['cli_flags'] = np.array(json.dumps(flags))
out['cli_description'] = np.array(ref_cli.define_input_args().description)

# ---- (d) the prediction at 50 digits -------------------------------------------------------------------------------------------------
mp.mp.dps = 50
NX, NY = 72, 37
lon_z, lat_z, fields, hz = H.model_fields(NX, NY)
DLON, DLAT = mp.mpf(360) / NX, mp.mpf(180) / (NY - 1)
RAD = mp.pi / 180
# (omega, phi0, which (t1, t2) pair or closed form)
TABLE = {'m2': ('1.405189e-4', '1.731557546'), 's2': ('1.454441e-4', '0'), 'n2': ('1.378797e-4', '6.050721243'), 'k2': ('1.458423e-4', '3.487600001'),
         'k1': ('7.292117e-5', '0.173003674'), 'o1': ('6.759774e-5', '1.558553872'), 'p1': ('7.252295e-5', '6.110181633'),
         'q1': ('6.495854e-5', '5.877717569'), 'm4': ('2.810377e-4', '3.463115091'), 'mf': ('0.053234e-4', '1.756042456'),
         '2n2': ('1.352405e-4', '4.086699633'), 'mm': ('0.026392e-4', '1.964021610'), 'mn4': ('2.783984e-4', '1.499093481'),
         'ms4': ('2.859630e-4', '1.731557546')}


def m(text):
    """The float64 the code holds for a decimal constant, as mpf: the oracle gets the parameters of the code."""
    return mp.mpf(float(text))


def exact_nodal(name, t):
    T = t / 86400 + 48622 - m('51544.4993')
    N = (m('125.0445') - m('0.05295377') * T) * RAD                          # sin and cos have period 360 degrees: the mod changes nothing
    S = [None] + [mp.sin(k * N) for k in (1, 2, 3)]
    C = [None] + [mp.cos(k * N) for k in (1, 2, 3)]

    def pair(a1, a2, b1, b2):
        t1, t2 = 1 + m(a1) * C[1] + m(a2) * C[2], m(b1) * S[1] + m(b2) * S[2]
        return mp.sqrt(t1 * t1 + t2 * t2), mp.atan(-t2 / t1)

    m2 = pair('-0.03731', '0.00052', '0.03731', '-0.00052')
    return {'mm': (1 - m('0.130') * C[1], mp.mpf(0)),
            'mf': (m('1.043') + m('0.414') * C[1], (m('-23.7') * S[1] + m('2.7') * S[2] - m('0.4') * S[3]) * RAD),
            'q1': (mp.sqrt((1 + m('0.188') * C[1]) ** 2 + (m('0.188') * S[1]) ** 2), mp.atan(m('0.189') * S[1] / (1 + m('0.189') * C[1]))),
            'o1': (mp.sqrt((1 + m('0.189') * C[1] - m('0.0058') * C[2]) ** 2 + (m('0.189') * S[1] - m('0.0058') * S[2]) ** 2),
                   (m('10.8') * S[1] - m('1.3') * S[2] + m('0.2') * S[3]) * RAD),
            'p1': (mp.mpf(1), mp.mpf(0)), 's2': (mp.mpf(1), mp.mpf(0)),
            'k1': pair('0.1158', '-0.0029', '0.1554', '-0.0029'),
            'm2': m2, 'n2': m2, '2n2': m2, 'ms4': m2,
            'k2': pair('0.2852', '0.0324', '0.3108', '0.0324'),
            'm4': (m2[0] ** 2, 2 * m2[1]), 'mn4': (m2[0] ** 2, 2 * m2[1])}[name]


def exact_terms(lon, lat, t):
    """The 14 terms of one point (mpf), or None where no wet node carries weight; also the number of dry corners of the cell."""
    lon, lat, t = mp.mpf(float(lon)), mp.mpf(float(lat)), mp.mpf(float(t))
    fx, fy = (lon - mp.floor(lon / 360) * 360) / DLON - 1, (lat + 90) / DLAT       # node i is at (i + 1) dlon
    ix, iy = int(mp.floor(fx)), min(int(mp.floor(fy)), NY - 2)
    wx, wy = fx - ix, fy - iy
    corners = [(ix % NX, iy, (1 - wx) * (1 - wy)), (ix % NX, iy + 1, (1 - wx) * wy), ((ix + 1) % NX, iy, wx * (1 - wy)), ((ix + 1) % NX, iy + 1, wx * wy)]
    ndry = sum(1 for i, j, _ in corners if not hz[i, j] > 0)
    kept = [(i, j, w) for i, j, w in corners if hz[i, j] > 0]
    total = sum(w for _, _, w in kept)
    if not kept or total == 0:
        return None, ndry
    terms = []
    for name in H.CONSTITUENTS:
        re, im = fields[name]
        zr = sum(w * int(re[i, j]) for i, j, w in kept) / total / 1000
        zi = sum(w * int(im[i, j]) for i, j, w in kept) / total / 1000
        f, u = exact_nodal(name, t)
        theta = m(TABLE[name][0]) * t + m(TABLE[name][1]) + u
        terms.append(f * (zr * mp.cos(theta) - zi * mp.sin(theta)))
    return terms, ndry


T0, T1 = -220838400.0, 1356998400.0                                              # 1985-01-01 ... 2035-01-01 in seconds since 1992-01-01
rng = np.random.default_rng(3)
lon, lat = [], []
nodes_i, nodes_j = rng.integers(68, 78, 40), rng.integers(30, 37, 40)            # on nodes (some of them dry)
lon += list((5.0 * (nodes_i + 1)) % 360)
lat += list(-90.0 + 5.0 * nodes_j)
lon += list(rng.uniform(340, 380, 20) % 360)                                     # on the last row
lat += [90.0] * 20
seam = rng.uniform(-5, 5, 40)                                                    # across the seam, given below 0, above 360 and inside
lon += list(np.where(np.arange(40) % 3 == 0, seam, np.where(np.arange(40) % 3 == 1, seam + 360, seam % 360)))
lat += list(rng.uniform(60, 90, 40))
lon += list(rng.uniform(0, 25, 120))                                             # around the dry patch (nodes at 5 ... 20 E, 65 ... 75 N)
lat += list(rng.uniform(60, 80, 120))
lon += list(rng.uniform(340, 380, 80) % 360)
lat += list(rng.uniform(60, 90, 80))
lon, lat = np.array(lon, dtype=np.float64), np.array(lat, dtype=np.float64)
t = np.rint(rng.uniform(T0, T1, lon.size))
t[::7] += rng.uniform(0, 1, t[::7].size)                                         # some with a fraction of a second
t[:4] = [T0, T1, 0.0, -1.0]
terms = np.full((lon.size, 14), np.nan)
ndry = np.zeros(lon.size, np.int64)
for k in range(lon.size):
    got, ndry[k] = exact_terms(lon[k], lat[k], t[k])
    if got is not None:
        terms[k] = [float(v) for v in got]
assert all((ndry[80:] == d).sum() >= 5 for d in (0, 1, 2, 3, 4)), np.bincount(ndry[80:])
assert np.isnan(terms[:, 0]).sum() >= 5 and np.abs(np.nansum(terms, axis=1)).max() < 10
assert (lon[60:100] < 0).any() and (lon[60:100] > 360).any() and (lat == 90).sum() >= 20
re_all, im_all = np.array([fields[c][0] for c in H.CONSTITUENTS]), np.array([fields[c][1] for c in H.CONSTITUENTS])
helper = H.predict(np.mod(lon, 360), lat, t, re_all, im_all, hz > 0, 5.0, 5.0, -90.0, 5.0, H.CONSTITUENTS, periodic=True, parts=True)
assert np.array_equal(np.isnan(helper), np.isnan(terms))
worst = float(np.nanmax(np.abs(helper.sum(axis=1) - terms.sum(axis=1))))
print(f'float64 helper against mpmath: {worst:.2e} m over {lon.size} points, dry corners {np.bincount(ndry).tolist()}')
assert worst < 1e-8
out['pred/lon'], out['pred/lat'], out['pred/t'], out['pred/terms'], out['pred/ndry'] = lon, lat, t, terms, ndry
out['pred/constituents'] = np.array(H.CONSTITUENTS)

# ---- (e) a profile for the command line ------------------------------------------------------------------------------------------------
NTR, DT_S, DEFAULT = 40, 5e-5, H.CONSTITUENTS[:8]


def profile(seed):
    r = np.random.default_rng(seed)
    lon_mas = np.rint(-0.1 * 3600000 + np.cumsum(r.normal(18000, 2000, NTR))).astype(np.int64)      # thousandths of arc-seconds, 0.1 W ... 0.1 E
    lat_mas = np.rint(62.0 * 3600000 + np.cumsum(r.normal(5000, 2000, NTR))).astype(np.int64)
    lon_mas[36:], lat_mas[36:] = lon_mas[5:9], lat_mas[5:9]
    start = r.integers(0, 86400 * 300)
    sec = start + np.cumsum(r.integers(1, 4000, NTR))                            # seconds of 2024 (a leap year), some hours apart
    return lon_mas, lat_mas, sec


for seed in range(1000):
    lon_mas, lat_mas, sec = profile(seed)
    times = np.datetime64('2024-01-01T00:00:00', 's') + sec.astype('timedelta64[s]')
    first = np.arange(NTR)
    first[36:] = np.arange(5, 9)                                                 # the trace whose time counts
    tsec = (times[first] - np.datetime64('1992-01-01T00:00:00', 's')).astype(np.int64).astype(np.float64)
    exact = []
    for k in range(NTR):
        got, _ = exact_terms(lon_mas[k] / 3600000, lat_mas[k] / 3600000, tsec[k])
        exact.append(sum(got[:8]))
    samples = [v / 750 / mp.mpf(DT_S) for v in exact]
    margin = min(abs(abs(s - mp.floor(s)) - mp.mpf('0.5')) for s in samples)
    if margin > 1e-4:                                                            # the cap on excluded traces is zero: every trace is kept
        break
else:
    raise AssertionError('no seed without a near tie')
assert margin > 1e-4 and len({int(mp.nint(s)) for s in samples}) > 5
days = (times - np.datetime64('2024-01-01', 's')).astype('timedelta64[D]')
rest = (times - np.datetime64('2024-01-01', 's') - days).astype(np.int64)
out['cli/seed'], out['cli/lon_mas'], out['cli/lat_mas'] = np.array(seed), lon_mas, lat_mas
out['cli/year'], out['cli/day'] = np.full(NTR, 2024), days.astype(np.int64) + 1
out['cli/hour'], out['cli/minute'], out['cli/second'] = rest // 3600, rest // 60 % 60, rest % 60
out['cli/time_used'] = np.datetime_as_string(times[first], 's')
out['cli/tide'] = np.array([float(v) for v in exact])
out['cli/offset'] = np.array([int(mp.nint(s)) for s in samples], np.int64)
out['cli/dt_us'] = np.array(50)
print(f'profile: seed {seed}, nearest rounding tie {float(margin):.2e} samples away, offsets {out["cli/offset"].min()} ... {out["cli/offset"].max()}')

path = os.path.join(HERE, 'tide.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
