"""Fixtures of step 10 (tests/golden/binning.npz) from the REFERENCE's own functions.

Run with an interpreter that has numpy, pandas and dask (the reference's cube_binning_3D imports xarray, pyproj, segyio and segysak
at module level, and ``functions.utils_io`` whose file is ``utils_IO.py``; empty stand-ins for those go into ``sys.modules`` first --
none of the recorded functions uses them):

    python3.9 tests/golden/make_golden_binning.py /path/to/reference

Recorded: the forward / inverse transforms and get_cube_parameter (bins, il/xl per trace) on a rotated square grid, a rotated
rectangular grid and a region with a coarser step; pad_trace on the cases where it works; and stacked bins for the four methods,
composed the way inlines_from_seismic does it: pad every trace, then dask's mean / median over the stack, the first trace per bin
after the distance idxmin, or the stack times the per-bin normalised weights 1 / d**f summed (a bin of one trace: the trace)."""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
for name in ('xarray', 'pyproj', 'segyio', 'segysak', 'segysak.segy', 'pseudo_3D_interpolation.functions.utils_io'):
    mod = types.ModuleType(name)
    mod.open_seisnc = mod.segy_header_scrape = mod.segy_bin_scrape = None
    mod.read_auxiliary_files = mod.extract_navigation_from_segy = None
    mod.set_options = lambda **kw: None
    sys.modules[name] = mod

import dask.array as da  # noqa: E402
import pandas as pd  # noqa: E402

from pseudo_3D_interpolation import cube_binning_3D as cb  # noqa: E402
from pseudo_3D_interpolation.functions.transform import Affine  # noqa: E402

out = {}
rng = np.random.default_rng(20261016)

# ---- geometry -----------------------------------------------------------------------------------------------------------------
cases = {
    'square': dict(corners=[[1000.0, 2000.0], [1000.0, 2600.0], [1800.0, 2600.0], [1800.0, 2000.0]], angle=23.0, center=None,
                   bin_size=(10, 10), region=None, bin_size_region=None),
    'rect': dict(corners=[[500.0, 100.0], [380.0, 650.0], [1150.0, 820.0], [1270.0, 270.0]], angle=-12.5, center=(800.0, 450.0),
                 bin_size=(12.5, 7.5), region=None, bin_size_region=None),
    'region': dict(corners=[[1000.0, 2000.0], [1000.0, 2400.0], [1600.0, 2400.0], [1600.0, 2000.0]], angle=15.0, center=(1300.0, 2200.0),
                   bin_size=(10, 10), region=[[900.0, 1900.0], [900.0, 2500.0], [1700.0, 2500.0], [1700.0, 1900.0]],
                   bin_size_region=(5, 5)),
}
for key, c in cases.items():
    corners = np.asarray(c['corners'])
    center = tuple(c['center']) if c['center'] is not None else tuple(cb.get_polygon_centroid(corners))
    fwd = Affine().rotate_around(angle=-c['angle'], origin=center)
    rev = fwd.inverse()
    lo, hi = corners.min(0) - 50, corners.max(0) + 50
    xy = rng.uniform(lo, hi, size=(400, 2))
    df_nav = pd.DataFrame(xy, columns=['x', 'y'])
    bsr = c['bin_size_region'] if c['bin_size_region'] is not None else c['bin_size']
    bins, ilxl, gcube, gregion, centres = cb.get_cube_parameter(
        fwd, rev, df_nav, bin_size=c['bin_size'], cube_corner_pts=corners, bin_size_region=bsr,
        region_corner_pts=np.asarray(c['region']) if c['region'] is not None else None, return_geometry=True)
    p = f'geom/{key}/'
    out[p + 'corners'] = corners
    out[p + 'angle'] = np.float64(c['angle'])
    out[p + 'center'] = np.asarray(center, dtype=np.float64)
    out[p + 'center_given'] = np.bool_(c['center'] is not None)
    out[p + 'bin_size'] = np.asarray(c['bin_size'], dtype=np.float64)
    out[p + 'bin_size_int'] = np.bool_(all(isinstance(s, int) for s in c['bin_size']))
    out[p + 'bin_size_region'] = np.asarray(bsr, dtype=np.float64)
    if c['region'] is not None:
        out[p + 'region'] = np.asarray(c['region'])
        out[p + 'extent_region'] = gregion[0]
        out[p + 'region_centres'] = centres
    out[p + 'fwd'] = fwd.matrix
    out[p + 'rev'] = rev.matrix
    out[p + 'xy'] = xy
    out[p + 'bins'] = bins[['il', 'xl']].to_numpy().astype(np.int32)
    out[p + 'bins_xy'] = bins[['x', 'y']].to_numpy()
    out[p + 'ilxl'] = ilxl[['il', 'xl']].to_numpy().astype(np.int32)
    out[p + 'extent_cube'] = gcube[0]
    out[p + 'extent_cube_t'] = np.asarray(gcube[1], dtype=np.float64)

# ---- pad_trace ---------------------------------------------------------------------------------------------------------------
pads = []
for delrt, ns, t0, t1, dt in [(100, 40, 100.0, 120.0, 0.5), (90, 60, 100.0, 120.0, 0.5), (104, 32, 100.0, 120.0, 0.5),
                              (95, 30, 100.0, 105.0, 0.25), (100, 80, 100.0, 110.0, 0.125), (97, 64, 100.0, 112.0, 0.25),
                              (103, 200, 100.0, 140.0, 0.2), (80, 120, 100.0, 110.0, 0.2)]:
    twt = np.around(np.arange(t0, t1, dt, dtype=np.float64), 5)
    x = (np.arange(ns) + 1).astype(np.float32)
    try:
        y = np.asarray(cb.pad_trace(da.from_array(x), delrt, twt, dt).compute())
    except AssertionError:
        continue
    pads.append((delrt, ns, t0, t1, dt, y))
out['pad/params'] = np.array([p[:5] for p in pads], dtype=np.float64)
for i, p in enumerate(pads):
    out[f'pad/{i}'] = p[5]

# ---- stacked bins ------------------------------------------------------------------------------------------------------------
dt, t0, t1 = 0.25, 50.0, 80.0
twt = np.around(np.arange(t0, t1, dt, dtype=np.float64), 5)
folds = [1, 2, 3, 4, 5, 7, 8, 12, 20]
ntr = sum(folds)
ns = 120
delays, samples = [], []
for k in folds:
    for _ in range(k):
        # start inside the window, or before it with the end inside / beyond (the cases pad_trace handles)
        if rng.random() < 0.5:
            d = int(rng.integers(50, 60))
            n = int(np.around((t1 - d) / dt)) + int(rng.integers(1, 20))    # ends past the window: clipped at the bottom
        else:
            d = int(rng.integers(40, 50))
            n = ns
        delays.append(d)
        samples.append(rng.standard_normal(n).astype(np.float32))
bin_of = np.repeat(np.arange(len(folds)), folds)
dist = rng.uniform(0.5, 5.0, ntr)
dist[bin_of == 3] = 2.0                        # a tie: the first trace wins
factor = 1.5
padded = [cb.pad_trace(da.from_array(s), d, twt, dt) for s, d in zip(samples, delays)]
res = {m: [] for m in ('average', 'median', 'nearest', 'IDW')}
for b, k in enumerate(folds):
    idx = np.flatnonzero(bin_of == b)
    tr = [padded[i] for i in idx]
    if k == 1:
        for m in res:
            res[m].append(np.asarray(tr[0].compute()))
        continue
    stk = da.stack(tr)
    res['average'].append(np.asarray(da.mean(stk, axis=0).compute()))
    res['median'].append(np.asarray(da.median(stk, axis=0).compute()))
    df = pd.DataFrame({'d': dist[idx]})
    res['nearest'].append(np.asarray(tr[int(df['d'].idxmin())].compute()))
    w = 1 / pd.Series(dist[idx]) ** factor
    wn = (w / w.sum()).values
    res['IDW'].append(np.asarray((stk * wn[..., np.newaxis]).sum(axis=0).compute()))
out['stack/twt'] = twt
out['stack/dt'] = np.float64(dt)
out['stack/folds'] = np.asarray(folds)
out['stack/delays'] = np.asarray(delays, dtype=np.float64)
out['stack/lengths'] = np.asarray([s.size for s in samples])
out['stack/samples'] = np.concatenate(samples)
out['stack/dist'] = dist
out['stack/factor'] = np.float64(factor)
for m, v in res.items():
    out[f'stack/{m}'] = np.stack(v)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'binning.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')
