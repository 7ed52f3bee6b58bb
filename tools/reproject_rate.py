"""Step-2 projection rate on the GPU: the forward and the inverse transverse Mercator kernel alone on resident points (device buffers), and a
device-to-device hipMemcpy of the same two arrays in the same process for scale.

Case (default): 1e6 points of a UTM zone (WGS84 / UTM 60S), latitudes -80 ... 84 degrees, up to 4 degrees from the central meridian; the minimum of
--reps runs after a warm-up (each run includes the launch and a device synchronisation).  Prints one JSON document; no threshold is applied.

    timeout 300 python tools/reproject_rate.py [--points 1000000 --reps 3 --out profiles/reproject_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions.crs import parse_crs  # noqa: E402


def min_of(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(min(ts[1:]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--points', type=int, default=1000000)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    n = a.points
    prm = parse_crs('EPSG:32760').prm
    rng = np.random.default_rng(0)
    lon, lat = 177 + rng.uniform(-4, 4, n), rng.uniform(-80, 84, n)
    dlon, dlat = _ffi.DeviceArray((n,), np.float64).upload(lon), _ffi.DeviceArray((n,), np.float64).upload(lat)
    de, dn = _ffi.DeviceArray((n,), np.float64), _ffi.DeviceArray((n,), np.float64)
    dlon2, dlat2 = _ffi.DeviceArray((n,), np.float64), _ffi.DeviceArray((n,), np.float64)
    copy_s = min_of(lambda: (dlon2.copy_from(dlon), dlat2.copy_from(dlat)), a.reps)
    fwd_s = min_of(lambda: _ffi.proj_tmerc_dev(dlon.ptr, dlat.ptr, n, prm, False, de.ptr, dn.ptr), a.reps)
    inv_s = min_of(lambda: _ffi.proj_tmerc_dev(de.ptr, dn.ptr, n, prm, True, dlon2.ptr, dlat2.ptr), a.reps)
    back = max(float(np.abs(dlon2.download() - lon).max()), float(np.abs(dlat2.download() - lat).max()))
    for b in (dlon, dlat, de, dn, dlon2, dlat2):
        b.free()
    res = {'case': dict(points=n, crs='EPSG:32760', reps=a.reps, statistic='min'),
           'd2d_copy_of_both_arrays': {'ms': round(copy_s * 1e3, 4)},
           'forward_kernel': {'ms': round(fwd_s * 1e3, 4), 'Mpoints_per_s': round(n / fwd_s / 1e6, 1)},
           'inverse_kernel': {'ms': round(inv_s * 1e3, 4), 'Mpoints_per_s': round(n / inv_s / 1e6, 1)},
           'round_trip_max_error_degrees': back}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
