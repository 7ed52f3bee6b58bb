"""Step-6 rates on the GPU: the tide prediction on resident points and tables (``p3d_tide_predict_dev`` on device buffers), the float64 NumPy oracle
of tests/helpers/tide_numpy.py on the host for the same points, and ``06_compensate_tide`` end to end on one file.

Case (default): 1e6 points with 8 constituents on the synthetic model of the tests (72 x 37 nodes), times over 50 years.  The figure is a CALL time,
not a kernel time: one host-clock window spans --calls calls in a row, each of them a launch followed by a device synchronisation, and the time per
call is the window divided by --calls; the minimum of --reps windows after a warm-up window is reported.  What part of a call is the launch and the
synchronisation is not measured here (a kernel trace would tell).  End to end: one SEG-Y file of 20 000 traces x 1000 samples.  Prints one JSON
document; no threshold is applied.

    timeout 300 python tools/tide_rate.py [--points 1000000 --traces 20000 --calls 200 --reps 3 --out profiles/tide_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import tide_numpy as H  # noqa: E402
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd import tide_compensation_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions.tide_model import load_subset  # noqa: E402


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
    p.add_argument('--traces', type=int, default=20000)
    p.add_argument('--samples', type=int, default=1000)
    p.add_argument('--calls', type=int, default=200)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    n, names = a.points, H.CONSTITUENTS[:8]
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, 'model')
        H.make_model(model, constituents=names)
        lon, lat, t = rng.uniform(100, 160, n), rng.uniform(-60, 20, n), np.rint(rng.uniform(-2.2e8, 1.35e9, n))
        sub = load_subset(model, names, lon, lat)
        nc, nxs, nys = sub.hre.shape
        arrays = [(sub.lon, np.float64), (lat, np.float64), (t, np.float64), (sub.hre, np.int32), (sub.him, np.int32), (sub.wet, np.uint8)]
        bufs = []
        try:
            for v, dt in arrays:
                bufs.append(_ffi.DeviceArray(np.shape(v), dt))
                bufs[-1].upload(np.ascontiguousarray(v, dtype=dt))
            bufs.append(_ffi.DeviceArray((n,), np.float64))
            ptrs, (grid, ids) = [b.ptr for b in bufs], (sub.grid, sub.ids)

            def window():
                for _ in range(a.calls):
                    _ffi.tide_predict_dev(*ptrs[:3], n, *ptrs[3:6], nc, nxs, nys, grid, ids, ptrs[6])
            call_s = min_of(window, a.reps) / a.calls
            got = bufs[6].download()
        finally:
            for b in bufs:
                b.free()
        t0 = time.perf_counter()
        want = H.predict(sub.lon, lat, t, sub.hre, sub.him, sub.wet.astype(bool), *sub.grid, names)
        host_s = time.perf_counter() - t0

        ntr, ns = a.traces, a.samples
        seconds = np.arange(ntr) * 3
        headers = {'SourceX': np.rint((120 + np.arange(ntr) * 1e-4) * 3600000).astype(np.int64), 'SourceY': np.rint((-30 + np.arange(ntr) * 5e-5) * 3600000).astype(np.int64),
                   'CoordinateUnits': 2, 'SourceGroupScalar': 1, 'YearDataRecorded': 2024, 'DayOfYear': 100 + seconds // 86400,
                   'HourOfDay': seconds // 3600 % 24, 'MinuteOfHour': seconds // 60 % 60, 'SecondOfMinute': seconds % 60}
        src = S.write_segy(os.path.join(tmp, 'line.sgy'), rng.standard_normal((ntr, ns)).astype(np.float32), 0.05, headers=headers)

        def run():
            try:
                cli.main(['06_compensate_tide', src, model])
            except SystemExit:
                pass
        file_s = min_of(run, 1)
    res = {'case': dict(points=n, constituents=len(names), model_nodes=[72, 37], calls_per_window=a.calls, windows=a.reps, statistic='min of the windows'),
           'call_with_launch_and_synchronisation': {'ms': round(call_s * 1e3, 4), 'Mpoints_per_s': round(n / call_s / 1e6, 1)},
           'numpy_oracle_on_the_host': {'ms': round(host_s * 1e3, 1), 'Mpoints_per_s': round(n / host_s / 1e6, 2)},
           'max_difference_m': float(np.nanmax(np.abs(got - want))),
           'file_end_to_end': {'traces': ntr, 'samples': ns, 's': round(file_s, 3)}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
