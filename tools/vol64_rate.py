"""Rate of the double-precision 3-D FFT POCS loop (pocs_volume64, csrc/p3d_vol64.hip) on one resident volume: --shape (256 x 512 x 512) complex128,
--missing (80 %) of the traces missing, --niter (20) iterations, hard threshold, exponential schedule from the volume's own double-precision statistics.
The workload of tools/vol_rate.py, widened.

Device milliseconds of the loop itself (the events of the C entry, no transfers), in one process:
  volume       the loop: fft2 of every slice (the line passes of p3d_plan64) | axis-0 transform + threshold + inverse in one kernel | ifft2 | update
  zpass        the axis-0 kernel alone (HIP events around every launch of a profiled run), and the bytes it must move -- 2 x 16 B per point -- as a
               fraction of the 6.29 TB/s copy ceiling of DESIGN.md section 8
  float32      beside them, what profiles/vol_rate.json records for the float32 volume loop at the same shape (read from that file, not measured here)
Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied: a record, there is no earlier figure to hold it to.

    python tools/vol64_rate.py [--shape 256 512 512 --niter 20 --reps 3 --out profiles/vol64_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402
from vol_rate import COPY_CEILING_TBS, summary, volume_of  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=3, default=[256, 512, 512])
    p.add_argument('--missing', type=float, default=0.8)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    n0, n1, n2 = a.shape
    x32, mask32 = volume_of(n0, n1, n2, a.missing)
    x, mask = x32.astype(np.complex128), mask32.astype(np.float64)
    del x32
    points = x.size
    res = {'shape': [n0, n1, n2], 'dtype': 'complex128', 'missing': a.missing, 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps}
    xd, od = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x.shape, x.dtype)
    md = _ffi.DeviceArray(mask.shape, np.float64).upload(mask)

    with _ffi.VolumePlan64(n0, n1, n2) as vol:
        tau = P._schedule_from_stats(vol.stats_dev(xd.ptr, _ffi.P3D_C128), points, 'exponential', a.niter, 0.99, 1e-3, 'values')[0]
        ms = [vol.run_dev(xd.ptr, _ffi.P3D_C128, md.ptr, tau, a.niter, od.ptr, thresh_op='hard')[2] for _ in range(a.reps + 1)][1:]
        res['volume'] = summary(ms, points, a.niter)
        zms = []
        for _ in range(a.reps):
            vol.run_dev(xd.ptr, _ffi.P3D_C128, md.ptr, tau, a.niter, od.ptr, thresh_op='hard', profile=True)
            zms.append(vol.last_profile()['zpass_ms'])
        z = float(np.median(zms))
        tbs = 2 * 16 * points / (z * 1e-3) * 1e-12
        res['zpass'] = {'ms': round(z, 4), 'ms_min_max': [round(min(zms), 4), round(max(zms), 4)], 'bytes_needed': 2 * 16 * points, 'tb_per_s': round(tbs, 3),
                        'fraction_of_copy_ceiling': round(tbs / COPY_CEILING_TBS, 3), 'copy_ceiling_tb_per_s': COPY_CEILING_TBS,
                        'share_of_iteration': round(z / res['volume']['ms_per_iteration'], 3)}
    for d in (xd, od, md):
        d.free()

    f32 = os.path.join(ROOT, 'profiles', 'vol_rate.json')
    if os.path.isfile(f32):
        with open(f32) as fh:
            rec = json.loads(fh.readline())
        if rec.get('shape') == [n0, n1, n2] and rec.get('niter') == a.niter:
            res['float32'] = {'source': 'profiles/vol_rate.json', 'volume': rec['volume'], 'zpass': rec['zpass']}
            res['double_over_float32_time'] = round(res['volume']['ms'] / rec['volume']['ms'], 2)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
