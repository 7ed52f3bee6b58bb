"""Rate of 3-D FFT POCS (pocs_volume, csrc/p3d_vol.hip) on one resident volume: --shape (256 x 512 x 512) complex64, --missing (80 %) of the traces
missing, --niter (20) iterations, hard threshold, exponential schedule from the volume's own statistics.

Device milliseconds of the loops themselves (the events of the C entries, no transfers), in one process:
  volume       the volume loop: fft2 of every slice | axis-0 transform + threshold + inverse in one kernel | ifft2 | update
  slices       the SAME array as 256 independent slices through the unfused 2-D FFT loop (a mask per slice: the route pocs_cube takes for
               (nslices, nil, nxl) masks), which has the same fft2 | threshold | ifft2 | update structure without the axis-0 pass
  zpass        the axis-0 kernel alone (HIP events around every launch of a profiled run), and the bytes it must move -- 2 x 8 B per point --
               as a fraction of the 6.29 TB/s copy ceiling of DESIGN.md section 8
Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied.

    python tools/vol_rate.py [--shape 256 512 512 --niter 20 --reps 3 --out profiles/vol_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402

COPY_CEILING_TBS = 6.29


def volume_of(n0, n1, n2, missing, seed=0):
    """A few plane waves through the volume plus noise, complex64, and a binary (n1, n2) trace mask."""
    rng = np.random.default_rng(seed)
    z, il, xl = np.arange(n0)[:, None, None] / n0, np.arange(n1)[None, :, None] / n1, np.arange(n2)[None, None, :] / n2
    x = np.zeros((n0, n1, n2), np.complex64)
    for _ in range(5):
        k0, k1, k2 = (int(rng.integers(-n // 8, n // 8 + 1)) for n in (n0, n1, n2))
        amp = np.complex64(rng.standard_normal() + 1j * rng.standard_normal())
        x += amp * (np.exp(2j * np.pi * k0 * z).astype(np.complex64) * np.exp(2j * np.pi * k1 * il).astype(np.complex64)
                    * np.exp(2j * np.pi * k2 * xl).astype(np.complex64))
    x += (0.02 * (rng.standard_normal((n0, n1, n2), dtype=np.float32) + 1j * rng.standard_normal((n0, n1, n2), dtype=np.float32))).astype(np.complex64)
    mask = (rng.random((n1, n2)) >= missing).astype(np.float32)
    return x * mask, mask


def summary(ms, points, niter):
    med = float(np.median(ms))
    return {'ms': round(med, 3), 'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'ms_per_iteration': round(med / niter, 4),
            'gpoint_per_s': round(points * niter / med * 1e-6, 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=3, default=[256, 512, 512])
    p.add_argument('--missing', type=float, default=0.8)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    n0, n1, n2 = a.shape
    x, mask = volume_of(n0, n1, n2, a.missing)
    points = x.size
    res = {'shape': [n0, n1, n2], 'dtype': 'complex64', 'missing': a.missing, 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps}
    xd, od = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x.shape, x.dtype)
    md = _ffi.DeviceArray(mask.shape, np.float32).upload(mask)

    with _ffi.VolumePlan(n0, n1, n2) as vol:
        tau = P._schedule_from_stats(vol.stats_dev(xd.ptr, _ffi.P3D_C64), points, 'exponential', a.niter, 0.99, 1e-3, 'values')[0]
        ms = [vol.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, a.niter, od.ptr, thresh_op='hard')[2] for _ in range(a.reps + 1)][1:]
        res['volume'] = summary(ms, points, a.niter)
        zms = []
        for _ in range(a.reps):
            vol.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, a.niter, od.ptr, thresh_op='hard', profile=True)
            zms.append(vol.last_profile()['zpass_ms'])
        z = float(np.median(zms))
        tbs = 2 * 8 * points / (z * 1e-3) * 1e-12
        res['zpass'] = {'ms': round(z, 4), 'ms_min_max': [round(min(zms), 4), round(max(zms), 4)], 'bytes_needed': 2 * 8 * points, 'tb_per_s': round(tbs, 3),
                        'fraction_of_copy_ceiling': round(tbs / COPY_CEILING_TBS, 3), 'copy_ceiling_tb_per_s': COPY_CEILING_TBS}

    # the same array as n0 independent slices, one mask each: the unfused 2-D loop
    ms3 = _ffi.DeviceArray(x.shape, np.float32).upload(np.ascontiguousarray(np.broadcast_to(mask, x.shape)))
    with _ffi.Plan(n1, n2, n0) as plan:
        tau2 = P._schedule_from_stats(plan.stats_dev(xd.ptr, _ffi.P3D_C64, n0), n1 * n2, 'exponential', a.niter, 0.99, 1e-3, 'values')
        ms = [plan.run_dev(xd.ptr, _ffi.P3D_C64, ms3.ptr, tau2, a.niter, od.ptr, n0, thresh_op='hard', mask_per_slice=True)[2] for _ in range(a.reps + 1)][1:]
        res['slices'] = summary(ms, points, a.niter)
    res['volume_over_slices_time'] = round(res['volume']['ms'] / res['slices']['ms'], 3)
    for d in (xd, od, md, ms3):
        d.free()
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
