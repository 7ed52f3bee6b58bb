"""Rate of 3-D DCT POCS (pocs_volume_dct, csrc/p3d_vol_dct.hip) on one resident volume, the workload of tools/vol_rate.py: --shape (256 x 512 x 512)
complex64, --missing (80 %) of the traces missing, --niter (20) iterations, hard threshold, exponential schedule from the volume's own statistics.

Device milliseconds of the loops themselves (the events of the C entries, no transfers), all in ONE process:
  volume_dct   the DCT volume loop: fft2 | combine | axis-0 cosine pass (transform, group step + threshold, inverse in one kernel) | split | ifft2 | update
  zpass_dct    its axis-0 kernel alone (HIP events around every launch of a profiled run)
  volume_fft   the FFT volume loop (pocs_volume) on the same array, and zpass_fft, its axis-0 kernel: what the cosine pass is reported against
  slices_dct   the SAME array as 256 independent slices through the 2-D DCT loop with a mask per slice
The byte model: 13 x 8 B per point and iteration for the FFT volume loop plus two group passes of 16 B, so the DCT loop is
reported against 17/13 of the FFT loop.  Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied, and what binds
the axis-0 pass is not measured here.

    python tools/vol_dct_rate.py [--shape 256 512 512 --niter 20 --reps 3 --norm ortho --out profiles/vol_dct_rate.json]"""
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


def zpass(plan, run, points, reps):
    zms = []
    for _ in range(reps):
        run(profile=True)
        zms.append(plan.last_profile()['zpass_ms'])
    z = float(np.median(zms))
    tbs = 2 * 8 * points / (z * 1e-3) * 1e-12
    return {'ms': round(z, 4), 'ms_min_max': [round(min(zms), 4), round(max(zms), 4)], 'bytes_needed': 2 * 8 * points, 'tb_per_s': round(tbs, 3),
            'fraction_of_copy_ceiling': round(tbs / COPY_CEILING_TBS, 3), 'copy_ceiling_tb_per_s': COPY_CEILING_TBS}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=3, default=[256, 512, 512])
    p.add_argument('--missing', type=float, default=0.8)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--norm', type=str, default='ortho', choices=['ortho', 'backward'])
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    n0, n1, n2 = a.shape
    x, mask = volume_of(n0, n1, n2, a.missing)
    points = x.size
    res = {'shape': [n0, n1, n2], 'dtype': 'complex64', 'missing': a.missing, 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps, 'dct_norm': a.norm,
           'what_binds_the_axis0_pass': 'not measured'}
    xd, od = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x.shape, x.dtype)
    md = _ffi.DeviceArray(mask.shape, np.float32).upload(mask)

    with _ffi.VolumePlanDct(n0, n1, n2) as vol:
        tau = P._schedule_from_stats(vol.stats_dev(xd.ptr, _ffi.P3D_C64, norm=a.norm), points, 'exponential', a.niter, 0.99, 1e-3, 'values')[0]
        run = lambda **k: vol.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, a.niter, od.ptr, thresh_op='hard', norm=a.norm, **k)  # noqa: E731
        res['volume_dct'] = summary([run()[2] for _ in range(a.reps + 1)][1:], points, a.niter)
        res['zpass_dct'] = zpass(vol, run, points, a.reps)

    with _ffi.VolumePlan(n0, n1, n2) as vol:
        tau = P._schedule_from_stats(vol.stats_dev(xd.ptr, _ffi.P3D_C64), points, 'exponential', a.niter, 0.99, 1e-3, 'values')[0]
        run = lambda **k: vol.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, a.niter, od.ptr, thresh_op='hard', **k)  # noqa: E731
        res['volume_fft'] = summary([run()[2] for _ in range(a.reps + 1)][1:], points, a.niter)
        res['zpass_fft'] = zpass(vol, run, points, a.reps)

    # the same array as n0 independent slices, one mask each: the 2-D DCT loop
    ms3 = _ffi.DeviceArray(x.shape, np.float32).upload(np.ascontiguousarray(np.broadcast_to(mask, x.shape)))
    with _ffi.Plan(n1, n2, n0) as plan:
        tau2 = P._schedule_from_stats(plan.dct_stats_dev(xd.ptr, _ffi.P3D_C64, n0, norm=a.norm), n1 * n2, 'exponential', a.niter, 0.99, 1e-3, 'values')
        ms = [plan.dct_run_dev(xd.ptr, _ffi.P3D_C64, ms3.ptr, tau2, a.niter, od.ptr, n0, thresh_op='hard', norm=a.norm, mask_per_slice=True)[2]
              for _ in range(a.reps + 1)][1:]
        res['slices_dct'] = summary(ms, points, a.niter)
    res['zpass_dct_over_zpass_fft'] = round(res['zpass_dct']['ms'] / res['zpass_fft']['ms'], 3)
    res['volume_dct_over_volume_fft'] = round(res['volume_dct']['ms'] / res['volume_fft']['ms'], 3)
    res['byte_model_dct_over_fft'] = round(17 / 13, 3)
    res['volume_dct_over_slices_dct'] = round(res['volume_dct']['ms'] / res['slices_dct']['ms'], 3)
    for d in (xd, od, md, ms3):
        d.free()
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
