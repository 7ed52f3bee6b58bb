"""Rate of the double-precision FFT loop with a percentile operator (csrc/p3d_select64.hip inside csrc/p3d_f64.hip) next to the loops the plan already
had, on one resident batch: --slices (16) complex128 slices of --shape (1024 x 1024), --niter (20) iterations, 70 % of the traces missing.

Device milliseconds of the loop itself (the events of the C entry, no transfers):
  pct64           hard-percentile, percentages linear 97 -> 60: rows | columns forward | select | threshold | columns inverse
  fft64_fused     hard, exponential schedule from the batch's statistics: the two fused kernels per iteration -- for scale
  pct64_unfused   hard-percentile on a plan forced onto the line passes (P3D_F64_UNFUSED=1 at plan creation): fft2 | select | threshold | ifft2 | update
  fft64_unfused   hard on such a plan: the same passes without the select -- the difference is what the select adds
The two unfused rows come from a child process of their own, since the knob is read when a plan is created.
And the sort of the 'data-driven' model, wall milliseconds of the entry on the resident batch (fft2 + keys + sort + peaks; it synchronises):
  sort64          p3d_pocs64_sorted_spectrum: 128-bit keys, thirty-two 4-bit passes
  sort32          p3d_pocs_sorted_spectrum on the same slices narrowed to complex64: 64-bit keys, sixteen passes
Medians of --reps runs after one warm-up run, minimum and maximum beside them.  Prints one JSON line; no threshold is applied.

    python tools/pct64_rate.py [--shape 1024 1024 --slices 16 --niter 20 --reps 3 --out profiles/pct64_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402
from dct64_rate import cube_of  # noqa: E402  (the same cube as tools/dct64_rate.py)


def row(ms, n, niter):
    med = float(np.median(ms))
    return {'ms': round(med, 3), 'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'slice_iterations_per_s': round(n * niter / med * 1e3, 1),
            'iterations_per_s': round(niter / med * 1e3, 2)}


def time_loops(plan, x, mask, niter, reps):
    n, nil, nxl = x.shape
    xd, od, md = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x.shape, x.dtype), _ffi.DeviceArray(mask.shape, mask.dtype).upload(mask)
    tau = P._schedule_from_stats(plan.stats_dev(xd.ptr, _ffi.P3D_C128, n), nil * nxl, 'exponential', niter, 0.99, 1e-3, 'values')
    perc = P._schedule('linear', niter, 97, 60, 'factors', None, None, None, None, None)
    out = {}
    for name, sched, op in (('pct64', perc, 'hard-percentile'), ('fft64', tau, 'hard')):
        out[name] = row([plan.run_dev(xd.ptr, _ffi.P3D_C128, md.ptr, sched, niter, od.ptr, n, thresh_op=op)[2] for _ in range(reps + 1)][1:], n, niter)
    for b in (xd, od, md):
        b.free()
    return out


def time_sorts(plan64, x, reps):
    n, nil, nxl = x.shape
    x32 = x.astype(np.complex64)
    xd, xd32 = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x32.shape, x32.dtype).upload(x32)
    out = {}
    with _ffi.Plan(nil, nxl, n) as plan32:
        for name, call in (('sort64', lambda: plan64.sorted_spectrum_dev(xd.ptr, _ffi.P3D_C128, n)), ('sort32', lambda: plan32.sorted_spectrum_dev(xd32.ptr, n))):
            ms = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            out[name] = {'ms': round(float(np.median(ms[1:])), 3), 'ms_min_max': [round(min(ms[1:]), 3), round(max(ms[1:]), 3)]}
    for b in (xd, xd32):
        b.free()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=2, default=[1024, 1024])
    p.add_argument('--slices', type=int, default=16)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--unfused-rows', action='store_true', help='(the child process, under P3D_F64_UNFUSED=1) time the two loops and print their rows')
    a = p.parse_args()
    nil, nxl = a.shape
    x, mask = cube_of(a.slices, nil, nxl, 0.7)
    if a.unfused_rows:
        with _ffi.Plan64(nil, nxl, a.slices) as plan:
            r = time_loops(plan, x, mask, a.niter, a.reps)
        print(json.dumps({'pct64_unfused': r['pct64'], 'fft64_unfused': r['fft64']}))
        return
    res = {'shape': [a.slices, nil, nxl], 'dtype': 'complex128', 'niter': a.niter, 'thresh_op': 'hard-percentile', 'percentages': [97, 60], 'reps': a.reps,
           'select_bytes_per_point_and_iteration': [56, 64]}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--unfused-rows', '--shape', str(nil), str(nxl), '--slices', str(a.slices), '--niter', str(a.niter),
                            '--reps', str(a.reps)], env=dict(os.environ, P3D_F64_UNFUSED='1'), capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit(f'the P3D_F64_UNFUSED=1 child failed ({child.returncode}): {child.stderr[-2000:]}')
    res.update(json.loads(child.stdout.strip().splitlines()[-1]))
    os.environ.pop('P3D_F64_UNFUSED', None)
    with _ffi.Plan64(nil, nxl, a.slices) as plan:
        r = time_loops(plan, x, mask, a.niter, a.reps)
        res['pct64'], res['fft64_fused'] = r['pct64'], r['fft64']
        res.update(time_sorts(plan, x, a.reps))
    res['select_share_of_pct64_unfused'] = round(1.0 - res['fft64_unfused']['ms'] / res['pct64_unfused']['ms'], 3)
    res['pct64_over_fft64_fused_rate'] = round(res['fft64_fused']['ms'] / res['pct64']['ms'], 3)
    res['sort64_over_sort32_time'] = round(res['sort64']['ms'] / res['sort32']['ms'], 2)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
