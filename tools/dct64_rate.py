"""Rate of the double-precision DCT loop (transform_kind='DCT', precision='reference'; csrc/p3d_dct64.hip) next to the double-precision FFT loop on one
resident batch: --slices (16) complex128 slices of --shape (1024 x 1024), --niter (20) iterations, hard threshold, exponential schedule from the
batch's own statistics, 70 % of the traces missing.

Four loops on the same cube, device milliseconds of the loop itself (the events of the C entry, no transfers):
  dct64          the DCT loop a caller gets: fft2 | group pass | ifft2 | update pass, the column transforms on the plan's own column kernels
  fft64_fused    the FFT loop a caller gets (two fused kernels per iteration) -- for scale, not a like-for-like comparison
  dct64_unfused  the DCT loop on a plan forced onto the line passes (P3D_F64_UNFUSED=1 at plan creation)
  fft64_unfused  the FFT loop on such a plan: fft2 | threshold pass | ifft2 | update pass -- by bytes the same loop as the DCT one (64 + 32 + 64 + 56
                 = 216 bytes per point and iteration)
The two unfused rows come from a child process of their own, since the knob is read when a plan is created.
Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied.

    python tools/dct64_rate.py [--shape 1024 1024 --slices 16 --niter 20 --reps 3 --out profiles/dct64_rate.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402


def cube_of(n, nil, nxl, missing, seed=0):
    rng = np.random.default_rng(seed)
    il, xl = np.arange(nil)[:, None] / nil, np.arange(nxl)[None, :] / nxl
    x = np.zeros((n, nil, nxl), np.complex128)
    for s in range(min(n, 4)):
        acc = 0.02 * (rng.standard_normal((nil, nxl)) + 1j * rng.standard_normal((nil, nxl)))
        for _ in range(5):
            k1, k2 = rng.integers(-nil // 8, nil // 8 + 1), rng.integers(-nxl // 8, nxl // 8 + 1)
            acc = acc + (rng.standard_normal() + 1j * rng.standard_normal()) * np.exp(2j * np.pi * (k1 * il + k2 * xl))
        x[s] = acc
    for s in range(4, n):   # (four distinct slices, the others scaled copies: the host should not spend longer making the cube than the GPU iterating)
        x[s] = x[s % 4] * (1.0 + 0.01 * s)
    mask = (rng.random((nil, nxl)) >= missing).astype(np.float64)
    return x * mask, mask


def time_loop(plan, dct, x, mask, niter, reps):
    n, nil, nxl = x.shape
    xd, od, md = _ffi.DeviceArray(x.shape, x.dtype).upload(x), _ffi.DeviceArray(x.shape, x.dtype), _ffi.DeviceArray(mask.shape, mask.dtype).upload(mask)
    stats = plan.dct_stats_dev(xd.ptr, _ffi.P3D_C128, n, norm='ortho') if dct else plan.stats_dev(xd.ptr, _ffi.P3D_C128, n)
    tau = P._schedule_from_stats(stats, nil * nxl, 'exponential', niter, 0.99, 1e-3, 'values')
    run = (lambda: plan.dct_run_dev(xd.ptr, _ffi.P3D_C128, md.ptr, tau, niter, od.ptr, n, thresh_op='hard', norm='ortho')) if dct else \
          (lambda: plan.run_dev(xd.ptr, _ffi.P3D_C128, md.ptr, tau, niter, od.ptr, n, thresh_op='hard'))
    ms = [run()[2] for _ in range(reps + 1)][1:]
    for b in (xd, od, md):
        b.free()
    med = float(np.median(ms))
    return {'ms': round(med, 3), 'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'slice_iterations_per_s': round(n * niter / med * 1e3, 1),
            'iterations_per_s': round(niter / med * 1e3, 2)}


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
            print(json.dumps({'dct64_unfused': time_loop(plan, True, x, mask, a.niter, a.reps), 'fft64_unfused': time_loop(plan, False, x, mask, a.niter, a.reps)}))
        return
    res = {'shape': [a.slices, nil, nxl], 'dtype': 'complex128', 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps, 'bytes_per_point_and_iteration': 216}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--unfused-rows', '--shape', str(nil), str(nxl), '--slices', str(a.slices), '--niter', str(a.niter),
                            '--reps', str(a.reps)], env=dict(os.environ, P3D_F64_UNFUSED='1'), capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit(f'the P3D_F64_UNFUSED=1 child failed ({child.returncode}): {child.stderr[-2000:]}')
    res.update(json.loads(child.stdout.strip().splitlines()[-1]))
    os.environ.pop('P3D_F64_UNFUSED', None)
    with _ffi.Plan64(nil, nxl, a.slices) as plan:
        res['dct64'] = time_loop(plan, True, x, mask, a.niter, a.reps)
        res['fft64_fused'] = time_loop(plan, False, x, mask, a.niter, a.reps)
    res['dct64_over_fft64_unfused_rate'] = round(res['fft64_unfused']['ms'] / res['dct64_unfused']['ms'], 3)   # like for like
    res['dct64_over_fft64_fused_rate'] = round(res['fft64_fused']['ms'] / res['dct64']['ms'], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
