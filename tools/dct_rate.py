"""Rate of the DCT loop (transform_kind='DCT', csrc/p3d_dct.hip) next to the FFT loop on one resident batch: --slices (64) complex64 slices of
--shape (1024 x 1024), --niter (20) iterations, hard threshold, exponential schedule from the batch's own statistics, 70 % of the traces missing.

Four loops on the same cube, device milliseconds of the loop itself (the events of the C entry, no transfers):
  dct            the DCT loop on the plan a caller gets (the tuned / register-engine 2-D FFT + group pass + update pass)
  fft_fused      the FFT loop a caller gets (fused row / column passes) -- for scale, not a like-for-like comparison
  dct_unfused    the DCT loop on a plan forced onto the any-length line FFT (P3D_FORCE_GENERIC at plan creation)
  fft_unfused    the FFT loop on such a plan: fft2 | threshold pass | ifft2 | update pass -- the pipeline the DCT loop has the memory passes of
Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied.

    python tools/dct_rate.py [--shape 1024 1024 --slices 64 --niter 20 --reps 3 --out profiles/dct_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402


def cube_of(n, nil, nxl, missing, seed=0):
    rng = np.random.default_rng(seed)
    il, xl = np.arange(nil)[:, None] / nil, np.arange(nxl)[None, :] / nxl
    x = np.zeros((n, nil, nxl), np.complex64)
    for s in range(min(n, 8)):
        acc = 0.02 * (rng.standard_normal((nil, nxl)) + 1j * rng.standard_normal((nil, nxl)))
        for _ in range(5):
            k1, k2 = rng.integers(-nil // 8, nil // 8 + 1), rng.integers(-nxl // 8, nxl // 8 + 1)
            acc = acc + (rng.standard_normal() + 1j * rng.standard_normal()) * np.exp(2j * np.pi * (k1 * il + k2 * xl))
        x[s] = acc
    for s in range(8, n):   # (eight distinct slices, the others scaled copies: the host should not spend longer making the cube than the GPU iterating)
        x[s] = x[s % 8] * np.float32(1.0 + 0.01 * s)
    mask = (rng.random((nil, nxl)) >= missing).astype(np.float32)
    return x * mask, mask


def time_loop(plan, dct, x, mask, niter, reps):
    n, nil, nxl = x.shape
    xd, od, md = plan.alloc(x.nbytes).upload(x), plan.alloc(x.nbytes), plan.alloc(mask.nbytes).upload(mask)
    stats = plan.dct_stats_dev(xd.ptr, _ffi.P3D_C64, n, norm='ortho') if dct else plan.stats_dev(xd.ptr, _ffi.P3D_C64, n)
    tau = P._schedule_from_stats(stats, nil * nxl, 'exponential', niter, 0.99, 1e-3, 'values')
    run = (lambda: plan.dct_run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, niter, od.ptr, n, thresh_op='hard', norm='ortho')) if dct else \
          (lambda: plan.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, niter, od.ptr, n, thresh_op='hard'))
    ms = [run()[2] for _ in range(reps + 1)][1:]
    for b in (xd, od, md):
        b.free()
    med = float(np.median(ms))
    return {'ms': round(med, 3), 'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'slice_iterations_per_s': round(n * niter / med * 1e3, 1),
            'iterations_per_s': round(niter / med * 1e3, 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=2, default=[1024, 1024])
    p.add_argument('--slices', type=int, default=64)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    nil, nxl = a.shape
    x, mask = cube_of(a.slices, nil, nxl, 0.7)
    res = {'shape': [a.slices, nil, nxl], 'dtype': 'complex64', 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps}
    os.environ.pop('P3D_FORCE_GENERIC', None)
    with _ffi.Plan(nil, nxl, a.slices) as plan:
        res['dct'] = time_loop(plan, True, x, mask, a.niter, a.reps)
        res['fft_fused'] = time_loop(plan, False, x, mask, a.niter, a.reps)
    os.environ['P3D_FORCE_GENERIC'] = '1'          # read once, when a plan is created
    try:
        with _ffi.Plan(nil, nxl, a.slices) as plan:
            res['dct_unfused'] = time_loop(plan, True, x, mask, a.niter, a.reps)
            res['fft_unfused'] = time_loop(plan, False, x, mask, a.niter, a.reps)
    finally:
        del os.environ['P3D_FORCE_GENERIC']
    res['dct_over_fft_unfused_rate'] = round(res['fft_unfused']['ms'] / res['dct_unfused']['ms'], 3)
    res['dct_over_fft_fused_rate'] = round(res['fft_fused']['ms'] / res['dct']['ms'], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
