"""Rate of the FFT loop with one mask PER SLICE (P3D_FLAG_MASK_PER_SLICE) on one resident batch: --slices (64) complex64 slices of --shape
(1024 x 1024), --niter (20) iterations, hard threshold, exponential schedule from the batch's own statistics, 70 % of the traces missing.

Three loops on the same cube, device milliseconds of the loop itself (the events of the C entry, no transfers):
  per_slice       a (nslices, nil, nxl) mask on the plan a caller gets: the loop takes the unfused passes (fft2 | threshold | ifft2 | update) on the plan's
                  generic twin, the update pass reads mask[s] -- nslices masks streamed from HBM
  shared_unfused  the same job with ONE mask (slice 0's) on a plan forced onto the same unfused passes (P3D_FORCE_GENERIC at plan creation): the
                  like-for-like comparison -- both move 108 B per point and iteration, the shared mask is served from cache
  shared_fused    the shared-mask job on the plan a caller gets (fused row / column passes) -- for scale
Medians of --reps runs after one warm-up run.  Prints one JSON line; no threshold is applied.

    python tools/mask3d_rate.py [--shape 1024 1024 --slices 64 --niter 20 --reps 3 --out profiles/mask3d_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402
from dct_rate import cube_of  # noqa: E402


def time_loop(plan, x, mask, niter, reps):
    n, nil, nxl = x.shape
    per_slice = mask.ndim == 3
    xd, od, md = plan.alloc(x.nbytes).upload(x), plan.alloc(x.nbytes), plan.alloc(mask.nbytes).upload(mask)
    stats = plan.stats_dev(xd.ptr, _ffi.P3D_C64, n)
    tau = P._schedule_from_stats(stats, nil * nxl, 'exponential', niter, 0.99, 1e-3, 'values')
    ms = [plan.run_dev(xd.ptr, _ffi.P3D_C64, md.ptr, tau, niter, od.ptr, n, thresh_op='hard', mask_per_slice=per_slice)[2] for _ in range(reps + 1)][1:]
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
    full, _ = cube_of(a.slices, nil, nxl, 0.0)
    masks = (np.random.default_rng(1).random((a.slices, nil, nxl)) >= 0.7).astype(np.float32)     # a mask of its own for every slice
    x_own = full * masks                      # every slice observed under its own mask ...
    x_one = full * masks[0]                   # ... and all of them under slice 0's
    res = {'shape': [a.slices, nil, nxl], 'dtype': 'complex64', 'niter': a.niter, 'thresh_op': 'hard', 'reps': a.reps}
    os.environ.pop('P3D_FORCE_GENERIC', None)
    with _ffi.Plan(nil, nxl, a.slices) as plan:
        res['per_slice'] = time_loop(plan, x_own, masks, a.niter, a.reps)
        res['shared_fused'] = time_loop(plan, x_one, masks[0], a.niter, a.reps)
    os.environ['P3D_FORCE_GENERIC'] = '1'          # read once, when a plan is created
    try:
        with _ffi.Plan(nil, nxl, a.slices) as plan:
            res['shared_unfused'] = time_loop(plan, x_one, masks[0], a.niter, a.reps)
    finally:
        del os.environ['P3D_FORCE_GENERIC']
    res['per_slice_over_shared_unfused_rate'] = round(res['shared_unfused']['ms'] / res['per_slice']['ms'], 3)
    res['per_slice_over_shared_fused_rate'] = round(res['shared_fused']['ms'] / res['per_slice']['ms'], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
