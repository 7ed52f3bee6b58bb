"""Rate of windowed POCS on one resident batch: --slices (64) complex64 slices of --shape (1024 x 1024), windows of --window (64 x 64) with --overlap (32),
--niter (20) iterations, hard threshold, exponential schedule from every window's own statistics, 70 % of the traces missing.

Device milliseconds of the loop itself (the events of the C entries, no transfers), --reps (3) repetitions of one run after a warm-up run:
  one_kernel      p3d_patch_run_dev: the whole loop of every window in one kernel, a workgroup per window, one packed mask per window
  generic         the same patch cube through the plan's own loop with P3D_FLAG_MASK_PER_SLICE and one materialised mask window per job (the unfused passes
                  fft2 | threshold | ifft2 | update): what windowed POCS costs with the kernels that existed before -- the comparator
  whole_slice     the cube itself, every slice ONE job, on the fused passes of the plan a caller gets -- for scale only (another job: one spectrum per slice)
and the wall-clock milliseconds of the gather and blend calls (synchronous entries) with their bytes per point of the cube.
Prints one JSON line; no threshold is applied.

    python tools/patch_rate.py [--shape 1024 1024 --slices 64 --window 64 64 --overlap 32 --niter 20 --reps 3 --out profiles/patch_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import POCS as P  # noqa: E402
from dct_rate import cube_of  # noqa: E402


def summary(ms, work):
    med = float(np.median(ms))
    return {'ms': round(med, 3), 'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'point_iterations_per_s': round(work / med * 1e3, 1)}


def wall(fn, reps):
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=2, default=[1024, 1024])
    p.add_argument('--slices', type=int, default=64)
    p.add_argument('--window', type=int, nargs=2, default=[64, 64])
    p.add_argument('--overlap', type=int, default=32)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    (nil, nxl), (w_il, w_xl), n, niter = a.shape, a.window, a.slices, a.niter
    x, mask = cube_of(n, nil, nxl, 0.7)
    s_il, s_xl = P.patch_starts(nil, w_il, a.overlap), P.patch_starts(nxl, w_xl, a.overlap)
    npatch = len(s_il) * len(s_xl)
    njobs = n * npatch
    dt, prm = _ffi.P3D_C64, dict(thresh_op='hard')
    res = {'shape': [n, nil, nxl], 'window': [w_il, w_xl], 'overlap': a.overlap, 'windows_per_slice': npatch, 'jobs': njobs, 'dtype': 'complex64', 'niter': niter,
           'thresh_op': 'hard', 'reps': a.reps, 'patch_points_per_cube_point': round(npatch * w_il * w_xl / (nil * nxl), 3)}
    os.environ.pop('P3D_NO_PATCH_RESIDENT', None)
    with _ffi.Plan(w_il, w_xl, njobs) as plan, _ffi.PatchPlan(plan, nil, nxl, s_il, s_xl, P.patch_taper(w_il), P.patch_taper(w_xl), n) as pp:
        per = w_il * w_xl
        xd, od, md = plan.alloc(x.nbytes).upload(x), plan.alloc(x.nbytes), plan.alloc(mask.nbytes).upload(mask)
        pd, qd, mw = plan.alloc(njobs * per * 8), plan.alloc(njobs * per * 8), plan.alloc(njobs * per * 4)
        points = n * nil * nxl
        # gather: reads every window's points from the cube (the overlap from cache), writes the patch cube
        res['gather'] = {'ms': round(float(np.median(wall(lambda: pp.gather_dev(xd.ptr, dt, n, pd.ptr), a.reps))), 3),
                         'bytes_per_cube_point': round(8 + 8 * njobs * per / points, 2)}
        assert not pp.mask_dev(md.ptr, 1, n, mw.ptr) and pp.route('hard')
        stats = plan.stats_dev(pd.ptr, dt, njobs)
        active = ~(stats[:, 2] == 0)
        stats[~active] = 1.0
        tau = P._schedule_from_stats(stats, per, 'exponential', niter, 0.99, 1e-3, 'values')
        work = float(njobs) * per * niter
        res['one_kernel'] = summary([pp.run_dev(pd.ptr, dt, tau, niter, qd.ptr, n, active=active, **prm)[2] for _ in range(a.reps + 1)][1:], work)
        one = qd.download((npatch, w_il, w_xl), np.complex64)
        res['generic'] = summary([plan.run_dev(pd.ptr, dt, mw.ptr, tau, niter, qd.ptr, njobs, active=active, mask_per_slice=True, want_sums=False, **prm)[2]
                                  for _ in range(a.reps + 1)][1:], work)
        gen = qd.download((npatch, w_il, w_xl), np.complex64)
        res['routes_rel_l2_first_slice'] = float(np.linalg.norm(gen - one) / np.linalg.norm(one))
        # blend: reads every window result once, writes the cube
        res['blend'] = {'ms': round(float(np.median(wall(lambda: pp.blend_dev(qd.ptr, dt, active, od.ptr, n), a.reps))), 3),
                        'bytes_per_cube_point': round(8 + 8 * njobs * per / points, 2)}
        for b in (xd, od, md, pd, qd, mw):
            b.free()
    with _ffi.Plan(nil, nxl, n) as plan:
        xd, od, md = plan.alloc(x.nbytes).upload(x), plan.alloc(x.nbytes), plan.alloc(mask.nbytes).upload(mask)
        stats = plan.stats_dev(xd.ptr, dt, n)
        tau = P._schedule_from_stats(stats, nil * nxl, 'exponential', niter, 0.99, 1e-3, 'values')
        res['whole_slice'] = summary([plan.run_dev(xd.ptr, dt, md.ptr, tau, niter, od.ptr, n, want_sums=False, **prm)[2] for _ in range(a.reps + 1)][1:],
                                     float(n) * nil * nxl * niter)
        for b in (xd, od, md):
            b.free()
    res['one_kernel_over_generic_rate'] = round(res['generic']['ms'] / res['one_kernel']['ms'], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
