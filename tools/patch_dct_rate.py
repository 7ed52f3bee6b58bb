"""Rate of windowed DCT POCS on one resident batch, the job of tools/patch_rate.py: --slices (64) complex64 slices of --shape (1024 x 1024), windows of
--window (64 x 64) with --overlap (32), --niter (20) iterations, hard threshold, norm 'ortho', exponential schedule from every window's own DCT statistics,
70 % of the traces missing.

Device milliseconds of the loop itself (the events of the C entries, no transfers), --reps (3) repetitions after a warm-up run, three loops in one process:
  dct_one_kernel  p3d_patch_dct_run_dev: the whole DCT loop of every window in one kernel (resident_dct_kernel), a workgroup per window
  dct_generic     the same patch cube and schedule through the plan's generic DCT loop (p3d_pocs_dct_run_dev with P3D_FLAG_MASK_PER_SLICE and one materialised
                  mask window per job: update | fft2 | group pass | ifft2 per iteration), what the windowed driver runs with P3D_NO_PATCH_RESIDENT=1 -- the
                  kernels that existed before, the comparator
  fft_one_kernel  p3d_patch_run_dev on the same patch cube with its FFT schedule -- for scale only (another transform)
Prints one JSON line (median, min and max per loop); no threshold is applied.

    python tools/patch_dct_rate.py [--shape 1024 1024 --slices 64 --window 64 64 --overlap 32 --niter 20 --reps 3 --out profiles/patch_dct_rate.json]"""
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
from patch_rate import summary  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', type=int, nargs=2, default=[1024, 1024])
    p.add_argument('--slices', type=int, default=64)
    p.add_argument('--window', type=int, nargs=2, default=[64, 64])
    p.add_argument('--overlap', type=int, default=32)
    p.add_argument('--niter', type=int, default=20)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--norm', type=str, default='ortho')
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    (nil, nxl), (w_il, w_xl), n, niter, norm = a.shape, a.window, a.slices, a.niter, a.norm
    x, mask = cube_of(n, nil, nxl, 0.7)
    s_il, s_xl = P.patch_starts(nil, w_il, a.overlap), P.patch_starts(nxl, w_xl, a.overlap)
    npatch = len(s_il) * len(s_xl)
    njobs = n * npatch
    dt, prm = _ffi.P3D_C64, dict(thresh_op='hard')
    res = {'shape': [n, nil, nxl], 'window': [w_il, w_xl], 'overlap': a.overlap, 'windows_per_slice': npatch, 'jobs': njobs, 'dtype': 'complex64', 'niter': niter,
           'thresh_op': 'hard', 'norm': norm, 'reps': a.reps}
    os.environ.pop('P3D_NO_PATCH_RESIDENT', None)
    with _ffi.Plan(w_il, w_xl, njobs) as plan, _ffi.PatchPlan(plan, nil, nxl, s_il, s_xl, P.patch_taper(w_il), P.patch_taper(w_xl), n) as pp:
        per = w_il * w_xl
        xd, md = plan.alloc(x.nbytes).upload(x), plan.alloc(mask.nbytes).upload(mask)
        pd, qd, mw = plan.alloc(njobs * per * 8), plan.alloc(njobs * per * 8), plan.alloc(njobs * per * 4)
        pp.gather_dev(xd.ptr, dt, n, pd.ptr)
        assert not pp.mask_dev(md.ptr, 1, n, mw.ptr) and pp.route('hard', transform='DCT', norm=norm) and pp.route('hard')
        work = float(njobs) * per * niter

        def schedule(stats):
            active = ~(stats[:, 2] == 0)
            stats[~active] = 1.0
            return P._schedule_from_stats(stats, per, 'exponential', niter, 0.99, 1e-3, 'values'), active
        tau, active = schedule(plan.dct_stats_dev(pd.ptr, dt, njobs, norm=norm))
        res['dct_one_kernel'] = summary([pp.dct_run_dev(pd.ptr, dt, tau, niter, qd.ptr, n, active=active, norm=norm, **prm)[2] for _ in range(a.reps + 1)][1:], work)
        one = qd.download((npatch, w_il, w_xl), np.complex64)
        os.environ['P3D_NO_PATCH_RESIDENT'] = '1'
        assert not pp.route('hard', transform='DCT', norm=norm)
        res['dct_generic'] = summary([plan.dct_run_dev(pd.ptr, dt, mw.ptr, tau, niter, qd.ptr, njobs, active=active, norm=norm, mask_per_slice=True, want_sums=False,
                                                       **prm)[2] for _ in range(a.reps + 1)][1:], work)
        del os.environ['P3D_NO_PATCH_RESIDENT']
        gen = qd.download((npatch, w_il, w_xl), np.complex64)
        res['routes_rel_l2_first_slice'] = float(np.linalg.norm(gen - one) / np.linalg.norm(one))
        tau, active = schedule(plan.stats_dev(pd.ptr, dt, njobs))
        res['fft_one_kernel'] = summary([pp.run_dev(pd.ptr, dt, tau, niter, qd.ptr, n, active=active, **prm)[2] for _ in range(a.reps + 1)][1:], work)
        for b in (xd, md, pd, qd, mw):
            b.free()
    res['dct_one_kernel_over_generic_rate'] = round(res['dct_generic']['ms'] / res['dct_one_kernel']['ms'], 3)
    res['dct_over_fft_one_kernel_time'] = round(res['dct_one_kernel']['ms'] / res['fft_one_kernel']['ms'], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
