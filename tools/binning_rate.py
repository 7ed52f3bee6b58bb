"""Step-10 stacking rate on the GPU: p3d_bin_stack_dev on a survey-sized CSR layout, every method, against the copy ceiling.

Case (default): a 1024 x 1024 bin grid with 1024 twt samples, about 20 % of the bins covered with fold 1 ... 8, traces of 1024 samples
shifted by -64 ... +64 samples.  Bytes counted: the selected trace samples read (their overlap with the window, once) plus the cube
written.  Host preparation (IBM SEG-Y decode, the stable sort into bin order) is timed separately.  Prints one JSON document.

    python tools/binning_rate.py [--nil 1024 --nxl 1024 --nt 1024 --cover 0.2 --maxfold 8 --reps 5 --out profiles/binning_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402

CEILING = 6.29e12


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nil', type=int, default=1024)
    p.add_argument('--nxl', type=int, default=1024)
    p.add_argument('--nt', type=int, default=1024)
    p.add_argument('--ns', type=int, default=1024)
    p.add_argument('--cover', type=float, default=0.2)
    p.add_argument('--maxfold', type=int, default=8)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    rng = np.random.default_rng(0)
    nb = a.nil * a.nxl
    fold = np.where(rng.random(nb) < a.cover, rng.integers(1, a.maxfold + 1, nb), 0)
    ntr = int(fold.sum())
    bs = np.r_[0, np.cumsum(fold)].astype(np.int64)
    ln = np.full(ntr, a.ns, np.int32)
    sh = rng.integers(-64, 65, ntr).astype(np.int32)
    off = np.arange(ntr, dtype=np.int64) * a.ns
    smp = rng.standard_normal(ntr * a.ns, dtype=np.float32)
    w = np.ones(ntr) / np.repeat(np.maximum(fold, 1), fold)
    read = int(np.clip(np.minimum(ln + sh, a.nt) - np.maximum(sh, 0), 0, None).sum()) * 4
    written = a.nt * nb * 4
    res = {'case': dict(nil=a.nil, nxl=a.nxl, nt=a.nt, ns=a.ns, traces=ntr, covered_bins=int((fold > 0).sum()), maxfold=a.maxfold),
           'bytes_read': read, 'bytes_written': written, 'ceiling_GBps': CEILING / 1e9, 'methods': {}}
    bufs = [_ffi.DeviceArray(x.shape, x.dtype).upload(x) for x in (smp, off, ln, sh, w, bs)]
    out = _ffi.DeviceArray((a.nt, a.nil, a.nxl), np.float32)
    for m in ('average', 'median', 'nearest', 'IDW'):
        if m == 'nearest':                        # one trace per bin: the first of each
            bsn = np.r_[0, np.cumsum(fold > 0)].astype(np.int64)
            first = bs[:-1][fold > 0]
            tb = [_ffi.DeviceArray(x.shape, x.dtype).upload(x) for x in (off[first], ln[first], sh[first], bsn)]
            args = (bufs[0].ptr, tb[0].ptr, tb[1].ptr, tb[2].ptr, tb[3].ptr)
            rd = int(np.clip(np.minimum(ln[first] + sh[first], a.nt) - np.maximum(sh[first], 0), 0, None).sum()) * 4
        else:
            args = (bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[5].ptr)
            rd = read
        ts = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            _ffi.bin_stack_dev(*args, out.ptr, a.nil, a.nxl, a.nt, method=m, weight=bufs[4].ptr)
            ts.append(time.perf_counter() - t0)
        best = min(ts[1:])
        res['methods'][m] = {'ms': round(best * 1e3, 3), 'ms_median': round(float(np.median(ts[1:])) * 1e3, 3),
                             'GBps': round((rd + written) / best / 1e9, 1), 'frac_ceiling': round((rd + written) / best / CEILING, 3)}
        if m == 'nearest':
            for b in tb:
                b.free()
    for b in bufs + [out]:
        b.free()
    res['median_over_average'] = round(res['methods']['median']['ms'] / res['methods']['average']['ms'], 2)

    # host preparation: IBM decode of a SEG-Y file of 65536 traces, stable sort of the traces' bin ids
    with tempfile.TemporaryDirectory() as d:
        n = 65536
        S.write_segy(os.path.join(d, 'a.sgy'), rng.standard_normal((n, a.ns)).astype(np.float32), 0.25, fmt=1)
        t0 = time.perf_counter()
        f = S.SegyFile(os.path.join(d, 'a.sgy'))
        f.traces()
        dec = time.perf_counter() - t0
    bid = rng.integers(0, nb, ntr)
    t0 = time.perf_counter()
    np.argsort(bid, kind='stable')
    srt = time.perf_counter() - t0
    res['host'] = {'segy_ibm_decode_ms_per_65536_traces': round(dec * 1e3, 1), 'segy_decode_GBps': round(n * a.ns * 4 / dec / 1e9, 2),
                   f'stable_sort_ms_{ntr}_traces': round(srt * 1e3, 1)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
