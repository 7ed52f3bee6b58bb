"""Step-8 despiking rate on the GPU: detection (p3d_despike_detect_dev) per mode and window, replacement, and host array to host array,
against the device-to-device copy of the same buffer measured in the same run.

Case (default): a section of 65536 traces x 8192 samples float32 (2 GiB), 0.1 % of the traces carrying one burst of 400 samples, time window
of 1024 samples.  Bytes counted for detection: the section read once.  The NumPy restatement (tests/helpers/despike_numpy.py) is timed on a
slice of 4096 traces of the same section.  Prints one JSON document.

    python tools/despike_rate.py [--ntr 65536 --ns 8192 --reps 3 --cpu-traces 4096 --out profiles/despike_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import despike_numpy as H  # noqa: E402
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import despike as D  # noqa: E402

THRESHOLD = {'mean': 3.0, 'median': 6.0, 'rms': 3.0}   # detection timing (the kernel's time does not depend on the outcome)
E2E = {'mode': 'mean', 'threshold': 4.0}


def best_of(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts[1:])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--ntr', type=int, default=65536)
    p.add_argument('--ns', type=int, default=8192)
    p.add_argument('--window', type=int, default=1024)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--cpu-traces', type=int, default=4096)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    rng = np.random.default_rng(0)
    ntr, ns = a.ntr, a.ns
    sec = rng.standard_normal((ntr, ns), dtype=np.float32)
    spiky = np.sort(rng.choice(np.arange(16, ntr - 16), max(1, ntr // 1000), replace=False))
    for x in spiky:
        r0 = int(rng.integers(0, ns - 400))
        sec[x, r0:r0 + 400] = (60.0 * (1 + 0.1 * rng.random(400)) * rng.choice([-1.0, 1.0], 400)).astype(np.float32)
    M, dy, main_end, add_start = D.window_rows(ns, a.window, 1.0, 10)
    nbytes = sec.nbytes
    res = {'case': dict(ntr=ntr, ns=ns, window_samples=M, spiky_traces=int(spiky.size), GiB=round(nbytes / 2**30, 3)), 'detect': {}}
    dsec, dcopy = _ffi.DeviceArray(sec.shape, np.float32).upload(sec), _ffi.DeviceArray(sec.shape, np.float32)
    dmask, dcnt = _ffi.DeviceArray((ntr, (ns + 63) // 64), np.uint64), _ffi.DeviceArray((2, ntr), np.int32)
    t = best_of(lambda: dcopy.copy_from(dsec), a.reps)
    res['d2d_copy'] = {'ms': round(t * 1e3, 3), 'GBps_read_plus_write': round(2 * nbytes / t / 1e9, 1)}
    for w in (5, 21):
        for mode in ('mean', 'median', 'rms'):
            t = best_of(lambda: _ffi.despike_detect_dev(dsec.ptr, ntr, ns, w, mode, THRESHOLD[mode], main_end, add_start, dmask.ptr, dcnt.ptr), a.reps)
            res['detect'][f'{mode}_w{w}'] = {'ms': round(t * 1e3, 3), 'GBps': round(nbytes / t / 1e9, 1),
                                             'time_over_d2d_copy': round(t / (res['d2d_copy']['ms'] / 1e3), 2)}
    res['median_over_mean_w21'] = round(res['detect']['median_w21']['ms'] / res['detect']['mean_w21']['ms'], 2)
    # replacement and host-to-host: mean over 5 traces at threshold 4, where Gaussian noise alone leaves no trace above the count filter
    # (median at threshold 6 flags 3.4 % of pure noise and nearly every trace passes the filter: not the isolated-spike case)
    mode, thr = E2E['mode'], E2E['threshold']
    _ffi.despike_detect_dev(dsec.ptr, ntr, ns, 5, mode, thr, main_end, add_start, dmask.ptr, dcnt.ptr)
    t0 = time.perf_counter()
    mask, counts = dmask.download(), dcnt.download()
    t1 = time.perf_counter()
    rec = D.spikes_from_mask(mask, counts, ns, M, main_end, add_start, 5)
    t2 = time.perf_counter()
    ordered, level_start = D.order_by_level(rec, D.assign_levels(rec))
    t3 = time.perf_counter()
    res['host'] = {'mask_and_counts_download_ms': round((t1 - t0) * 1e3, 1), 'runs_from_mask_ms': round((t2 - t1) * 1e3, 1),
                   'levels_ms': round((t3 - t2) * 1e3, 1), 'traces_past_count_filter': int((counts > M * 0.1).any(axis=0).sum()),
                   'candidate_fraction': round(float(counts.sum()) / sec.size, 6)}
    res['spikes'] = int(rec.shape[0])
    res['levels'] = int(level_start.size - 1)
    res['replace'] = {}
    for out in ('scaled', 'threshold', 'median', 'zeros'):
        t = best_of(lambda: _ffi.despike_replace_dev(dcopy.ptr, ntr, ns, ordered, level_start, mode, out, thr), a.reps)
        res['replace'][out] = {'ms': round(t * 1e3, 3)}
    t = best_of(lambda: dsec.upload(sec), 1)
    res['upload'] = {'ms': round(t * 1e3, 1), 'GBps': round(nbytes / t / 1e9, 2)}
    t = best_of(lambda: dsec.download(), 1)
    res['download'] = {'ms': round(t * 1e3, 1), 'GBps': round(nbytes / t / 1e9, 2)}
    for b in (dsec, dcopy, dmask, dcnt):
        b.free()
    kw = dict(window=a.window, dt=1.0, overlap=10, ntraces=5, out='threshold', **E2E)
    t = best_of(lambda: D.despike_2D(sec, trace_major=True, **kw), 1)
    res['host_to_host'] = {'ms': round(t * 1e3, 1), 'GBps': round(nbytes / t / 1e9, 2), 'ns_per_sample': round(t / sec.size * 1e9, 4), **E2E}
    n = min(a.cpu_traces, ntr)
    part = np.ascontiguousarray(sec[:n].T)
    t0 = time.perf_counter()
    H.despike_2D(part, **kw)
    t = time.perf_counter() - t0
    res['numpy_helper'] = {'traces': n, 's': round(t, 2), 'ns_per_sample': round(t / part.size * 1e9, 2),
                           'per_sample_over_gpu_host_to_host': round(t / part.size * 1e9 / res['host_to_host']['ns_per_sample'], 1)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
