"""Step-4 padding rate on the GPU: the pad kernel alone on a resident section (device buffers) against a device-to-device hipMemcpy of the same
number of OUTPUT bytes, timed in the same process.

Case (default): 20000 traces x 4000 samples float32 padded to 6000 samples (305 MiB read, 458 MiB written), the traces in runs of equal top padding
as a profile recorded in window mode has them; medians of --reps runs after a warm-up.  Bytes counted for the kernel: the input section read once
and the output section written once; for the copy: the output bytes read and written.  Prints one JSON document; no threshold is applied.

    python tools/delrt_rate.py [--ntr 20000 --ns 4000 --ns-out 6000 --reps 7 --out profiles/delrt_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402


def median_of(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--ntr', type=int, default=20000)
    p.add_argument('--ns', type=int, default=4000)
    p.add_argument('--ns-out', type=int, default=6000)
    p.add_argument('--reps', type=int, default=7)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    ntr, ns, ns_out = a.ntr, a.ns, a.ns_out
    rng = np.random.default_rng(0)
    sec = rng.standard_normal((ntr, ns), dtype=np.float32)
    runs = rng.integers(0, ns_out - ns + 1, max(ntr // 500, 1))                 # runs of 500 traces with one delay each, any residue mod 4
    top = np.resize(np.repeat(runs, 500), ntr).astype(np.int32)
    din, dtop = _ffi.DeviceArray(sec.shape, np.float32).upload(sec), _ffi.DeviceArray((ntr,), np.int32).upload(top)
    dout, dcopy = _ffi.DeviceArray((ntr, ns_out), np.float32), _ffi.DeviceArray((ntr, ns_out), np.float32)
    nin, nout = sec.nbytes, dout.nbytes
    copy_s = median_of(lambda: dcopy.copy_from(dout), a.reps)
    pad_s = median_of(lambda: _ffi.delrt_pad_dev(din.ptr, ntr, ns, ns_out, dtop.ptr, dout.ptr), a.reps)
    check = dout.download(0, 4)
    want = np.zeros((4, ns_out), np.float32)
    for x in range(4):
        want[x, top[x]:top[x] + ns] = sec[x]
    for b in (din, dtop, dout, dcopy):
        b.free()
    res = {'case': dict(ntr=ntr, ns_in=ns, ns_out=ns_out, MiB_in=round(nin / 2**20, 1), MiB_out=round(nout / 2**20, 1), reps=a.reps,
                        top_residues_mod_4=sorted(set((top % 4).tolist()))),
           'd2d_copy_of_output_bytes': {'ms': round(copy_s * 1e3, 4), 'GBps_read_plus_write': round(2 * nout / copy_s / 1e9, 1)},
           'pad_kernel': {'ms': round(pad_s * 1e3, 4), 'GBps_read_plus_write': round((nin + nout) / pad_s / 1e9, 1), 'includes': 'the copy of top[] to the host for the check'},
           'pad_time_over_copy_time': round(pad_s / copy_s, 3), 'first_traces_correct': bool(check.tobytes() == want.tobytes())}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
