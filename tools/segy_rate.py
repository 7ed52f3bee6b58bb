"""SEG-Y codec rates on the GPU (steps 9 and 16): the encode kernel on a resident cube in both layouts and both sample formats, the decode kernel on
the records it wrote (formats 1 and 5), and a device-to-device hipMemcpy of the same number of OUTPUT bytes as the encode, all in one process;
and the host path the encode replaces (np.transpose + segy.ieee2ibm) on a slab of --host-inlines inlines.

Case (default): 1024 x 1024 traces x 512 samples float32 (2 GiB of samples, 2.23 GiB of records); the cube is a slab of 64 inlines of normal
deviates repeated along the inline axis.  Medians of --reps runs after a warm-up; the host path is timed once.  Bytes counted for a kernel: its
input read once and its output written once; for the copy: the output bytes read and written.  Every timed call ends with the entry's own
device synchronisation.  Prints one JSON document; no threshold is applied.

    python tools/segy_rate.py [--nil 1024 --nxl 1024 --ns 512 --reps 7 --host-inlines 64 --out profiles/segy_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402

COLUMNS = [(0, 4), (4, 4), (20, 4), (32, 2), (180, 4), (184, 4), (188, 4), (192, 4)]       # the eight per-trace words of step 16
FIELDS = [(4, 4, 1), (70, 2, 1), (72, 4, 1), (76, 4, 1), (108, 2, 1)]                      # the five words step 9 scrapes


def median_of(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nil', type=int, default=1024)
    p.add_argument('--nxl', type=int, default=1024)
    p.add_argument('--ns', type=int, default=512)
    p.add_argument('--reps', type=int, default=7)
    p.add_argument('--host-inlines', type=int, default=64)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    nil, nxl, ns = a.nil, a.nxl, a.ns
    ntr, reclen, slab_il = nil * nxl, 240 + 4 * ns, min(a.host_inlines, nil)
    rng = np.random.default_rng(0)
    slab = rng.standard_normal((slab_il * nxl, ns), dtype=np.float32)                      # trace-major [slab traces][ns]
    slab_t = np.ascontiguousarray(slab.T)                                                  # slice-major [ns][slab traces]
    values = rng.integers(-2**31, 2**31, (len(COLUMNS), ntr)).astype(np.int32)
    template = rng.integers(0, 256, 240, dtype=np.uint8)

    dtrace, dslice = _ffi.DeviceArray((ntr, ns), np.float32), _ffi.DeviceArray((ns, ntr), np.float32)
    drec, dcopy = _ffi.DeviceArray((ntr, reclen), np.uint8), _ffi.DeviceArray((ntr, reclen), np.uint8)
    dback, dwords = _ffi.DeviceArray((ntr, ns), np.float32), _ffi.DeviceArray((len(FIELDS), ntr), np.int32)
    dtmpl, dval = _ffi.DeviceArray((240,), np.uint8).upload(template), _ffi.DeviceArray(values.shape, np.int32).upload(values)
    row = np.empty((ns, ntr), np.float32)
    for first in range(0, nil, slab_il):                                                   # the slab repeated along the inline axis
        n = min(slab_il, nil - first) * nxl
        dtrace.upload(slab[:n], first * nxl)
        row[:, first * nxl:first * nxl + n] = slab_t[:, :n]
    dslice.upload(row)
    del row
    nin, nout = dtrace.nbytes, drec.nbytes

    res = {'case': dict(nil=nil, nxl=nxl, ns=ns, GiB_samples=round(nin / 2**30, 3), GiB_records=round(nout / 2**30, 3), reps=a.reps,
                        per_trace_columns=len(COLUMNS), scraped_words=len(FIELDS))}
    copy_s = median_of(lambda: dcopy.copy_from(drec), a.reps)
    res['d2d_copy_of_record_bytes'] = {'ms': round(copy_s * 1e3, 3), 'GBps_read_plus_write': round(2 * nout / copy_s / 1e9, 1)}
    first_ok = {}
    for layout, src in (('trace', dtrace), ('slice', dslice)):
        for fmt in (1, 5):
            s = median_of(lambda: _ffi.segy_encode_dev(src.ptr, ntr, ns, layout, fmt, dtmpl.ptr, COLUMNS, dval.ptr, drec.ptr), a.reps)
            res[f'encode_{layout}_major_format_{fmt}'] = {'ms': round(s * 1e3, 3), 'GBps_read_plus_write': round((nin + nout) / s / 1e9, 1),
                                                          'time_over_copy_time': round(s / copy_s, 3)}
            got = drec.download(0, 2)[:, 240:].copy().view('>u4')
            first_ok[f'{layout}_{fmt}'] = bool(np.array_equal(got, S.ieee2ibm(slab[:2]) if fmt == 1 else slab[:2].view(np.uint32)))
    for key in ('1', '5'):
        res[f'slice_over_trace_major_format_{key}'] = round(res[f'encode_slice_major_format_{key}']['ms'] / res[f'encode_trace_major_format_{key}']['ms'], 3)
    for fmt in (1, 5):
        _ffi.segy_encode_dev(dtrace.ptr, ntr, ns, 'trace', fmt, dtmpl.ptr, COLUMNS, dval.ptr, drec.ptr)
        s = median_of(lambda: _ffi.segy_decode_dev(drec.ptr, ntr, ns, fmt, FIELDS, dback.ptr, dwords.ptr), a.reps)
        res[f'decode_format_{fmt}'] = {'ms': round(s * 1e3, 3), 'GBps_read_plus_write': round((nin + nout + dwords.nbytes) / s / 1e9, 1),
                                       'time_over_copy_time': round(s / copy_s, 3)}
        back = dback.download(0, 2)
        first_ok[f'decode_{fmt}'] = bool(np.array_equal(back, S.ibm2ieee(S.ieee2ibm(slab[:2])) if fmt == 1 else slab[:2]))
    res['first_traces_correct'] = first_ok
    for b in (dtrace, dslice, drec, dcopy, dback, dwords, dtmpl, dval):
        b.free()

    t0 = time.perf_counter()
    host = S.ieee2ibm(np.ascontiguousarray(slab_t.T))                                      # what the kernel's LDS transpose and integer coding replace
    host_s = time.perf_counter() - t0
    per_sample = host_s / host.size
    res['host_transpose_and_ieee2ibm'] = {'inlines': slab_il, 'seconds': round(host_s, 3), 'MSamples_per_s': round(host.size / host_s / 1e6, 1),
                                          'seconds_for_the_whole_cube_at_this_rate': round(per_sample * ntr * ns, 1)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
