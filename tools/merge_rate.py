"""Step-1 call times on the GPU: the keys entry and the records entry (csrc/p3d_merge.hip) on a resident group of records, and a
device-to-device hipMemcpy of the same number of OUTPUT bytes, all in one process.

Cases (default): --traces records (200 000) of 2048 float32 samples (8432 bytes: 16-byte units), of 2047 float32 samples (8428 bytes: 4-byte units)
and of 2047 int16 samples (4334 bytes: single bytes; a quarter of the records, the path is slow).  The group is a slab of 4096 records of random
bytes repeated, TRACE_SEQUENCE_LINE counting up with one number in 1000 left out (a gap trace each) and one record in 997 repeated with another
TRACE_SEQUENCE_FILE (dropped).  The plan is made on the host from the keys the kernel returned, as `functions.merge.merge_segys` makes it.

Medians of --reps calls after two warm-up calls.  The figures are CALL times, not kernel times: a host clock around one `_dev` entry, which ends in
its own device synchronisation; the records entry also allocates, uploads (three ints per output row) and frees its plan inside the timed call.
The kernels' own times come from `rocprofv3 --kernel-trace --stats -- python tools/merge_rate.py --reps 5` (profiles/merge_kernel_stats.csv).  Bytes counted: keys -- 240 header bytes read and 20 bytes written per record
(the keys kernel touches whole cache lines of a record it strides over, so this is a lower bound of its traffic); records and copy -- the output
bytes read and written.  Prints one JSON document; no threshold is applied.

    python tools/merge_rate.py [--traces 200000 --reps 15 --out profiles/merge_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd.functions import merge as M  # noqa: E402

SLAB = 4096


def median_of(fn, reps, warmup=2):
    ts = []
    for _ in range(reps + warmup):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[warmup:])), float(np.min(ts[warmup:])), float(np.max(ts[warmup:]))


def run_case(n, reclen, reps, rng):
    slab = rng.integers(0, 256, (SLAB, reclen), dtype=np.uint8)
    line = np.arange(n, dtype=np.int64) + 1
    line += np.arange(n) // 1000                                                           # one number in 1000 is missing
    repeated = np.arange(997, n, 997)
    repeated = repeated[repeated % SLAB != 0]                                              # the record before lies in the same chunk
    line[repeated] = line[repeated - 1]
    drec = _ffi.DeviceArray((n, reclen), np.uint8)
    for first in range(0, n, SLAB):
        count = min(SLAB, n - first)
        chunk = slab[:count].copy()
        chunk[:, :4] = line[first:first + count].astype('>i4').view(np.uint8).reshape(count, 4)
        chunk[:, 4:8] = np.arange(first, first + count).astype('>i4').view(np.uint8).reshape(count, 4)
        at = repeated[(repeated >= first) & (repeated < first + count)] - first
        chunk[at, 8:240] = chunk[at - 1, 8:240]                                            # the header of the record before, another TRACE_SEQUENCE_FILE
        drec.upload(chunk, first)
    dtracl, dfull, dsub = (_ffi.DeviceArray((n,), dt) for dt in (np.int32, np.uint64, np.uint64))
    keys_s = median_of(lambda: _ffi.merge_keys_dev(drec.ptr, n, reclen, dtracl.ptr, dfull.ptr, dsub.ptr), reps)
    tracl, full, sub = dtracl.download(), dfull.download(), dsub.download()
    headers = drec.download()[:, :240]
    t0 = time.perf_counter()
    overlapping, internal = M.duplicate_masks(headers, full, sub)
    src, lo_row, hi_row = M.merge_plan(tracl, overlapping | internal)
    host_s = time.perf_counter() - t0
    nout = src.size
    dout, dcopy = _ffi.DeviceArray((nout, reclen), np.uint8), _ffi.DeviceArray((nout, reclen), np.uint8)
    copy_s = median_of(lambda: dcopy.copy_from(dout), reps)
    rec_s = median_of(lambda: _ffi.merge_records_dev(drec.ptr, n, reclen, src, lo_row, hi_row, dout.ptr), reps)
    rows = np.flatnonzero(src >= 0)[[0, 1, -1]]
    ok = all(np.array_equal(np.delete(dout.download(int(r), 1)[0], np.s_[4:8]), np.delete(drec.download(int(src[r]), 1)[0], np.s_[4:8])) for r in rows)
    gap = int(np.flatnonzero(src < 0)[0])
    got = dout.download(gap, 1)[0]
    ok = ok and not got[240:].any() and int(got[4:8].view('>i4')[0]) == gap + 1 and int(got[:4].view('>i4')[0]) == int(tracl[src[0]]) + gap
    nbytes = nout * reclen
    for b in (drec, dtracl, dfull, dsub, dout, dcopy):
        b.free()

    def entry(t, moved):
        return {'ms': round(t[0] * 1e3, 3), 'ms_min_max': [round(t[1] * 1e3, 3), round(t[2] * 1e3, 3)], 'GBps': round(moved / t[0] / 1e9, 1)}
    res = {'records_in': n, 'record_bytes': reclen, 'rows_out': int(nout), 'gap_rows': int(np.count_nonzero(src < 0)),
           'dropped': int(np.count_nonzero(overlapping | internal)), 'GiB_out': round(nbytes / 2**30, 3),
           'keys_call': entry(keys_s, n * 260), 'host_masks_and_plan_ms': round(host_s * 1e3, 1),
           'd2d_copy_of_output_bytes': entry(copy_s, 2 * nbytes), 'records_call': entry(rec_s, 2 * nbytes),
           'records_call_time_over_copy_time': round(rec_s[0] / copy_s[0], 3), 'spot_checks_correct': bool(ok)}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--traces', type=int, default=200000)
    p.add_argument('--reps', type=int, default=15)
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    rng = np.random.default_rng(0)
    res = {'reps': a.reps,
           'units_of_16_bytes_2048_float32_samples': run_case(a.traces, 240 + 4 * 2048, a.reps, rng),
           'units_of_4_bytes_2047_float32_samples': run_case(a.traces, 240 + 4 * 2047, a.reps, rng),
           'single_bytes_2047_int16_samples': run_case(max(a.traces // 4, 2000), 240 + 2 * 2047, a.reps, rng)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
