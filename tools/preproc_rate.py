"""Rate of the step-11 pre-processing kernels (p3d_pre_*_dev, p3d_preproc.hip) on a device-resident 512 x 1024 x 1024 float32
cube (2 GiB, 1 Mi traces of 512 samples): gain (curves + gpow + clips), balance rms, a 3-section and a 10-section Butterworth
sosfiltfilt, resample_poly down 2 and up 2, FFT resample down 2 and the envelope, next to p3d_time2freq_dev (complex, nfft = nt)
on the same cube.  Every entry point synchronises the device before it returns, so the wall time of a call is its device time
plus the upload of its small tables; the median of --reps calls after one warm-up call is reported, in ms and in GB/s of the
bytes per point each operation must move at least (against the 6.29 TB/s copy ceiling).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/preproc_rate.py --reps 2` for the per-kernel statistics.

    python tools/preproc_rate.py [--nt 512] [--ntr 1048576] [--reps 5] [--json out.json]
"""
import argparse

import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CEILING_GBS = 6290.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, default=512)
    ap.add_argument('--ntr', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from pseudo_3d_interpolation_amd import _ffi
    from pseudo_3d_interpolation_amd.functions import filter as F
    from pseudo_3d_interpolation_amd.functions import signal as S
    lib, chk, ptr = _ffi.lib(), _ffi.check, _ffi._ptr
    nt, ntr = a.nt, a.ntr
    npts = nt * ntr
    x = _ffi.DeviceArray((nt, ntr), np.float32)
    rng = np.random.default_rng(0)
    for r0 in range(0, nt, 64):
        x.upload(rng.standard_normal((min(64, nt - r0), ntr), dtype=np.float32), first=r0)
    out = _ffi.DeviceArray((2 * nt, ntr), np.float32)
    ref = _ffi.DeviceArray((ntr,), np.float32)
    work = _ffi.DeviceArray((4 * nt * ntr,), np.float32)        # 16 B/pt: two complex64 lines, or the filter's extension (doubles above 8 sections)
    twt = np.arange(nt) * 0.0005
    prm, curves = S.gain_tables(nt, twt, tpow=2.0, epow=0.5, gpow=0.5, clip=2.0, pclip=1.5, nclip=-1.5)

    def filt(freqs, fs, ft):
        _, _, sos = F.design_filter(freqs, fs, ft)
        zi, pad = F.sosfilt_zi(sos), F.sos_padlen(sos)
        return sos.shape[0], (lambda: chk(lib.p3d_pre_sosfiltfilt_dev(0, x.ptr, nt, ntr, sos.shape[0], ptr(sos), ptr(zi), pad, out.ptr, work.ptr)))

    def poly(up, down):
        op = S.resample_poly_op(nt, up, down, 'hann')
        h = np.ascontiguousarray(op[1])
        return op[5], (lambda: chk(lib.p3d_pre_upfirdn_dev(0, x.ptr, nt, ntr, ptr(h), h.size, op[2], op[3], op[4], op[5], out.ptr)))

    def spectral(op):
        src, fac = np.ascontiguousarray(op[2], np.int32), np.ascontiguousarray(op[3], np.float32)
        return (lambda: chk(lib.p3d_pre_spectral_dev(0, x.ptr, nt, ntr, op[1], ptr(src), ptr(fac), int(op[4]), op[5], op[6], out.ptr,
                                                     work.ptr)))

    ns3, f3 = filt([50, 100, 600, 900], 2000.0, 'bandpass')
    ns10, f10 = filt([200, 215], 1000.0, 'lowpass')
    nd2, pd2 = poly(1, 2)
    nu2, pu2 = poly(2, 1)
    tf_out = _ffi.DeviceArray((nt, ntr), np.complex64)
    cases = [
        ('gain (tpow, epow, gpow, clip, pclip, nclip)', 8, 1.0,
         lambda: chk(lib.p3d_pre_gain_dev(0, x.ptr, nt, ntr, ptr(prm), ptr(curves), out.ptr, work.ptr))),
        ('balance rms', 12, 1.5, lambda: chk(lib.p3d_pre_balance_dev(0, x.ptr, nt, ntr, 0, out.ptr, ref.ptr))),
        (f'sosfiltfilt {ns3} sections', 16, 3.0, f3),
        (f'sosfiltfilt {ns10} sections', 12 + 16 + 16 + 12, None, f10),      # two groups, the signal between them in double
        ('resample_poly down 2', 4 + 2, 1.0, pd2),
        ('resample_poly up 2', 4 + 8, None, pu2),
        ('resample (FFT) down 2', 4 + 2, None, spectral(S.resample_op(nt, nt // 2, 'hann'))),
        ('envelope', 8, None, spectral(S.envelope_op(nt))),
        ('time2freq_dev (complex, nfft = nt)', 12, None,
         lambda: chk(lib.p3d_time2freq_dev(0, x.ptr, nt, ntr, 0.0005, 0.0, nt, 0, None, tf_out.ptr))),
    ]
    rows = []
    for name, bpp, bar, fn in cases:
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(ts)
        gbs = bpp * npts / (ms * 1e-3) / 1e9
        rows.append(dict(op=name, ms=round(ms, 3), bytes_per_point=bpp, GBps=round(gbs, 1), of_ceiling=round(gbs / CEILING_GBS, 3),
                         bar_ms=bar))
        print(f'{name:45s} {ms:9.3f} ms  {bpp:3d} B/pt  {gbs:8.1f} GB/s  {100 * gbs / CEILING_GBS:5.1f} %  bar {bar}', flush=True)
    env = next(r for r in rows if r['op'] == 'envelope')['ms']
    t2f = rows[-1]['ms']
    print(f'envelope / time2freq_dev = {env / t2f:.2f} (bar 2.5)')
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(dict(nt=nt, ntraces=ntr, reps=a.reps, rows=rows, envelope_over_time2freq=round(env / t2f, 3)), f, indent=1)



if __name__ == '__main__':
    main()
