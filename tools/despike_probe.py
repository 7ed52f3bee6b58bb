"""The six detection cases of tools/despike_rate.py and nothing else, for a profiler (rocprofv3 --kernel-trace --stats, or --pmc):
mean / median / rms at w = 5 and 21 on a section of --ntr traces x --ns samples, --reps launches each.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/despike_probe.py"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pseudo_3d_interpolation_amd import _ffi  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--ntr', type=int, default=65536)
    p.add_argument('--ns', type=int, default=8192)
    p.add_argument('--reps', type=int, default=3)
    a = p.parse_args()
    sec = np.random.default_rng(0).standard_normal((a.ntr, a.ns), dtype=np.float32)
    dsec = _ffi.DeviceArray(sec.shape, np.float32).upload(sec)
    dmask, dcnt = _ffi.DeviceArray((a.ntr, (a.ns + 63) // 64), np.uint64), _ffi.DeviceArray((2, a.ntr), np.int32)
    for w in (5, 21):
        for mode in ('mean', 'median', 'rms'):
            for _ in range(a.reps):
                _ffi.despike_detect_dev(dsec.ptr, a.ntr, a.ns, w, mode, 4.0, a.ns, None, dmask.ptr, dcnt.ptr)
    for b in (dsec, dmask, dcnt):
        b.free()
    print('done')


if __name__ == '__main__':
    main()
