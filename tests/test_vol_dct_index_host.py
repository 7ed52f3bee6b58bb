"""csrc/p3d_vol_dct_index.hpp on the CPU (tests/csrc/test_vol_dct_index_host.cpp, a stand-alone program built with g++ and the address and
undefined-behaviour sanitizers; nothing is loaded into Python): for every 7-smooth n0 <= 1024 position <-> coefficient of the axis-0 cosine pass are inverse
permutations, the partner of a position is the position of (n0 - k) mod n0, the owners' pairs cover every position exactly once and the LDS size never
exceeds 163 840 bytes; for axis lengths 1 ... 40 the reorder / FFT / combine / split identities and the kernel's column program hold in double."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'pseudo-3d-interpolation_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'csrc', 'test_vol_dct_index_host.cpp')


def test_vol_dct_index_maps(tmp_path):
    exe = os.path.join(str(tmp_path), 'vol_dct_index_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, SRC, '-o', exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith('ALL OK'), res.stdout[-2000:] + res.stderr[-2000:]
