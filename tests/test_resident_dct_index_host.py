"""csrc/p3d_resident_dct_index.hpp on the CPU (tests/csrc/test_resident_dct_index_host.cpp, a stand-alone program built with g++ and the address and
undefined-behaviour sanitizers): for the eight routed window shapes the reordered position <-> natural sample map is a bijection consistent with ``perm``,
the mask-bit lookup returns ``mask[i][j]`` of a mask packed as ``patch_pack_kernel`` packs it, the thread slots partition the N1 x N2 coefficients (each is
stored exactly once), and the group step as the kernel writes it is the DCT-II / its inverse in double precision."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'pseudo-3d-interpolation_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'csrc', 'test_resident_dct_index_host.cpp')


def test_resident_dct_index_maps(tmp_path):
    exe = os.path.join(str(tmp_path), 'resident_dct_index_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, SRC, '-o', exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith('ALL OK'), res.stdout[-2000:] + res.stderr[-2000:]
