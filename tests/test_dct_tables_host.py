"""csrc/p3d_dct_tables.hpp on the CPU (tests/csrc/test_dct_tables_host.cpp, a stand-alone program built with g++): the coefficient tables against their
closed forms, the even/odd reordering, the groups of the group pass covering every coefficient exactly once for N = 1 ... 40 (even and odd, in one
and in two dimensions), and the DCT identities themselves in double precision."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'pseudo-3d-interpolation_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'csrc', 'test_dct_tables_host.cpp')


def test_dct_tables_and_group_indexing(tmp_path):
    exe = os.path.join(str(tmp_path), 'dct_tables_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-ffp-contract=off', '-I', CSRC, SRC, '-o', exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith('ALL OK'), res.stdout[-2000:] + res.stderr[-2000:]
