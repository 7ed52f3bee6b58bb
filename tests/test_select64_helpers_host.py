"""The plain-C++ helpers of the double-precision order statistics on the CPU (tests/csrc/test_select64_host.cpp, a stand-alone program built as host
code): the order-preserving 64-bit key of a double and its inverse (-0.0 and +0.0 share a key), the key of a modulus, np.percentile's rank with a
double weight beside the float one, and NumPy's two-branch interpolation, against literals from np.percentile."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'pseudo-3d-interpolation_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'csrc', 'test_select64_host.cpp')


def test_select64_host_helpers(tmp_path):
    exe = os.path.join(str(tmp_path), 'select64_host')
    # -ffp-contract=off as the unit itself is built: the interpolation rounds its product and its sum separately
    subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off',
                    '-I', CSRC, '-I', os.path.join(ROOT, 'include'), SRC, '-o', exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith('ALL OK'), res.stdout[-2000:] + res.stderr[-2000:]
