"""The single-kernel DCT loop of the windowed jobs (``resident_dct_kernel<N1, N2, OP>`` in patch_dct.o): 3 operators x 8 routed window shapes, no scratch
memory, no spilled register, and at most 256 vector registers -- the largest workgroup has 512 threads, two wavefronts per SIMD (128 should an
instantiation ever have 1024 threads).  Read from the code object on the CPU, the pattern of test_patch_kernel_resources.py."""
import os
import re
import shutil

import pytest

from test_kernel_resources import BUILD, LLVM, _kernels
from test_mask3d_kernel_resources import _short

TOOLS = os.path.exists(f"{LLVM}/clang-offload-bundler") and shutil.which("c++filt")
needs_objects = pytest.mark.skipif(not os.path.isfile(os.path.join(BUILD, "patch_dct.o")) or not TOOLS,
                                   reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")

ROUTED = [(32, 32), (32, 64), (64, 32), (64, 64), (32, 128), (128, 32), (64, 128), (128, 64)]


@needs_objects
def test_resident_dct_kernels_use_no_scratch_and_fit_their_registers():
    k = {_short(m): res for m, res in _kernels(os.path.join(BUILD, "patch_dct.o")).items()}
    assert set(k) == {f"resident_dct_kernel<{n1}, {n2}, {op}>" for n1, n2 in ROUTED for op in range(3)}, sorted(k)
    for name, res in k.items():
        n1, n2 = map(int, re.match(r"resident_dct_kernel<(\d+), (\d+),", name).groups())
        threads = n1 * n2 // 16
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)
        assert res["vgpr_count"] <= (128 if threads > 512 else 256), (name, res)


@needs_objects
def test_the_units_of_the_fft_loops_hold_no_dct_kernel():
    """patch.o and resident.o keep their code: the DCT loop is a unit of its own."""
    for obj in ("patch.o", "resident.o"):
        assert not [n for n in map(_short, _kernels(os.path.join(BUILD, obj))) if "dct" in n]
