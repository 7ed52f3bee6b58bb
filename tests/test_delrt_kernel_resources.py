"""The step-3 / step-4 kernels (csrc/p3d_delrt.hip) use no scratch memory, spill no register and stay within 64 VGPRs, read from the code object
on the CPU -- the pattern of test_static_kernel_resources.py: both kernels are memory-bound and read a handful of traces per workgroup, so
occupancy is what they live on, and an edit that costs it shows up in no functional test."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "delrt.o")
KERNELS = {"delrt_pad_kernel", "delrt_window_kernel"}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_delrt_kernels_use_no_scratch_and_spill_nothing():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen[short] = res
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
        assert res["vgpr_count"] <= 64, (short, res)             # 8 wavefronts per SIMD
    assert set(seen) == KERNELS, sorted(seen)
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
