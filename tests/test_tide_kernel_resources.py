"""The step-6 kernel (csrc/p3d_tide.hip) uses no scratch memory and spills no register, read from the code object on the CPU -- the pattern of
test_reproject_kernel_resources.py.  The kernel selects the nodal factors of a constituent by its id inside a loop whose trip count is an
argument; an array of factors indexed by that id would live in private memory, which shows up in no functional test."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "tide.o")
KERNELS = {"tide_predict_kernel"}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_tide_kernel_uses_no_scratch_and_spills_nothing():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen[short] = res
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
        assert res["vgpr_count"] <= 128, (short, res)             # 4 wavefronts per SIMD at least
    assert set(seen) == KERNELS, sorted(seen)
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
