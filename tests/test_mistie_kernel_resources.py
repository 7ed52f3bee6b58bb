"""The step-7 kernels (csrc/p3d_mistie.hip) use no scratch memory and spill no register, read from the code object on the CPU -- the pattern
of test_static_kernel_resources.py: the segment test returns its (up to two) points in named registers, never in an indexed array, and an
edit that breaks this shows up in no functional test."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "mistie.o")
KERNELS = {"mistie_tilebox_kernel", "mistie_cross_kernel", "mistie_nearest_kernel", "mistie_xcorr_kernel<true>", "mistie_xcorr_kernel<false>"}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_mistie_kernels_use_no_scratch_and_spill_nothing():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen[short] = res
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
        assert res["vgpr_count"] <= 128, (short, res)            # double arithmetic: 4 wavefronts per SIMD at the least
    assert set(seen) == KERNELS, sorted(seen)
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
