"""The SEG-Y codec kernels (csrc/p3d_segy.hip) use no scratch memory, spill no register and stay within 64 VGPRs, read from the code object on the
CPU -- the pattern of test_delrt_kernel_resources.py: both kernels only move and recode words, so they live on occupancy; and the header tables
they take by value must stay in the kernel-argument segment, where a careless index would put them into scratch."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "segy.o")
KERNELS = {"segy_encode_kernel", "segy_decode_kernel"}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_segy_kernels_use_no_scratch_and_spill_nothing():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        full = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen.setdefault(re.sub(r"<.*>$", "", full), []).append(full)               # the instantiations of one template count as one kernel
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (full, res)
        assert res["vgpr_count"] <= 64, (full, res)             # 8 wavefronts per SIMD
    assert set(seen) == KERNELS, sorted(seen)
    assert len(seen["segy_encode_kernel"]) == 4 and len(seen["segy_decode_kernel"]) == 2, seen    # {trace, slice}-major x {4, 16}-byte stores; {4, 16}-byte
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
