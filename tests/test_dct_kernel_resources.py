"""The DCT kernels (csrc/p3d_dct.hip) use no scratch memory and spill no register, read from the code object on the CPU -- the pattern of
test_merge_kernel_resources.py.  The group pass holds four coefficients, eight table entries and the threshold in registers and is bound by
memory; a spill would add traffic to the one pass the DCT loop has over the FFT loop's threshold pass."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "dct.o")


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_dct_kernels_use_no_scratch_and_spill_nothing():
    seen = set()
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        full = re.sub(r"\(.*$", "", name.replace("p3d::", "")).replace("void ", "")
        seen.add(full)
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (full, res)
        assert res["vgpr_count"] <= 64, (full, res)             # 8 wavefronts per SIMD
    # the group pass: fused, combine only, split only, threshold + split
    assert seen == {"dct_group_kernel<0>", "dct_group_kernel<1>", "dct_group_kernel<2>", "dct_group_kernel<3>", "dct_update_kernel"}, sorted(seen)
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
