"""The step-1 kernels (csrc/p3d_merge.hip) use no scratch memory, spill no register and stay within 64 VGPRs, read from the code object on the
CPU -- the pattern of test_segy_kernel_resources.py: both kernels only move and compare words, so they live on occupancy; and the table of word
widths (p3d_merge_words.hpp) must be folded into compares against constants, where a careless index would put it into scratch."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "merge.o")


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_merge_kernels_use_no_scratch_and_spill_nothing():
    seen = set()
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        full = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen.add(full)
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (full, res)
        assert res["vgpr_count"] <= 64, (full, res)             # 8 wavefronts per SIMD
    # keys: 4-byte aligned records or not; records: 16-, 4- and 1-byte units
    assert seen == {"merge_keys_kernel<true>", "merge_keys_kernel<false>", "merge_records_kernel<16>", "merge_records_kernel<4>", "merge_records_kernel<1>"}, sorted(seen)
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
