"""The kernels of the 3-D DCT volume loop (csrc/p3d_vol_dct.hip) use no scratch memory, spill no register and keep the register counts DESIGN.md section
3.19.2 records, read from the code object on the CPU -- the pattern of test_vol64_kernel_resources.py.  Four 256-thread workgroups of the axis-0 pass share a
compute unit where the tile allows it, which takes no more than 128 vector registers.  Register and scratch figures only: no instruction is inspected."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "vol_dct.o")
# DESIGN.md section 3.19.2, "Registers": vector registers per kernel
VGPRS = {"voldct_z_kernel": 46, "voldct_update_kernel": 40, "voldct_fold_kernel": 18}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_vol_dct_kernels_use_no_scratch_and_keep_their_registers():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        full = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("p3d::", "")).replace("void ", "")
        seen[full] = res["vgpr_count"]
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (full, res)
    assert seen == VGPRS, sorted(seen.items())
    assert seen["voldct_z_kernel"] <= 128
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
    design = open(os.path.join(os.path.dirname(BUILD), "..", "..", "DESIGN.md"), encoding="utf-8").read()
    for kernel, n in VGPRS.items():
        assert f"`{kernel}` {n}" in design, (kernel, n)
