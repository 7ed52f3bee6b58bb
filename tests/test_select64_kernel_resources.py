"""The kernels of the double-precision order statistics (csrc/p3d_select64.hip) use no scratch memory, spill no register and keep the register counts
DESIGN.md section 3.3.1 records, read from the code object on the CPU -- the pattern of test_dct64_kernel_resources.py.  The scatter pass of the sort
holds a thread's sixteen 128-bit keys and their ranks in registers: an array indexed at run time there would go to scratch."""
import os
import re
import shutil
import subprocess

import pytest

from test_despike_kernel_resources import _sgpr_spills
from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "select64.o")
# DESIGN.md section 3.3.1, "Registers": vector registers per kernel
VGPRS = {"sel64::pct64_mod_kernel": 24, "sel64::pct64_hist_kernel": 12, "sel64::pct64_scan_kernel": 34, "sel64::pct64_succ_kernel": 10,
         "sel64::pct64_tau_kernel": 12, "sel64::lex_keys64_kernel": 14, "sel64::sort64_hist_kernel": 8, "sel64::sort64_scan_kernel": 42,
         "sel64::sort64_scatter_kernel": 101, "sel64::peaks64_kernel": 11, "sel64::pick64_kernel": 22}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_select64_kernels_use_no_scratch_and_keep_their_registers():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        full = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("p3d::", "")).replace("void ", "")
        seen[full] = res["vgpr_count"]
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (full, res)
    assert seen == VGPRS, sorted(seen.items())
    assert all(n == 0 for n in _sgpr_spills(OBJ).values())
    design = open(os.path.join(os.path.dirname(BUILD), "..", "..", "DESIGN.md"), encoding="utf-8").read()
    for kernel, n in VGPRS.items():
        assert f"`{kernel.split('::')[1]}` {n}" in design, (kernel, n)
