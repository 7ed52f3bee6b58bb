"""The step-8 kernels (csrc/p3d_despike.hip) use no scratch memory and spill no register, read from the code object on the CPU -- the
pattern of test_kernel_resources.py, for the new unit: the sliding windows and the sorting network live in registers that are only ever
indexed by compile-time constants, and an edit that breaks this shows up in no functional test."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM, _kernels

OBJ = os.path.join(BUILD, "despike.o")


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_despike_kernels_use_no_scratch():
    seen = {}
    for mangled, res in _kernels(OBJ).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        seen[short] = res
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
        assert res["vgpr_count"] <= 128, (short, res)            # at least 4 wavefronts per SIMD
    detect = {s for s in seen if s.startswith("despike_detect_kernel<")}
    assert detect == {f"despike_detect_kernel<{w}, {m}>" for w in range(3, 32, 2) for m in range(3)}, sorted(detect)
    assert {"despike_count_kernel", "despike_replace_kernel"} <= set(seen)


def _sgpr_spills(obj):
    """mangled name -> .sgpr_spill_count of the gfx950 code object (scalar registers parked in lanes of a vector register: no memory traffic)."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "f.fatbin"), os.path.join(d, "f.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", obj], check=True, capture_output=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    return {re.search(r"\.name:\s+(\S+)", blk).group(1): int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
            for blk in notes.split("- .agpr_count")[1:]}


@pytest.mark.skipif(not os.path.isfile(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the object files of the library build")
def test_scalar_register_spills_are_the_known_ones():
    """The hot kernels (detection, counts) park no scalar register.  The replacement kernel does: its run-time predicates over the 32-value
    neighbour window (k < n, k == rank) are wave-uniform and outnumber the scalar registers, so the compiler keeps some of them in lanes of
    a vector register (still no scratch memory, checked above).  It runs for 0.03 - 0.07 ms on a whole section, so this is accepted; the
    bound keeps it from growing unnoticed."""
    for mangled, n in _sgpr_spills(OBJ).items():
        if "despike_replace_kernel" in mangled:
            assert n <= 400, (mangled, n)
        else:
            assert n == 0, (mangled, n)
