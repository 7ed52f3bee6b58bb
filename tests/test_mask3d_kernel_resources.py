"""The kernels that gained the mask slice stride (P3D_FLAG_MASK_PER_SLICE) use no scratch memory, spill no register and keep the register class
their occupancy rests on -- read from the code objects on the CPU, the pattern of test_dct_kernel_resources.py.  The seven update kernels are bound
by memory and run at 8 wavefronts per SIMD (at most 64 registers); the stride is one more scalar in their address arithmetic.  The fused
double-precision row passes (row64_kernel; mix64::row_kernel on the register engine) read the mask with the same stride: row64_kernel keeps the 128
registers of test_kernel_resources.py's OCCUPANCY table, the register-engine row passes spill nothing."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import BUILD, LLVM, _kernels

# object file -> {kernel (demangled, without arguments): most registers it may use}
BUDGET = {
    "generic.o": {"gen_update_kernel": 64},
    "dct.o": {"dct_update_kernel": 64},
    "wavelet.o": {"wupdate_kernel<float>": 64, "wupdate_kernel<c32>": 64},
    "shearlet.o": {"supdate_kernel": 64},
    "f64.o": {"update64_kernel": 64, "row64_kernel<0, false>": 128, "row64_kernel<0, true>": 128, "row64_kernel<1, false>": 128, "row64_kernel<1, true>": 128,
              "row64_kernel<2, false>": 128, "row64_kernel<2, true>": 128},
    "wavelet64.o": {"wupdate64_kernel<double>": 64, "wupdate64_kernel<c64>": 64},
    "shearlet64.o": {"supdate64_kernel": 64},
}
TOOLS = os.path.exists(f"{LLVM}/clang-offload-bundler") and shutil.which("c++filt")


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("p3d::", "")).replace("void ", "")


@pytest.mark.skipif(not all(os.path.isfile(os.path.join(BUILD, o)) for o in BUDGET) or not TOOLS,
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
@pytest.mark.parametrize("obj", sorted(BUDGET))
def test_kernels_with_the_mask_stride_use_no_scratch_and_keep_their_register_class(obj):
    seen = {}
    for mangled, res in _kernels(os.path.join(BUILD, obj)).items():
        short = _short(mangled)
        if short in BUDGET[obj]:
            seen[short] = res
    assert set(seen) == set(BUDGET[obj]), sorted(set(BUDGET[obj]) - set(seen))
    for short, res in seen.items():
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
        assert res["vgpr_count"] <= BUDGET[obj][short], (short, res)


@pytest.mark.skipif(not all(os.path.isfile(os.path.join(BUILD, f"mix64_{i}.o")) for i in range(8)) or not TOOLS,
                    reason="needs the object files of the library build and the ROCm LLVM tools")
def test_register_engine_row_passes_use_no_scratch():
    n = tight = 0
    for i in range(8):
        for mangled, res in _kernels(os.path.join(BUILD, f"mix64_{i}.o")).items():
            short = _short(mangled)
            if short.startswith("mix64::row_kernel<"):
                n += 1
                assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (short, res)
                # rows of 280, 300 and 360 points: 140 threads and 31 ... 40 KiB of LDS per workgroup, five / four workgroups per CU -- four wavefronts
                # per SIMD, which 128 registers allow and 136 (what the slice offset as a product s * mask_stride cost these three plans) do not
                if re.match(r"mix64::row_kernel<mix::MixPlan<(280|300|360),", short):
                    tight += 1
                    assert res["vgpr_count"] <= 128, (short, res)
                # rows of 448 points: the one plan the stride moved across a register class (64 -> 66 registers, allocated as 72: 7 wavefronts per SIMD by
                # registers instead of 8).  LDS binds it first: a workgroup is two rows = 128 threads = 2 wavefronts on 14 KiB of LDS (16 B x 448 x 2), so at
                # most 11 workgroups = 22 wavefronts per CU = 5.5 per SIMD fit the 160 KiB -- occupancy is lost only beyond 72 registers (512 / 7 = 73)
                if re.match(r"mix64::row_kernel<mix::MixPlan<448,", short):
                    tight += 1
                    assert res["vgpr_count"] <= 72, (short, res)
    assert n > 150 and tight == 4   # (every planned length was looked at)
