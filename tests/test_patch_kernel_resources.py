"""The kernels of the windowed loop use no scratch memory and spill no register, the single-kernel loop with one mask per window stays within the register
class of the shared-mask instantiation of the same shape, and the shared-mask instantiations (resident.o) have exactly the register counts they had before the
kernel template moved into p3d_resident_job.hpp -- read from the code objects on the CPU, the pattern of test_mask3d_kernel_resources.py.

PARENT: ``vgpr_count`` of every ``resident_kernel<N1, N2, OP>`` in resident.o of the commit before the windowed loop (same compiler, same flags).  The
per-window-mask instantiations are ``resident_kernel<N1, N2, OP | 4>`` in patch.o (RESIDENT_MASK_PER_JOB = 4)."""
import os
import re
import shutil

import pytest

from test_kernel_resources import BUILD, LLVM, _kernels
from test_mask3d_kernel_resources import _short

TOOLS = os.path.exists(f"{LLVM}/clang-offload-bundler") and shutil.which("c++filt")
needs_objects = pytest.mark.skipif(not all(os.path.isfile(os.path.join(BUILD, o)) for o in ("patch.o", "resident.o")) or not TOOLS,
                                   reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")

PARENT = {
    (32, 32): (171, 172, 172), (32, 64): (176, 177, 177), (32, 128): (170, 168, 168),
    (64, 32): (174, 174, 174), (64, 64): (166, 168, 168), (64, 128): (169, 172, 172),
    (128, 32): (166, 166, 166), (128, 64): (168, 168, 168), (128, 128): (128, 128, 128),
}
ROUTED = [s for s in PARENT if s[0] * s[1] <= 8192]     # RESIDENT_MAX_POINTS


def _named(obj):
    return {_short(m): res for m, res in _kernels(os.path.join(BUILD, obj)).items()}


def _register_class(n):
    """Registers are allocated in blocks of 8; occupancy changes where 512 // registers does."""
    return 512 // (-(-n // 8) * 8)


@needs_objects
def test_new_kernels_use_no_scratch():
    k = _named("patch.o")
    new = [n for n in k if re.match(r"(patch_gather_kernel|patch_pack_kernel|patch_blend_kernel|resident_kernel)\b", n)]
    assert {re.sub(r"<.*", "", n) for n in new} == {"patch_gather_kernel", "patch_pack_kernel", "patch_blend_kernel", "resident_kernel"}
    assert sum(n.startswith("resident_kernel<") for n in new) == 3 * len(ROUTED)
    for n in new:
        assert k[n]["vgpr_spill_count"] == 0 and k[n]["private_segment_fixed_size"] == 0, (n, k[n])
    for n in new:   # memory-bound gather / pack / blend: 8 wavefronts per SIMD
        if not n.startswith("resident_kernel"):
            assert k[n]["vgpr_count"] <= 64, (n, k[n])


@needs_objects
def test_per_window_mask_loop_keeps_the_register_class_of_its_shape():
    k = _named("patch.o")
    for n1, n2 in ROUTED:
        for op in range(3):
            res = k[f"resident_kernel<{n1}, {n2}, {op | 4}>"]
            assert _register_class(res["vgpr_count"]) >= _register_class(PARENT[(n1, n2)][op]), ((n1, n2, op), res, PARENT[(n1, n2)][op])
    assert not any(n.startswith("resident_kernel<128, 128") for n in k)      # never routed: not instantiated


@needs_objects
def test_shared_mask_instantiations_keep_their_register_counts():
    k = _named("resident.o")
    seen = {n: res["vgpr_count"] for n, res in k.items() if n.startswith("resident_kernel<")}
    want = {f"resident_kernel<{n1}, {n2}, {op}>": PARENT[(n1, n2)][op] for (n1, n2) in PARENT for op in range(3)}
    assert seen == want
