"""The exchange of the 32 x 32 transform inside row_pipe32_kernel keeps its reads in flight together -- read from the code object on the CPU.

A transform of 1024 points is two in-register radix-32 butterflies around ONE trip through LDS: sixteen ds_write_b128 per lane, then 32 values and
31 twiddles read back (p3d_fft32.hpp: p32_half2).  Left to the compiler the reads came out one (value, twiddle) pair at a time, each waited for
before the next was requested: 30 s_waitcnt lgkmcnt per transform with one or two reads in flight, in a kernel that runs two wavefronts per
SIMD and so cannot hide an LDS round trip behind other wavefronts.  p32_half2 issues the reads in groups now; this test pins what that buys, in
every instantiation of the kernel and for every transform in it (behind each run of sixteen ds_write_b128):
  * at least 16 LDS reads are issued before the first s_waitcnt on lgkmcnt;
  * at most 12 such waits lie between the first and the last LDS read of the transform (the plain loads had 30).
An edit that hands the order back to the compiler -- plain loads again, a wait that takes no operands -- shows up here and in no functional test."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "pseudo-3d-interpolation_amd", "csrc", "build")
OBJ = os.path.join(BUILD, "inst_1024.o")
LLVM = "/opt/rocm/lib/llvm/bin"

MIN_READS_BEFORE_WAIT = 16
MAX_WAITS_INSIDE = 12


def _disassembly(obj):
    """{mangled kernel name: [instruction text, ...]} of the gfx950 code object inside a library object."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "f.fatbin"), os.path.join(d, "f.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", obj], check=True, capture_output=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True, capture_output=True)
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur.append(line.split("//")[0].strip())
    return out


def _transforms(insts):
    """[(reads before the first lgkmcnt wait, lgkmcnt waits between the first and the last read)] for every exchange of a kernel: the LDS reads
    that follow a run of sixteen ds_write_b128, up to the next LDS write (or the end of the kernel)."""
    res, i, n = [], 0, len(insts)
    while i < n:
        if not insts[i].startswith("ds_write_b128"):
            i += 1
            continue
        writes = 0
        while i < n and not insts[i].startswith("ds_read"):   # the run: LDS writes with arithmetic between them
            if insts[i].startswith("ds_write"):
                writes += 1
            i += 1
        span = []
        while i < n and not insts[i].startswith("ds_write"):
            span.append(insts[i])
            i += 1
        if writes != 16:
            continue
        reads = [k for k, s in enumerate(span) if s.startswith("ds_read")]
        waits = [k for k, s in enumerate(span) if s.startswith("s_waitcnt") and "lgkmcnt" in s]
        first_wait = min([k for k in waits if k > reads[0]], default=len(span))
        res.append((sum(1 for k in reads if k < first_wait), sum(1 for k in waits if reads[0] < k < reads[-1]), len(reads)))
    return res


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(f"{LLVM}/clang-offload-bundler") or not shutil.which("c++filt"),
                    reason="needs the object files of the library build (python -c 'import __graft_entry__ as g; g.build()') and the ROCm LLVM tools")
def test_exchange_reads_are_in_flight_together():
    kernels = {k: v for k, v in _disassembly(OBJ).items() if "row_pipe32_kernel" in k}
    assert len(kernels) >= 24, sorted(kernels)                 # FIRST x 4, MID and LAST x (dtype, sparse, sums) and the APOCS forms
    bad, table = [], []
    for mangled, insts in sorted(kernels.items()):
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*$", "", name).replace("void ", "").replace("p3d::", "")
        tr = _transforms(insts)
        table.append((short, tr))
        if not tr:
            bad.append((short, "no exchange found"))
        for before, inside, nreads in tr:
            if nreads < 32 or before < MIN_READS_BEFORE_WAIT or inside > MAX_WAITS_INSIDE:
                bad.append((short, before, inside, nreads))
    for short, tr in table:
        print(short, tr)
    # a steady-state pass holds two transforms, a first or last pass one
    assert all(len(tr) == (2 if re.search(r"<\d, (true|false), 0,", short) else 1) for short, tr in table), table
    assert not bad, bad
