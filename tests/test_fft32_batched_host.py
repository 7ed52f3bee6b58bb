"""The grouped exchange reads of the 32 x 32 transform's second half (p3d_fft32.hpp: p32_half2) against the plain loop they replaced, on the CPU
and bit for bit: tests/csrc/test_fft32_batched_host.cpp, built the way tests/test_host_logic.py builds its host programs, without contraction
(the library's own flag: a fused multiply-add in one of the two would be a difference of the compiler's making)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pseudo-3d-interpolation_amd", "csrc")


def test_grouped_exchange_reads_are_the_plain_loop(tmp_path):
    exe = tmp_path / "fft32_batched_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "test_fft32_batched_host.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "ALL OK" in res.stdout
