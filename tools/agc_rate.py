"""Rate of the step-15 AGC kernels (p3d_agc) on a 1024 x 1024 x 1024 float32 slice-major cube: rms, mean and median at win 101 and
501.  Each case runs in a child process of its own under `timeout -k 10 <s>` and `rocprofv3 --kernel-trace --stats`; the kernel
statistics of all cases are collected into one CSV (default profiles/agc_kernel_stats.csv) with the rate on two yardsticks:
8 B/pt (one read, one write) and 12 B/pt (plus the trailing window read from HBM again).  A case that fails or times out ends the run.

    python tools/agc_rate.py [--n 1024] [--out profiles/agc_kernel_stats.csv]
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("rms", 101), ("mean", 101), ("median", 101), ("rms", 501), ("mean", 501), ("median", 501)]


def child(kind, win, n):
    import numpy as np
    sys.path.insert(0, ROOT)
    from pseudo_3d_interpolation_amd import _ffi
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, n, n), dtype=np.float32)
    if kind == "mean":
        np.abs(x, out=x)
    for _ in range(2):       # the first launch warms the code object up; rocprofv3 reports both
        t0 = time.perf_counter()
        y = _ffi.agc(x, win, kind=kind)
        print(f"{kind} win {win}: {time.perf_counter() - t0:.3f} s wall (copies included)", flush=True)
    assert np.isfinite(y[::97, ::89, ::83]).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agc_kernel_stats.csv"))
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.n)
    points = a.n ** 3
    rows = []
    for kind, win in CASES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "agc", "--",
                   sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--child", kind, str(win)]
            res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            print(res.stdout.strip()[-600:], flush=True)
            if res.returncode != 0:
                print(res.stderr[-3000:], file=sys.stderr)
                print(f"{kind} win {win}: exit status {res.returncode}, stopping", file=sys.stderr)
                sys.exit(1)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            with open(stats[0]) as f:
                for r in csv.DictReader(f):
                    if "agc_" not in r["Name"]:
                        continue
                    ms = float(r["MinNs"]) / 1e6
                    rows.append(dict(kind=kind, win=win, kernel=r["Name"].replace("(anonymous namespace)::", "").split("(")[0], calls=r["Calls"], avg_ms=f"{float(r['AverageNs']) / 1e6:.3f}",
                                     min_ms=f"{ms:.3f}", tbps_8B=f"{8 * points / ms / 1e9:.2f}", tbps_12B=f"{12 * points / ms / 1e9:.2f}"))
                    print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
