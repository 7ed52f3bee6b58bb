"""Step-7 mistie correction rate on the GPU: line crossings, nearest shot points and the windowed cross-correlation on a synthetic survey, host
array to host array (transfers included), every stage in a child process under its own time limit; the stages after one that fails or runs
out of time are not started.

Case (default): 200 lines x 5000 shot points -- 100 along x and 100 along y over a square, every line wiggling by a fraction of the line
spacing, so that every line of one family crosses every line of the other once (10000 crossings among a million segments); the correlation
on --ncross pairs of envelope-like traces of --ns samples with planted shifts.  Prints one JSON document.

    python tools/mistie_rate.py [--lines 200 --shots 5000 --ns 4096 --ncross 2048 --reps 3 --limit 120 --out profiles/mistie_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ('cross', 'nearest', 'xcorr')


def median_of(fn, reps):
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:]))


def survey(nlines, shots, seed=0):
    rng = np.random.default_rng(seed)
    half = nlines // 2
    size = 1000.0 * half
    s = np.linspace(-50.0, size + 50.0, shots)
    lines = []
    for k in range(nlines):
        base = 1000.0 * (k % half) + 500.0
        wiggle = 120.0 * np.sin(2 * np.pi * s / size * (1 + k % 5) + k) + rng.normal(0, 0.3, shots)
        lines.append(np.stack([s, base + wiggle], axis=1) if k < half else np.stack([base + wiggle, s], axis=1))
    return lines


def traces(ncross, ns, seed=1):
    rng = np.random.default_rng(seed)
    pool = np.abs(rng.standard_normal((64, ns + 64))).astype(np.float32) + np.float32(0.01)
    kernel = np.hanning(31).astype(np.float32)
    pool = np.stack([np.convolve(p, kernel, 'same') for p in pool])
    pick, shift = rng.integers(0, 64, ncross), rng.integers(-20, 21, ncross)
    a = np.stack([pool[p, 32:32 + ns] for p in pick])
    b = np.stack([pool[p, 32 + d:32 + d + ns] for p, d in zip(pick, shift)])
    return a, b, shift


def stage(name, a):
    from pseudo_3d_interpolation_amd import _ffi
    from pseudo_3d_interpolation_amd.functions import mistie as M
    if name in ('cross', 'nearest'):
        lines = survey(a.lines, a.shots)
        nseg = sum(p.shape[0] - 1 for p in lines)
        found = {}

        def cross():
            found['xy'], found['idx'] = M.find_intersections(lines)
        if name == 'cross':
            pairs = M.candidate_pairs(lines)
            t = median_of(cross, a.reps)
            return dict(lines=a.lines, shots=a.shots, segments=nseg, candidate_pairs=int(pairs.shape[0]), crossings=int(found['xy'].shape[0]), ms=round(t * 1e3, 2),
                        segment_pairs_per_s_brute_force_equivalent=float(f'{sum((lines[i].shape[0] - 1) * (lines[j].shape[0] - 1) for i, j in pairs) / t:.4g}'))
        cross()
        t = median_of(lambda: M.nearest_intersection_vertices(lines, found['xy'], found['idx']), a.reps)
        k = found['xy'].shape[0]
        return dict(crossings=k, vertices_searched=2 * k * a.shots, ms=round(t * 1e3, 2), vertices_per_s=float(f'{2 * k * a.shots / t:.4g}'))
    ta, tb, shift = traces(a.ncross, a.ns)
    ranges = np.tile(np.array([0, a.ns, 0, a.ns], np.int32), (a.ncross, 1))
    out = {}
    res = dict(ncross=a.ncross, ns=a.ns)
    for path in ('auto', 'global'):
        t = median_of(lambda: out.update(r=_ffi.mistie_xcorr(ta, tb, ranges, path=path)), a.reps)
        terms = a.ncross * (a.ns * a.ns - (a.ns // 2) * (a.ns // 2 + 1) // 2 - ((a.ns - 1) // 2) * ((a.ns - 1) // 2 + 1) // 2)
        res[path] = dict(form='lds' if path == 'auto' and a.ns <= _ffi.MISTIE_LDS_SAMPLES else 'global', ms=round(t * 1e3, 2),
                         multiply_adds_per_s=float(f'{terms / t:.4g}'), crossings_per_s=round(a.ncross / t, 1),
                         planted_shifts_found=float(np.mean(out['r'][0] == -shift)))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--lines', type=int, default=200)
    p.add_argument('--shots', type=int, default=5000)
    p.add_argument('--ns', type=int, default=4096)
    p.add_argument('--ncross', type=int, default=2048)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--limit', type=float, default=120.0, help='time limit of every stage [s]')
    p.add_argument('--stage', choices=STAGES, default=None, help='run one stage in this process (what the parent starts)')
    p.add_argument('--out', type=str, default=None)
    a = p.parse_args()
    if a.stage:
        print(json.dumps(stage(a.stage, a)))
        return 0
    res = {}
    for name in STAGES:
        cmd = [sys.executable, os.path.abspath(__file__), '--stage', name, '--lines', str(a.lines), '--shots', str(a.shots), '--ns', str(a.ns),
               '--ncross', str(a.ncross), '--reps', str(a.reps)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            res[name] = {'error': f'no result within {a.limit} s'}
            break
        if done.returncode != 0:
            res[name] = {'error': f'exit status {done.returncode}', 'stderr': done.stderr[-2000:]}
            break
        res[name] = json.loads(done.stdout.strip().split('\n')[-1])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')
    return 0 if all('error' not in v for v in res.values()) and len(res) == len(STAGES) else 1


if __name__ == '__main__':
    sys.exit(main())
