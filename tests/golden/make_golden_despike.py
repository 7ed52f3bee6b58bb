"""Fixtures of step 8 (tests/golden/despike.npz) from the REFERENCE's own despike_2D.

    python tests/golden/make_golden_despike.py /path/to/reference

The reference's despiking_2D_segy imports segyio, tqdm, dask and xarray at module level; empty stand-ins go into ``sys.modules`` first (despike_2D
uses none of them).  Recorded per case: the flat indices of the samples the reference writes (taken from a run with out='zeros' on a section without
exact zeros) and the values it writes there; the sections themselves are recorded once and shared by the cases.  The script asserts that the set of
cases exercises what the tests rely on, so that a fixture which detects nothing cannot pass silently, and prints the spikes of every case."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, '..', 'helpers'))
for name in ('segyio', 'tqdm', 'dask', 'dask.array', 'xarray'):
    mod = types.ModuleType(name)
    mod.tqdm = lambda it, **kw: it
    sys.modules[name] = mod

import despike_numpy as H  # noqa: E402
from pseudo_3D_interpolation.despiking_2D_segy import despike_2D  # noqa: E402

THRESHOLD = {'mean': 3, 'median': 6, 'rms': 2}
MODES, OUTS = ('mean', 'median', 'rms'), ('scaled', 'mode', 'threshold', 'zeros', 'median')
NS, NTR = 360, 100
# (trace, first row, last row + 1) of the planted bursts
BURSTS = [(20, 40, 70), (20, 90, 94),               # an isolated spike, and a run too short to be one on a trace that passes the count filter
          (40, 100, 150), (40, 156, 206),           # two spikes on one trace whose padded rows overlap
          (60, 200, 230), (61, 210, 240),           # adjacent traces, overlapping rows: the second reads what the first wrote
          (85, 306, 326),                           # rows that only the additional view holds enough of (and the unexamined tail without one)
          (NTR - 1, 250, 280)]                      # right edge


def background(rng, ns, ntr):
    gain = 1.0 + 0.5 * np.sin(np.linspace(0, 3, ns))[:, None] * np.cos(np.linspace(0, 2, ntr))[None, :]
    a = (rng.standard_normal((ns, ntr)) * gain).astype(np.float32)
    a[a == 0] = np.float32(0.01)
    return a, gain


def section(seed, ns, ntr, bursts):
    rng = np.random.default_rng(seed)
    a, gain = background(rng, ns, ntr)
    for x, r0, r1 in bursts:
        amp = 30.0 * (1.0 + 0.1 * rng.random(r1 - r0)) * rng.choice([-1.0, 1.0], r1 - r0)
        a[r0:r1, x] = (amp * gain[r0:r1, x]).astype(np.float32)
    return a


def overlap_rows(p, q):
    return p[1] < q[2] and q[1] < p[2]


out = {'section/spiky': section(8, NS, NTR, BURSTS), 'section/quiet': section(9, 240, 40, [])}
cases = []
for mode in MODES:                                   # every mode x every out, additional view (360 % 99 != 0)
    for o in OUTS:
        cases.append(('spiky', 110, 10, 5, mode, o))
for w in (3, 7, 11, 21):                             # unexamined tail rows (360 % 90 == 0)
    cases += [('spiky', 100, 10, w, 'mean', 'zeros'), ('spiky', 100, 10, w, 'mean', 'threshold'), ('spiky', 100, 10, w, 'median', 'median')]
cases += [('spiky', 100, 10, 7, 'rms', 'scaled'), ('spiky', 100, 10, 11, 'rms', 'scaled'), ('spiky', 100, 10, 9, 'median', 'mode')]
cases.append(('quiet', 100, 10, 5, 'mean', 'zeros'))

names = []
seen = dict(two_on_one=0, cross=0, right_edge=0, short_rejected=0, one_view=0, tail=0, add=0)
for sec, window, ov, w, mode, o in cases:
    a = out['section/' + sec]
    thr = 2 if (mode, w) == ('mean', 3) else THRESHOLD[mode]           # |a| <= 3 mean|a| over 3 traces: a threshold of 3 can never fire there
    kw = dict(window=window, dt=1.0, overlap=ov, ntraces=w, mode=mode, threshold=thr)
    zeros = despike_2D(a.copy(), out='zeros', **kw)
    ref = despike_2D(a.copy(), out=o, **kw)
    idx = np.flatnonzero(zeros != a)
    assert np.array_equal(np.flatnonzero(ref != a)[~np.isin(np.flatnonzero(ref != a), idx)], []), 'a write outside the written set'
    got, spikes = H.despike_2D(a, out=o, return_spikes=True, **kw)
    assert got.tobytes() == ref.tobytes(), (sec, window, w, mode, o)
    h = w // 2
    assert all(x >= h for x, *_ in spikes), 'no reference fixture may have a spike at x < h'
    written = np.zeros(a.shape, bool)
    for x, lo, hi, _, _ in spikes:
        written[lo:hi, x] = True
    assert np.array_equal(np.flatnonzero(written), idx)
    # the spike list does not hang on a near-tie of the float32 sums: it is the same with the threshold moved by twice the summation bound
    for f in (1 - 2 * w * 2.0**-23, 1 + 2 * w * 2.0**-23):
        assert H.find_spikes(a, **dict(kw, threshold=thr * f)) == spikes, 'near-tie decides a spike'
    M, dy, main_end, add_start = H.window_params(a.shape[0], window, 1.0, ov)
    if sec == 'quiet':
        assert not spikes
    else:
        assert len(spikes) >= 5
        seen['tail' if add_start is None else 'add'] += 1
        seen['two_on_one'] += any(p[0] == q[0] and p is not q and overlap_rows(p, q) for p in spikes for q in spikes)
        seen['cross'] += any(0 < abs(p[0] - q[0]) <= h and overlap_rows(p, q) for p in spikes for q in spikes)
        seen['right_edge'] += any(x >= a.shape[1] - h for x, *_ in spikes)
        seen['short_rejected'] += any(x == 20 for x, *_ in spikes) and not any(x == 20 and first >= 85 for x, _, _, first, _ in spikes)
        if add_start is not None:
            cand = H.candidates(a, w, mode, thr)[:, 85]
            seen['one_view'] += (cand[:main_end].sum() <= M * 0.1 < cand[add_start:].sum()) and any(x == 85 for x, *_ in spikes)
        else:
            assert not any(last >= main_end for *_, last in spikes)          # rows 306 ... are beyond the main view and there is no other
    name = f'{sec}-{window}-{ov}-{w}-{mode}-{thr}-{o}'
    names.append(name)
    out[f'case/{name}/idx'] = idx.astype(np.int32)
    out[f'case/{name}/val'] = ref.ravel()[idx]
    print(f'{name}: {len(spikes)} spikes, {idx.size} samples written; M {M} dy {dy} main_end {main_end} add_start {add_start}')
    print('   ', spikes)
assert all(v > 0 for v in seen.values()), seen
assert {c[3] for c in cases} >= {3, 5, 7} and {c[3] for c in cases} & {9, 11, 21}
assert {(c[4], c[5]) for c in cases} >= {(m, o) for m in MODES for o in OUTS}
out['cases'] = np.array(names)
print(seen)
np.savez_compressed(os.path.join(HERE, 'despike.npz'), **out)
print(os.path.getsize(os.path.join(HERE, 'despike.npz')), 'bytes')
