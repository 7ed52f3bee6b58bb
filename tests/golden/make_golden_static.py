"""Fixtures of step 5 (tests/golden/static.npz) from the REFERENCE's own detect_seafloor_reflection / get_static / compensate_static.

    python tests/golden/make_golden_static.py /path/to/reference

The reference's static_correction_segy imports segyio and tqdm at module level (and its utils dask / xarray); empty stand-ins go into
``sys.modules`` first.  Its functions are run unchanged but for ONE wrapper: ``filter_interp_1d`` returns scipy spline values also at the samples
that were kept, equal to the input integers up to ~1e-13, and the callers truncate them -- one sample low at random.  The wrapper snaps values
within 1e-6 of an integer to it (asserting that none lies between 1e-6 and 1e-3, so the snap is unambiguous); the script prints how many traces
of every case the unmodified reference puts elsewhere.  The sections are quantised to multiples of 1/512 so that the file stays small; they are
recorded once and shared by the cases, and the padded variant is recorded as the per-trace number of leading zeros only.

Recorded per case: live-trace mask, threshold, raw first crossings, both spline stages (input / output), baseline, peak picks, final index, the
spline stage and the result of get_static, static_samples, and the parameters.  The script asserts what the tests rely on (see the asserts),
so that a weak fixture cannot pass silently."""
import json
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

import static_numpy as H  # noqa: E402
from pseudo_3D_interpolation import static_correction_segy as scs  # noqa: E402
from pseudo_3D_interpolation.functions import filter as rf  # noqa: E402
from pseudo_3D_interpolation.functions.utils import slice_valid_data  # noqa: E402

Q = 512.0
ORIGINAL_INTERP = rf.filter_interp_1d
LOG = []
SNAP = [True]


def snapping_interp(data, *args, **kwargs):
    res = ORIGINAL_INTERP(data, *args, **kwargs)
    if SNAP[0]:
        off = np.abs(res - np.rint(res))
        assert not np.any((off > 1e-6) & (off < 1e-3)), 'a spline value is ambiguously close to an integer'
        res = np.where(off <= 1e-6, np.rint(res), res)
    LOG.append(('interp', np.array(data), res.copy()))
    return res


def logging_ratio(a, nsta, nlta, axis=-1, _orig=rf.sta_lta_filter):
    res = _orig(a, nsta, nlta, axis=axis)
    LOG.append(('ratio', np.array(a), res, nsta, nlta))
    return res


def logging_median(a, win=3, padded=False, _orig=rf.moving_median):
    res = _orig(a, win, padded)
    LOG.append(('median', np.array(a), res.copy()))
    return res


rf.filter_interp_1d = scs.filter_interp_1d = snapping_interp
rf.sta_lta_filter = logging_ratio
rf.moving_median = logging_median


def section(seed, ns, ntr, floor, burst_row, bursts, zero_traces):
    """Seafloor wavelet on low water-column noise: smooth relief, one depression, a planted static of a few samples on most traces."""
    rng = np.random.default_rng(seed)
    x = np.arange(ntr)
    relief = floor + 18 * np.sin(2 * np.pi * x / ntr * 1.3) + 8 * np.cos(2 * np.pi * x / ntr * 3.1)
    c, half = int(0.62 * ntr), 14
    relief += 26 * np.exp(-0.5 * ((x - c) / (half / 2.0)) ** 4)                      # the depression: deeper seafloor
    jitter = np.where(rng.random(ntr) < 0.75, rng.integers(-5, 6, ntr), 0)
    seafloor = np.rint(relief).astype(int) + jitter
    a = rng.normal(0, 2.0 / Q, (ns, ntr))
    t = np.arange(-8, 40)
    tw = t - 0.37                                                                    # off-centre: no two samples of the wavelet are equal
    wavelet = (1 - 2 * (np.pi * 0.09 * tw) ** 2) * np.exp(-(np.pi * 0.09 * tw) ** 2) * 100
    coda = rng.normal(0, 1, (150, ntr)) * (6 * np.exp(-np.arange(150) / 40.0))[:, None]
    for k in range(ntr):
        amp = 1 + 0.1 * rng.random()
        a[seafloor[k] + t, k] += amp * wavelet
        a[seafloor[k] + 10:seafloor[k] + 160, k] += coda[:, k]
    for k in bursts:                                                                 # water-column bursts: false first crossings
        a[burst_row:burst_row + 12, k] += 25 * rng.choice([-1.0, 1.0], 12) * (1 + rng.random(12))
    a = np.rint(a * Q) / Q
    for k in range(ntr):                                                             # no two of a trace's large amplitudes are equal
        col = a[:, k]
        big = np.flatnonzero(col > 1.0)
        order = big[np.argsort(col[big], kind='stable')]
        for lo, hi in zip(order[:-1], order[1:]):
            if col[hi] <= col[lo]:
                col[hi] = col[lo] + 1 / Q
    a[0, a[0] == 0] = 1 / Q                                                          # a padded copy starts at the first non-zero sample
    a[:, zero_traces] = 0
    return a.astype(np.float32), seafloor


def run_case(data, detect_kw, static_kw, offset=None):
    """The reference on ``data`` (samples x traces); returns the recorded stages."""
    del LOG[:]
    idx_amp = rf.detect_seafloor_reflection(data, **detect_kw)
    kinds = [e[0] for e in LOG]
    assert kinds == ['ratio', 'interp', 'median', 'interp'], kinds
    _, ratio_in, ratio, nsta, nlta = LOG[0]
    live = np.count_nonzero(data, axis=0) > 0
    assert ratio_in.shape[1] == live.sum()
    thr = ratio[nlta:2 * nlta].max()
    raw = np.argmax(ratio > thr, axis=0)
    rec = dict(live=live, threshold=np.float64(thr), raw=raw, nsta_nlta=np.array([nsta, nlta]))
    assert np.array_equal(LOG[1][1], raw)
    rec['interp1_out'], rec['median_in'], rec['baseline'] = LOG[1][2], LOG[2][1], LOG[2][2].astype(int)
    rec['interp2_in'], rec['interp2_out'] = LOG[3][1], LOG[3][2]
    rec['peak'] = LOG[3][1][live]
    rec['idx_amp'] = idx_amp
    # either accumulation order and a threshold moved by 1e-5 (relative) give the same crossings
    ratio64 = logging_ratio(ratio_in.astype(np.float64), nsta, nlta, axis=0)
    thr64 = ratio64[nlta:2 * nlta].max()
    assert abs(thr64 - thr) <= 2e-6 * thr64, (thr, thr64)
    # (the one element that IS the threshold never exceeds it in a consistent computation and would exceed any lowered one: it is left out)
    for r, t in ((ratio, thr), (ratio64, thr64)):
        assert np.array_equal(np.argmax(r > t, axis=0), raw)
        others = r.copy()
        top = np.unravel_index(np.argmax(r[nlta:2 * nlta]), r[nlta:2 * nlta].shape)
        others[nlta + top[0], top[1]] = 0
        for f in (1 - 1e-5, 1 + 1e-5):
            assert np.array_equal(np.argmax(others > t * f, axis=0), raw), 'a near-tie decides a first crossing'
    # no tie among the n + 1 largest amplitudes of any search window
    win, n = detect_kw['win'], detect_kw['n']
    cols = data[:, live]
    for k, b in enumerate(rec['baseline']):
        assert b - win >= 0 and b + win < data.shape[0]
        top = np.sort(cols[b - win:b + win + 1, k])[::-1][:n + 1]
        assert np.unique(top).size == top.size, ('equal amplitudes among the candidates', k, top)
    # the NumPy restatement of the kernels agrees with the reference
    first, hthr, hraw = H.detect(data, nsta, nlta)
    assert np.array_equal(first >= 0, live) and np.array_equal(hraw[live], raw) and abs(hthr - thr) <= 2e-6 * thr
    base = np.zeros(data.shape[1], int)
    base[live] = rec['baseline']
    assert np.array_equal(H.peaks(data, first, base, win, n)[live], rec['peak'])

    idx = idx_amp if offset is None else idx_amp + offset
    del LOG[:]
    static = scs.get_static(idx, **static_kw)
    assert [e[0] for e in LOG] == ['interp']
    rec['gs_in'], rec['gs_interp_out'], rec['static'] = idx, LOG[0][2], static
    _, rec['static_samples'] = scs.compensate_static(data[:4], static, dt=0.25, units='ms', verbosity=0)
    ties = np.flatnonzero(np.abs(np.abs(static - np.floor(static)) - 0.5) <= 1e-3)
    assert ties.size == 0, ('a static on a rounding tie', ties, static[ties])
    assert np.count_nonzero(rec['static_samples']) >= 0.05 * idx.size
    # every clipping rule fires
    unclipped = scs.get_static(idx, **dict(static_kw, limit_depressions=False, limit_samples=None, limit_by_MAD=None))
    dep_only = scs.get_static(idx, **dict(static_kw, limit_samples=None, limit_by_MAD=None))
    rec['n_dep'] = int(np.sum(dep_only != unclipped))
    rec['n_lim'] = int(np.sum(np.abs(dep_only) > static_kw['limit_samples']))
    assert rec['n_dep'] >= 1 and rec['n_lim'] >= 1, (rec['n_dep'], rec['n_lim'])
    # the unmodified reference, for the record
    SNAP[0] = False
    plain = rf.detect_seafloor_reflection(data, **detect_kw)
    SNAP[0] = True
    rec['n_unsnapped_differ'] = int(np.sum(plain != idx_amp))
    return rec


STATIC_KW = dict(kind='diff', interp_kind='cubic', win_mad=None, win_sg=7, limit_perc=False, limit_samples=4, limit_by_MAD=3,
                 limit_depressions=[10, 6, 2])
SECTIONS = {
    'A': dict(seed=7, ns=1200, ntr=300, floor=600, burst_row=300, bursts=[40, 41, 150, 260], zero_traces=[90, 201]),     # nsta 1 -> 3 / 50
    'B': dict(seed=6, ns=2600, ntr=160, floor=1250, burst_row=700, bursts=[30, 100, 101], zero_traces=[55, 120]),        # nsta 3, nlta 130
}
CASES = {
    'A': ('A', dict(nsta=None, nlta=None, win=30, win_median=11, n=5), STATIC_KW),
    'A-wide': ('A', dict(nsta=None, nlta=None, win=100, win_median=11, n=7), dict(STATIC_KW, limit_samples=3, win_sg=9)),
    'B': ('B', dict(nsta=None, nlta=None, win=20, win_median=7, n=3), STATIC_KW),
    'B-mid': ('B', dict(nsta=5, nlta=150, win=40, win_median=11, n=5), dict(STATIC_KW, limit_depressions=[8, 8, 3])),
    'B-wide': ('B', dict(nsta=None, nlta=None, win=150, win_median=11, n=9), dict(STATIC_KW, win_mad=9)),
}
PAD = 40

out, seafloors = {}, {}
for name, kw in SECTIONS.items():
    out[f'section/{name}'], seafloors[name] = section(**kw)
    out[f'bursts/{name}'] = np.array(kw['bursts'])
    out[f'zero_traces/{name}'] = np.array(kw['zero_traces'])
names = []
for name, (sec, dkw, skw) in CASES.items():
    data = out[f'section/{sec}']
    rec = run_case(data, dkw, skw)
    bursts = SECTIONS[sec]['bursts']
    keep = np.cumsum(rec['live']) - 1
    assert all(abs(rec['raw'][keep[b]] - rec['idx_amp'][b]) > 50 for b in bursts), 'a burst trace without a false first crossing'
    assert (rec['nsta_nlta'][0] == 3 and rec['nsta_nlta'][1] == 50) == (sec == 'A')
    assert np.abs(rec['idx_amp'] - seafloors[sec])[rec['live']].max() <= 12
    for k, v in rec.items():
        out[f'case/{name}/{k}'] = np.asarray(v)
    out[f'case/{name}/params'] = np.array(json.dumps(dict(section=sec, detect=dkw, static=skw, padded=False)))
    names.append(name)
    print(f"{name}: nsta/nlta {rec['nsta_nlta']}, thr {rec['threshold']:.6g}, statics {rec['static_samples'].min()} ... {rec['static_samples'].max()}, "
          f"non-zero {np.count_nonzero(rec['static_samples'])}, clipped by depressions {rec['n_dep']}, beyond limit_samples {rec['n_lim']}, "
          f"unmodified reference differs on {rec['n_unsnapped_differ']} traces")

# the padded variant of A: every trace behind its own number of leading zeros; the reference is given the sliced array, as its CLI does
rng = np.random.default_rng(17)
A = out['section/A']
start = rng.integers(0, PAD + 1, A.shape[1])
start[[0, 7]] = [0, PAD]
padded = np.zeros((A.shape[0] + PAD, A.shape[1]), np.float32)
for k, s in enumerate(start):
    padded[s:s + A.shape[0], k] = A[:, k]
sliced, idx_start = slice_valid_data(padded, A.shape[0])
live = np.count_nonzero(A, axis=0) > 0
assert np.array_equal(sliced, A) and np.array_equal(idx_start[live], start[live])
_, dkw, skw = CASES['A']
rec = run_case(sliced, dkw, skw, offset=idx_start)
for k, v in rec.items():
    out[f'case/A-pad/{k}'] = np.asarray(v)
    if k not in ('gs_in', 'gs_interp_out', 'static', 'static_samples', 'n_dep', 'n_lim'):
        assert np.array_equal(np.asarray(v), out[f'case/A/{k}']), k
out['case/A-pad/params'] = np.array(json.dumps(dict(section='A', detect=dkw, static=skw, padded=True)))
out['pad/start'] = np.where(live, start, 0).astype(np.int32)
out['pad/extra'] = np.array(PAD)
names.append('A-pad')
print(f"A-pad: statics {rec['static_samples'].min()} ... {rec['static_samples'].max()}, non-zero {np.count_nonzero(rec['static_samples'])}")

out['cases'] = np.array(names)
flags = []
for action in scs.define_input_args()._actions:
    if action.dest != 'help':
        flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default,
                          choices=None if action.choices is None else list(action.choices), nargs=action.nargs,
                          type=None if action.type is None else action.type.__name__, help=action.help))
out['cli_flags'] = np.array(json.dumps(flags))
path = os.path.join(HERE, 'static.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
