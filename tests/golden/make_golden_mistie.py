"""Fixtures of step 7 (tests/golden/mistie.npz) from the REFERENCE's own compute_misties / load_trace / cross_correlation_shift /
compensate_mistie / envelope / rescale.

    python tests/golden/make_golden_mistie.py /path/to/reference

The reference's mistie_correction_segy imports segyio, tqdm, shapely, geopandas (and its utils dask / xarray / pyproj) at module level, and
``functions.utils_io`` although it ships ``utils_IO.py``.  Stand-ins go into ``sys.modules`` first (each with a ModuleSpec); the one for
segyio is a small in-memory file table -- ``open`` hands out an object with ``tracecount``, ``samples``, ``trace[i]`` and ``trace.raw[a:b]``,
``tools.dt`` its sample interval -- so that the reference's ``load_trace`` runs UNCHANGED on synthetic sections (the bad-trace test, the clipped
slice, the deleted row and the ``'env' in path`` rule are its own).  ``envelope`` is wrapped only to record its input and output.

Survey cases (``case/<name>/...``): small sections per line (quantised to multiples of 1/256), the crossings (line pair and trace on either
line), per crossing what went into the envelope, what came out, the window as (first sample, length) on either trace, the number of samples
left after the zeros are dropped, the shift, the coefficient (the reference's float32 value and recomputed in float64), the quality mask, and
per line the offsets, offsets in ms and the residuals.  Kernel cases (``kernel/<name>/...``): two windows, n, shift, float64 coefficient.

The script asserts what the tests rely on, so that the reference alone stays decisive: the winning correlation value beats every other lag's
by 1e-4 of itself (float64, direct sums); no |coeff| within 1e-3 of the quality threshold; no unrounded offset within 1e-6 of a half-integer;
crossings both kept and rejected; a bad trace in the mixing branch, one of them at trace 0 (the clipped slice); no bad-trace mean within 1e-3
of 0.4.  The kernel cases with n = 1 and 2 are exempt from the margin: their expected shift follows from the first-occurrence rule (n = 1: one
lag, shift 0, r = 0 / 0 = NaN; n = 2 with equal values at both lags: the first, shift 1).

``coeff_tol``: the survey tests that go through the GPU envelope compare coefficients within it.  The existing envelope parity test allows a
relative L2 error of 1e-5 per trace; the reference envelopes are perturbed by random errors of exactly that size (32 draws), and ten times the
largest change of a coefficient is stored -- ten-fold because the draws are a sample, not a bound."""
import importlib.machinery
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, '..', 'helpers'))

FILES = {}                                       # path -> fake SEG-Y file


class FakeTraces:
    def __init__(self, data):
        self.raw = data

    def __getitem__(self, i):
        return self.raw[i].copy()


class FakeFile:
    def __init__(self, data, dt_ms, delay_ms):
        self.tracecount = data.shape[0]
        self.samples = np.arange(data.shape[1]) * dt_ms + float(delay_ms)
        self.trace = FakeTraces(data)
        self.dt_us = dt_ms * 1000

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


for name in ('segyio', 'segyio.tools', 'tqdm', 'dask', 'dask.array', 'xarray', 'shapely', 'geopandas', 'pyproj'):
    mod = types.ModuleType(name)
    mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
    sys.modules[name] = mod
sys.modules['tqdm'].tqdm = lambda it, **kw: it
sys.modules['shapely'].GeometryType = []
sys.modules['segyio'].open = lambda path, *a, **kw: FILES[path]
sys.modules['segyio'].tools = sys.modules['segyio.tools']
sys.modules['segyio.tools'].dt = lambda f, *a, **kw: f.dt_us
import pseudo_3D_interpolation.functions  # noqa: E402

spec = importlib.util.spec_from_file_location('pseudo_3D_interpolation.functions.utils_io',
                                              os.path.join(REF, 'pseudo_3D_interpolation', 'functions', 'utils_IO.py'))
utils_io = importlib.util.module_from_spec(spec)
sys.modules['pseudo_3D_interpolation.functions.utils_io'] = utils_io
spec.loader.exec_module(utils_io)

import pandas as pd  # noqa: E402
from scipy.signal import correlate as scipy_correlate  # noqa: E402
from scipy.stats import pearsonr  # noqa: E402

import mistie_numpy as H  # noqa: E402
from pseudo_3D_interpolation import mistie_correction_segy as ref  # noqa: E402
from pseudo_3D_interpolation.functions.utils import rescale  # noqa: E402

Q = 256.0
LOG = []
ORIGINAL_ENVELOPE = ref.envelope


def logging_envelope(trace, *a, **kw):
    res = ORIGINAL_ENVELOPE(trace, *a, **kw)
    LOG.append((np.array(trace), np.array(res)))
    return res


ref.envelope = logging_envelope


def wavelet(t, f):
    return (1 - 2 * (np.pi * f * t) ** 2) * np.exp(-(np.pi * f * t) ** 2)


def reflectivity(rng, ns, nrefl):
    """A trace of a few wavelets at off-centre positions with distinct amplitudes."""
    t = np.arange(ns, dtype=float)
    x = np.zeros(ns)
    pos = np.sort(rng.choice(np.arange(40, ns - 60), nrefl, replace=False))
    for p, amp in zip(pos, rng.uniform(20, 60, nrefl)):              # positive: mean(rescale) of such a trace stays near 0.3
        x += amp * wavelet(t - p - 0.37, 0.09)
    return x


def shifted(x, d):
    out = np.zeros_like(x)
    if d >= 0:
        out[d:] = x[:x.size - d]
    else:
        out[:d] = x[-d:]
    return out


def margin_ok(a, b, shift):
    """The winning lag of the float64 direct correlation beats every other lag by 1e-4 of itself, and gives ``shift``."""
    n, s, r, cc = H.xcorr(a, b)
    k = n // 2 - s
    assert s == shift, (s, shift)
    others = np.delete(cc, k)
    gap = np.min(np.abs(cc[k]) - np.abs(others)) if others.size else np.inf
    assert gap >= 1e-4 * abs(cc[k]), ('a near-tie decides the shift', gap, cc[k])
    return n, r


def survey_case(name, seed, env, win, quality, delays, dt=0.25, ns=200, ntr=6):
    """Four lines 0 ... 3, every pair crossing once.  Line L sits ``TRUE[L]`` samples deep; the crossing of (i, j) shows one reflectivity on
    both lines, each at its line's depth.  One crossing is noise on one side (rejected by quality).  Line 1 has a bad (noisy, high-mean) trace at
    its crossing with line 0 in the middle of the file, line 2 one at trace 0."""
    rng = np.random.default_rng(seed)
    TRUE = [0, -4, 3, 6]
    nlines = len(TRUE)
    tag = '_env' if env else ''
    files = [f'line{L}_UTM60S{tag}.sgy' for L in range(nlines)]
    data = [rng.normal(0, 0.5, (ntr, ns)) for _ in range(nlines)]
    pairs = [(i, j) for i in range(nlines) for j in range(i + 1, nlines)]
    # trace of every crossing on either line; (0, 1) on line 1 is at trace 3 (a bad trace, mixing of 2 and 4); (0, 2) on line 2 at trace 0
    trace_of = {p: [1 + k % (ntr - 2), 1 + (k + 2) % (ntr - 2)] for k, p in enumerate(pairs)}
    trace_of[(0, 1)] = [1, 3]
    trace_of[(0, 2)] = [2, 0]
    trace_of[(1, 2)] = [1, 4]
    trace_of[(1, 3)] = [5, 2]
    trace_of[(2, 3)] = [2, 4]
    trace_of[(0, 3)] = [4, 1]
    used = set()
    for p in pairs:
        for side in range(2):
            key = (p[side], trace_of[p][side])
            assert key not in used, key
            used.add(key)
    noisy = (1, 3)
    for p in pairs:
        refl = reflectivity(rng, ns, 5)
        for side in range(2):
            L, tr = p[side], trace_of[p][side]
            x = shifted(refl, 10 + TRUE[L] - (round(delays[L] / dt)))
            if p == noisy and side == 1:
                x = reflectivity(rng, ns, 7)
            data[L][tr] = x + rng.normal(0, 0.3, ns)
    # bad traces: a strong positive bias makes mean(rescale) large; their neighbours carry the signal instead
    for (L, tr, p, side) in ((1, 3, (0, 1), 1), (2, 0, (0, 2), 1)):
        good = data[L][tr].copy()
        data[L][tr] = 50 + rng.normal(0, 1, ns)
        data[L][tr][rng.integers(0, ns)] = -60
        if tr == 0:
            data[L][1] = good                    # the clipped slice [0, 2): row 1 is deleted, the bad trace itself remains
        else:
            data[L][tr - 1] = good + rng.normal(0, 0.2, ns)
            data[L][tr + 1] = good + rng.normal(0, 0.2, ns)
    if env:                                      # files of envelopes: non-negative, exact zeros at the ends and in the middle
        for L in range(nlines):
            data[L] = np.abs(data[L]) + 1 / Q
            data[L][:, :7 + L] = 0
            data[L][:, ns - 5 - L:] = 0
            data[L][:, 90 + 3 * L:93 + 3 * L] = 0
        # the clipped bad trace stays bad as an envelope file: a high plateau
    sections = [(np.rint(d * Q) / Q).astype(np.float32) for d in data]
    seg_dir = f'/fixture/{name}'
    for L in range(nlines):
        FILES[os.path.join(seg_dir, files[L])] = FakeFile(sections[L], dt, delays[L])
    lookup = pd.DataFrame({'line': files, 'line_core': [f'line{L}' for L in range(nlines)]}).set_index('line_core')
    names = np.array([[f'line{i}', f'line{j}'] for i, j in pairs], dtype=object)
    idx = np.array(pairs)
    near = [np.array([[trace_of[p][side], 0.0] for p in pairs], np.float32) for side in range(2)]

    del LOG[:]
    loaded = []
    original_load = ref.load_trace

    def logging_load(path, idx_tr, **kw):
        res = original_load(path, idx_tr, **kw)
        loaded.append((path, idx_tr, np.array(res[0])))
        return res

    ref.load_trace = logging_load
    try:
        (offsets, residuals), offsets_ms, coeffs = ref.compute_misties(seg_dir, names, idx, near[0], near[1], win=win, quality=quality, lookup_df=lookup,
                                                                       lookup_col='line', check_bad_traces=True, ntraces2mix=3, return_ms=True,
                                                                       return_coeff=True, verbosity=0)
    finally:
        ref.load_trace = original_load
    assert len(loaded) == 2 * len(pairs) and (env or len(LOG) == 2 * len(pairs))
    rec = dict(files=np.array(files), pairs=idx, traces=np.array([trace_of[p] for p in pairs]), delays=np.array(delays, float), dt=np.float64(dt),
               quality=np.float64(quality), win=np.array([float(w) for w in win]), env=np.array(env), offsets=offsets, offsets_ms=offsets_ms,
               residuals=np.asarray(residuals), coeffs_kept=coeffs)
    for L in range(nlines):
        rec[f'section{L}'] = sections[L]
    # per crossing: repeat the reference's window and zero rules on what its load_trace returned, with its own correlate / rule / pearsonr
    k = len(pairs)
    loaded_tr = np.stack([t for _, _, t in loaded]).reshape(k, 2, ns)
    raw_in = np.stack([t for t, _ in LOG]).reshape(k, 2, ns) if not env else loaded_tr.copy()
    ranges, nleft, shifts, c32, c64, mixed = np.zeros((k, 4), np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k), []
    for c, p in enumerate(pairs):
        twt = [FILES[os.path.join(seg_dir, files[L])].samples for L in p]
        up, lo = win
        if not all([up, lo]):
            up, lo = max(twt[0].min(), twt[1].min()), min(twt[0].max(), twt[1].max())
        up, lo = max(up, twt[0].min(), twt[1].min()), min(lo, twt[0].max(), twt[1].max())
        m = [(t >= up) & (t <= lo) for t in twt]
        for side in range(2):
            ranges[c, 2 * side:2 * side + 2] = np.flatnonzero(m[side])[0], m[side].sum()
            assert np.array_equal(np.flatnonzero(m[side]), ranges[c, 2 * side] + np.arange(ranges[c, 2 * side + 1]))
        t0, t1 = loaded_tr[c, 0][m[0]], loaded_tr[c, 1][m[1]]
        z = (t0 == 0) | (t1 == 0)
        t0, t1 = t0[~z], t1[~z]
        nleft[c] = t0.size
        shifts[c] = ref.cross_correlation_shift(scipy_correlate(t0, t1, mode='same', method='fft'))
        c32[c] = pearsonr(t0, t1)[0]
        c64[c] = pearsonr(t0.astype(np.float64), t1.astype(np.float64))[0]
        n, r = margin_ok(t0, t1, shifts[c])
        assert n == nleft[c] and abs(r - c64[c]) < 1e-12
        assert abs(abs(c32[c]) - quality) > 1e-3, ('a coefficient at the quality threshold', c32[c])
    for (path, idx_tr, _) in loaded:
        f = FILES[path]
        mean = float(np.mean(rescale(f.trace[idx_tr])))
        assert abs(mean - 0.4) > 1e-3, ('a bad-trace mean at its threshold', mean)
        mixed.append(mean > 0.4)
    mixed = np.array(mixed).reshape(k, 2)
    mask = np.abs(c32) >= quality
    assert np.array_equal(c32[mask], coeffs) and mask.any() and (~mask).any(), mask
    assert mixed[pairs.index((0, 1)), 1] and mixed[pairs.index((0, 2)), 1] and mixed.sum() == 2, mixed
    # least squares again, unrounded
    A = np.zeros((mask.sum(), nlines), np.int32)
    A[np.arange(mask.sum()), idx[mask][:, 0]] = 1
    A[np.arange(mask.sum()), idx[mask][:, 1]] = -1
    unrounded = np.linalg.lstsq(A, shifts[mask].astype(np.int16), rcond=None)[0]
    assert np.array_equal(np.around(unrounded, 0).astype('int16'), offsets)
    assert np.all(np.abs(np.abs(unrounded - np.floor(unrounded)) - 0.5) > 1e-6), unrounded
    assert np.array_equal(offsets_ms, offsets * dt)
    # tolerance of the coefficients behind an envelope that is 1e-5 (relative L2) off
    tol = 0.0
    prng = np.random.default_rng(seed + 1000)
    for _ in range(32):
        for c in range(k):
            pert = []
            for side in range(2):
                x = loaded_tr[c, side].astype(np.float64)
                e = prng.standard_normal(ns)
                pert.append(x + e * (1e-5 * np.linalg.norm(x) / np.linalg.norm(e)))
            w0 = pert[0][ranges[c, 0]:ranges[c, 0] + ranges[c, 1]]
            w1 = pert[1][ranges[c, 2]:ranges[c, 2] + ranges[c, 3]]
            z = (loaded_tr[c, 0][ranges[c, 0]:ranges[c, 0] + ranges[c, 1]] == 0) | (loaded_tr[c, 1][ranges[c, 2]:ranges[c, 2] + ranges[c, 3]] == 0)
            tol = max(tol, abs(pearsonr(w0[~z], w1[~z])[0] - c64[c]))
    rec.update(raw=raw_in.astype(np.float32), envelopes=loaded_tr.astype(np.float32), ranges=ranges, n=nleft, shifts=shifts, coeff32=c32, coeff64=c64,
               mask=mask, mixed=mixed, unrounded=unrounded, coeff_tol=np.float64(10 * tol))
    print(f'{name}: shifts {shifts.tolist()}, |coeff| {np.round(np.abs(c32), 3).tolist()}, kept {mask.sum()} of {k}, offsets {offsets.tolist()}, '
          f'unrounded {np.round(unrounded, 3).tolist()}, n {nleft.tolist()}, coeff_tol {10 * tol:.2e}')
    return rec


def kernel_case(seed, n, signed=False, zeros=False, shift=3):
    """Two windows whose compacted length is n, the second the first one moved by ``shift`` samples (plus a little noise)."""
    rng = np.random.default_rng(seed)
    if n == 1:
        a, b = np.array([3.0]), np.array([2.0])                           # one lag: shift 0; r = 0 / 0
    elif n == 2:
        a, b = np.array([2.0, 1.0]), np.array([1.0, 2.0])                 # cc = [a0 b1, a0 b0 + a1 b1] = [4, 4]: the first lag wins, shift 1; r = -1
    else:
        t = np.arange(n + 40, dtype=float)
        x = np.zeros(n + 40)
        for p, amp in zip(rng.choice(np.arange(10, n + 20), max(2, n // 40), replace=False), rng.uniform(20, 60, max(2, n // 40))):
            x += amp * wavelet(t - p - 0.37, 0.09) * (rng.choice([-1, 1]) if signed else 1)
        if signed:                                                       # the second trace is the negative of the first, moved: the minimum wins
            a, b = x[20:20 + n], -x[20 - shift:20 - shift + n]
        else:
            x = np.abs(x) + 0.5
            a, b = x[20:20 + n], x[20 - shift:20 - shift + n]
        a = a + rng.normal(0, 0.05, n)
        b = b + rng.normal(0, 0.05, n)
    a, b = np.rint(a * Q) / Q, np.rint(b * Q) / Q
    a[a == 0] = 1 / Q
    b[b == 0] = 1 / Q
    if zeros:                                                            # zeros at both ends and in the middle, in either trace
        za = np.concatenate([np.zeros(3), a[:n // 2], np.zeros(2), a[n // 2:], np.zeros(4)])
        zb = np.concatenate([np.ones(3), b[:n // 2], np.ones(2), b[n // 2:], np.ones(4)])
        zb[1] = 0
        a, b = za, zb
    a, b = a.astype(np.float32), b.astype(np.float32)
    keep = ~((a == 0) | (b == 0))
    ca, cb = a[keep], b[keep]
    assert ca.size == n
    got_n, s, r, cc = H.xcorr(a, b)
    want = ref.cross_correlation_shift(scipy_correlate(ca, cb, mode='same', method='fft')) if n > 2 else s
    if n > 2:
        margin_ok(a, b, want)
        coeff = pearsonr(ca.astype(np.float64), cb.astype(np.float64))[0]
        assert (cc[n // 2 - s] < 0) == signed
    else:
        coeff = np.nan if n == 1 else pearsonr(ca.astype(np.float64), cb.astype(np.float64))[0]
        assert s == (0 if n == 1 else 1) and (n == 1 or cc[0] == cc[1])
    return dict(a=a, b=b, n=np.int32(n), shift=np.int32(want), coeff64=np.float64(coeff))


out = {}
survey = {
    'raw': dict(seed=11, env=False, win=(False, False), quality=0.5, delays=[0, 5, 0, 0]),
    'raw-win': dict(seed=12, env=False, win=(12.0, 40.0), quality=0.5, delays=[0, 0, 2, 0]),
    'env': dict(seed=13, env=True, win=(False, False), quality=0.5, delays=[0, 0, 0, 3]),
}
for name, kw in survey.items():
    for attempt in range(40):                    # the first seed (in steps of 100) whose sections meet every condition asserted above
        try:
            rec = survey_case(name, **dict(kw, seed=kw['seed'] + 100 * attempt))
            break
        except AssertionError as err:
            print(f'{name}: seed {kw["seed"] + 100 * attempt} rejected: {str(err)[:100]}')
    else:
        raise SystemExit(f'{name}: no seed met the conditions')
    rec['seed'] = np.int64(kw['seed'] + 100 * attempt)
    for k, v in rec.items():
        out[f'case/{name}/{k}'] = np.asarray(v)
out['cases'] = np.array(list(survey))
# (the seeds below were picked the same way, by hand)
kernel = {'n1': dict(seed=1, n=1), 'n2': dict(seed=2, n=2), 'n63': dict(seed=3, n=63), 'n64': dict(seed=4, n=64, shift=-2), 'n65': dict(seed=5, n=65),
          'n300': dict(seed=6, n=300, shift=7), 'n301': dict(seed=7, n=301, shift=-5), 'n1025': dict(seed=8, n=1025, shift=11),
          'signed': dict(seed=9, n=257, signed=True, shift=4), 'zeros': dict(seed=10, n=130, zeros=True, shift=-3)}
for name, kw in kernel.items():
    rec = kernel_case(**kw)
    for k, v in rec.items():
        out[f'kernel/{name}/{k}'] = np.asarray(v)
    print(f"kernel {name}: n {int(rec['n'])}, shift {int(rec['shift'])}, coeff {float(rec['coeff64']):.6f}")
out['kernels'] = np.array(list(kernel))

# compensate_mistie of the reference on a small section, for offsets -5, 0, 7 and one of ns samples
rng = np.random.default_rng(3)
sec = (np.rint(rng.normal(0, 4, (37, 9)) * Q) / Q).astype(np.float32)
out['shift/section'] = sec
out['shift/offsets'] = np.array([-5, 0, 7, 37, -37])
for m in out['shift/offsets']:
    got = ref.compensate_mistie(sec, int(m), verbosity=0)
    assert got.shape == sec.shape
    out[f'shift/out{int(m)}'] = np.asarray(got, np.float32)
assert not out['shift/out37'].any() and not out['shift/out-37'].any()

flags = []
for action in ref.define_input_args()._actions:
    if action.dest != 'help':
        flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default, required=action.required,
                          choices=None if action.choices is None else list(action.choices), nargs=action.nargs, const=action.const,
                          type=None if action.type is None else action.type.__name__, help=action.help))
out['cli_flags'] = np.array(json.dumps(flags))
out['cli_description'] = np.array(ref.define_input_args().description)
path = os.path.join(HERE, 'mistie.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
