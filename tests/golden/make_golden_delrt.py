"""Fixtures of steps 3 and 4 (tests/golden/delrt.npz) from the REFERENCE's own pad_trace_data, correct_single_trace_DelayRecordingTime and
check_DelayRecordingTime_changes.

    python tests/golden/make_golden_delrt.py /path/to/reference

The reference's modules import segyio and tqdm at module level (its utils dask / xarray, the correction script its plot module, which needs
matplotlib); empty stand-ins go into ``sys.modules`` first.  The functions are run unchanged.  What the correction function computes on the way
is visible only in its debug messages: ``xprint`` is replaced by a recorder, and the NumPy restatement of the kernels (tests/helpers/delrt_numpy.py)
must reproduce the messages about the peak and the clipped maxima character by character (all samples are multiples of 1/512, so the four
decimals of the message tell any two values apart).  ``check_DelayRecordingTime_changes`` is given a stand-in for the open segyio file.

Recorded: padding cases (input, delays, dt and everything pad_trace_data returns), the decision table (window maxima, delays and what the
reference returned), section cases (profile, header delays, per examined change the peak, the clipped maxima and the result) and both parsers'
flags.  The script asserts what the tests rely on (see the asserts), so that a weak fixture cannot pass silently."""
import itertools
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, '..', 'helpers'))
for name in ('segyio', 'tqdm', 'dask', 'dask.array', 'xarray', 'pseudo_3D_interpolation.functions.plot'):
    mod = types.ModuleType(name)
    mod.tqdm = lambda it, **kw: it
    mod.plot_seismic_wiggle = None
    sys.modules[name] = mod
sys.modules['segyio'].TraceField = types.SimpleNamespace(TRACE_SEQUENCE_FILE=5, FieldRecord=9, DelayRecordingTime=109)

import delrt_numpy as H  # noqa: E402
from pseudo_3D_interpolation import delrt_correction_segy as dcs  # noqa: E402
from pseudo_3D_interpolation import delrt_padding_segy as dps  # noqa: E402

Q = 512.0
MESSAGES = []
dcs.xprint = lambda *args, **kw: MESSAGES.append(' '.join(str(a) for a in args))
dps.xprint = lambda *args, **kw: None
out = {}


# ---- padding ----------------------------------------------------------------------------------------------------------------------------------------
BASE = [10] * 7 + [40] * 5 + [25] * 6 + [10] * 3
PAD_CASES = {
    'base': (BASE, 400, 0.25),
    'dt0.05': (BASE, 400, 0.05), 'dt0.0625': (BASE, 400, 0.0625), 'dt0.1': (BASE, 400, 0.1), 'dt0.125': (BASE, 400, 0.125), 'dt0.3': (BASE, 400, 0.3),
    'ns397': (BASE, 397, 0.25), 'ns3': (BASE, 3, 0.25),
    'ends-differ': ([10] * 7 + [40] * 5 + [25] * 6 + [30] * 3, 400, 0.25),
    'odd': ([10, 10, 13, 13, 13, 11, 11, 15, 12], 37, 1.0),
    'two': ([10, 20], 50, 0.25),
}
rng = np.random.default_rng(3)
pad_section = (rng.integers(-64, 65, (400, len(BASE))) / Q).astype(np.float32)
pad_section[0] = np.where(pad_section[0] == 0, 1 / Q, pad_section[0])      # the ends of every trace can be told from the padding
out['pad/section'] = pad_section
residues, rolled, unrolled, any_top0, any_bottom0 = set(), 0, 0, False, False
for name, (delays, ns, dt) in PAD_CASES.items():
    delays = np.array(delays)
    data = pad_section[:ns, :delays.size].copy()
    data[-1] = np.where(data[-1] == 0, 1 / Q, data[-1])
    twt = np.arange(ns) * dt + delays[0]                                     # segyio's sample axis: t0 of the first trace
    padded, twt_padded, n_padded, (idx_delay, dmin, dmax) = dps.pad_trace_data(data, delays, delays.size, dt, twt)
    assert padded.dtype == np.float32 and padded.shape == (n_padded, delays.size) and n_padded == twt_padded.size
    top = np.array([np.flatnonzero(padded[:, x])[0] for x in range(delays.size)])
    bottom = n_padded - ns - top
    assert np.array_equal(H.pad(data, top, n_padded), padded), name
    residues |= set((top % 4).tolist())
    any_top0 |= bool(np.any(top == 0))
    any_bottom0 |= bool(np.any(bottom == 0))
    if delays[0] == delays[-1]:
        rolled += 1
    else:
        unrolled += 1
    for k, v in dict(delays=delays, ns=ns, dt=np.float64(dt), data_padded=padded, twt_padded=twt_padded, n_samples_padded=n_padded, idx_delay=idx_delay,
                     min_delay=dmin, max_delay=dmax, top=top).items():
        out[f'pad/{name}/{k}'] = np.asarray(v)
    print(f'pad {name}: {ns} -> {n_padded} samples, top {sorted(set(top.tolist()))}, bottom {sorted(set(bottom.tolist()))}')
assert out['pad/base/n_samples_padded'] == 520
assert residues == {0, 1, 2, 3} and any_top0 and any_bottom0 and rolled >= 1 and unrolled >= 1
out['pad/cases'] = np.array(list(PAD_CASES))


# ---- the correction function with its messages ------------------------------------------------------------------------------------------------------
BRANCHES = dict(none='<<< No correction needed >>>', wrong='*** Incorrect DelayRecordingTime! ***', eligible='Eligible for adjusting offset trace',
                offset='*** [OFFSET TRACE] Incorrect DelayRecordingTime! ***', refusal='Found more than one DelayRecordingTime to choose from. No changes applied.')
fired = dict.fromkeys(list(BRANCHES) + ['before', 'after', 'boundary', 'exit'], 0)
closest = [1.0]


def run_reference(data, delrt, n_traces, n_samples):
    """The reference on one subset (samples x traces).  Returns (peak_idx, peak_val, raw maxima, clipped maxima, kind, delay, index) with kind 0:
    (None, None), 1: (delay, index), 2: SystemExit."""
    del MESSAGES[:]
    try:
        delay, index = dcs.correct_single_trace_DelayRecordingTime(0, data, delrt.copy(), np.arange(delrt.size), n_traces, n_samples, verbosity=2)
        kind = 0 if delay is None else 1
    except SystemExit:
        delay, index, kind = None, None, 2
        fired['exit'] += 1
    # the restatement of the kernel reproduces what the reference saw
    width = data.shape[1]
    full = data if width == 2 * n_traces + 1 else np.concatenate([data, data[:, -1:]], axis=1)     # a subset one trace short: filled up
    peak_idx, peak_val, maxima = H.windows(full, [n_traces], n_traces, n_samples)
    peak_idx, peak_val, maxima = int(peak_idx[0]), peak_val[0], maxima[0, :width]
    clipped = np.minimum(maxima, maxima[n_traces])
    assert MESSAGES[0] == f'ref_tr_peak_idx:  {peak_idx} --> {peak_val}', (MESSAGES[0], peak_idx, peak_val)
    assert MESSAGES[1] == f'tr_amp_maxima:          {np.around(clipped, 4)}', (MESSAGES[1], clipped)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.abs(clipped - peak_val) / peak_val
    if np.any(np.isfinite(rel)):
        closest[0] = min(closest[0], float(np.min(np.abs(rel[np.isfinite(rel)] - 0.8))))
    for key, text in BRANCHES.items():
        fired[key] += any(text in m for m in MESSAGES)
    if any(BRANCHES['offset'] in m for m in MESSAGES) and kind == 1:
        fired['before' if index < n_traces else 'after'] += 1
    if any(BRANCHES['eligible'] in m for m in MESSAGES) and not any(BRANCHES['offset'] in m for m in MESSAGES):
        fired['boundary'] += 1
    return peak_idx, peak_val, maxima, clipped, kind, (0 if delay is None else delay), (-1 if index is None else index)


# ---- decision table -----------------------------------------------------------------------------------------------------------------------------------
def subset_of(bits, n_traces, width):
    """16 samples x ``width`` traces: the reference trace peaks at row 8 with 1.0; a neighbour with bit 0 peaks there too (with 1.0, or with 1.5 on
    odd positions: clipped), one with bit 1 holds 1/512 at most."""
    data = np.zeros((16, width), np.float32)
    data[3] = 1 / Q
    neighbours = [j for j in range(width) if j != n_traces]
    data[8, n_traces] = 1.0
    for j, b in zip(neighbours, bits):
        if not b:
            data[8, j] = 1.5 if j % 2 else 1.0
    return data


rows = []
for n in (1, 2, 3):
    for width in (2 * n + 1, 2 * n):                           # the whole subset, and the one the reference cuts at the end of the file
        two = [[a] * k + [b] * (width - k) for k in range(1, width) for a, b in ((10, 30), (30, 10))]
        three = [[10] * k + [30] * (width - k - 1) + [20] for k in range(1, width - 1)] + [[20] + [10] * k + [30] * (width - k - 1) for k in range(1, width - 1)]
        for bits in itertools.product((0, 1), repeat=width - 1):
            for delays in two + three:
                delrt = np.array(delays)
                data = subset_of(bits, n, width)
                _, peak_val, maxima, _, kind, delay, index = run_reference(data, delrt, n, 4)
                rows.append((n, width, maxima, peak_val, delrt, kind, delay, index))
W = 7
table = dict(n_traces=[], width=[], maxima=[], peak_val=[], delrt=[], kind=[], delay=[], index=[])
for n, width, maxima, peak_val, delrt, kind, delay, index in rows:
    table['n_traces'].append(n)
    table['width'].append(width)
    table['maxima'].append(np.pad(maxima, (0, W - width)))
    table['peak_val'].append(peak_val)
    table['delrt'].append(np.pad(delrt, (0, W - width)))
    table['kind'].append(kind)
    table['delay'].append(delay)
    table['index'].append(index)
for k, v in table.items():
    out[f'table/{k}'] = np.array(v, dtype=np.float32 if k in ('maxima', 'peak_val') else np.int32)
print(f'decision table: {len(rows)} rows, fired {fired}')
for key in ('none', 'wrong', 'before', 'after', 'boundary', 'refusal'):
    assert fired[key] >= 1, key
out['table/exit_fired'] = np.array(fired['exit'])               # 0: the reference's sys.exit cannot be reached with n_traces <= 3


# ---- section cases: check_DelayRecordingTime_changes on a stand-in for the open file -----------------------------------------------------------------
class FakeFile:
    def __init__(self, section, delrt, dt):
        ntr, ns = section.shape
        self.samples = np.arange(ns) * dt + delrt[0]
        self.trace = types.SimpleNamespace(raw=section)
        self._attr = {5: np.arange(1, ntr + 1), 9: np.arange(ntr) + 100, 109: np.asarray(delrt)}
        self.header = None

    def attributes(self, key):
        return self._attr[key]


LOG = []
ORIGINAL = dcs.correct_single_trace_DelayRecordingTime


def logging_correct(idx, data, delrt, fldr, n_traces=5, n_samples=120, verbosity=0):
    LOG.append((int(idx), np.array(data), np.array(delrt)))
    return ORIGINAL(idx, data, delrt, fldr, n_traces, n_samples, verbosity)


def profile(seed, ntr, ns, dt, data_delay, arrival_ms=40.0):
    """Samples x traces: noise of a few 1/512 and a three-sample wavelet at the row of ``arrival_ms`` in the trace's TRUE recording window."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-4, 5, (ns, ntr)) / Q
    for x in range(ntr):
        row = int(round((arrival_ms - data_delay[x]) / dt))
        amp = (512 + int(rng.integers(-20, 21))) / Q
        a[row, x] += amp
        if row + 1 < ns:
            a[row + 1, x] -= 0.5
        if row - 1 >= 0:
            a[row - 1, x] += 0.25
    return a.astype(np.float32)


def jump(ntr, at, first=10, second=30):
    return np.array([first] * at + [second] * (ntr - at))


NTR, NS, DT = 60, 300, 0.25
SECTION_CASES = {}
SECTION_CASES['clean'] = (profile(1, NTR, NS, DT, jump(NTR, 30)), jump(NTR, 30), 5, 120)
SECTION_CASES['late-header'] = (profile(2, NTR, NS, DT, jump(NTR, 30)), jump(NTR, 31), 5, 120)
SECTION_CASES['early-header'] = (profile(3, NTR, NS, DT, jump(NTR, 31)), jump(NTR, 30), 5, 120)
d = jump(NTR, 30)
d[31] = 10                                                                   # one trace behind the jump is still recorded in the old window
SECTION_CASES['offset-after'] = (profile(4, NTR, NS, DT, d), jump(NTR, 30), 5, 120)
d = jump(NTR, 30)
d[28] = 30                                                                   # one trace before the jump is already recorded in the new window
SECTION_CASES['offset-before'] = (profile(5, NTR, NS, DT, d), jump(NTR, 29), 5, 120)
ends = np.array([10] * 3 + [30] * 27 + [10] * 25 + [30] * 5)                # changes at 3 (skipped), 30, 55 = ntr - n_traces (a subset one trace short)
SECTION_CASES['ends'] = (profile(6, NTR, NS, DT, ends), ends, 5, 120)
ends2 = np.array([10] * 30 + [30] * 27 + [10] * 3)                          # a change at ntr - 3: skipped
SECTION_CASES['end-skipped'] = (profile(7, NTR, NS, DT, ends2), ends2, 5, 120)
three = np.array([10] * 28 + [20] * 4 + [30] * 28)
SECTION_CASES['three-delays'] = (profile(8, NTR, NS, DT, three), three, 5, 120)
SECTION_CASES['narrow'] = (profile(9, 24, NS, DT, jump(24, 13)), jump(24, 12), 2, 7)   # other window sizes; an early header
SECTION_CASES['peak-first-row'] = (profile(11, 20, 50, DT, jump(20, 10, 30, 40)), jump(20, 10, 30, 40), 3, 9)    # trace 10: arrival at row 0
last = profile(12, 20, 50, DT, jump(20, 10, 35, 27.75))                     # trace 10: arrival at row 49, the last one
SECTION_CASES['peak-last-row'] = (last, jump(20, 10, 35, 28), 3, 9)
tie = profile(13, 20, 50, DT, jump(20, 10, 30, 35))
tie[40, 10] = tie[:, 10].max()                                               # trace 10 holds its maximum twice: rows 20 and 40, the first wins
SECTION_CASES['tie'] = (tie, jump(20, 10, 30, 35), 3, 9)
neg = profile(14, 20, 50, DT, jump(20, 10, 30, 35))
neg[:, 8] = -np.abs(neg[:, 8]) - 1 / Q                                       # an all-negative neighbour
SECTION_CASES['negative-neighbour'] = (neg, jump(20, 10, 30, 35), 3, 9)
zero = profile(15, 20, 50, DT, jump(20, 10, 30, 35))
zero[:, 10] = 0                                                              # an all-zero reference trace: 0 / 0
SECTION_CASES['zero-reference'] = (zero, jump(20, 10, 30, 35), 3, 9)

dcs.correct_single_trace_DelayRecordingTime = logging_correct
for name, (data, delrt, n_traces, n_samples) in SECTION_CASES.items():
    del LOG[:]
    section = np.ascontiguousarray(data.T)
    assert dcs.check_DelayRecordingTime_changes(FakeFile(section, delrt, DT), delrt.size, 109, n_traces, n_samples, update_segy=False, verbosity=2) is True
    rec = dict(idx=[], width=[], peak_idx=[], peak_val=[], maxima=[], kind=[], delay=[], index=[])
    for idx, subset, delrt_subset in list(LOG):
        peak_idx, peak_val, _, clipped, kind, delay, index = run_reference(subset, delrt_subset, n_traces, n_samples)
        assert kind != 2
        rec['idx'].append(idx)
        rec['width'].append(subset.shape[1])
        rec['peak_idx'].append(peak_idx)
        rec['peak_val'].append(peak_val)
        rec['maxima'].append(np.pad(clipped, (0, 2 * n_traces + 1 - clipped.size)))
        rec['kind'].append(kind)
        rec['delay'].append(delay)
        rec['index'].append(index)
    out[f'section/{name}/data'] = data
    out[f'section/{name}/delrt'] = delrt
    out[f'section/{name}/window'] = np.array([n_traces, n_samples])
    for k, v in rec.items():
        shape = (len(rec['idx']), 2 * n_traces + 1) if k == 'maxima' else (len(rec['idx']),)
        out[f'section/{name}/{k}'] = np.array(v, dtype=np.float32 if k in ('peak_val', 'maxima') else np.int32).reshape(shape)
    print(f"section {name}: changes examined {rec['idx']}, peaks {rec['peak_idx']}, results {list(zip(rec['kind'], rec['delay'], rec['index']))}")
out['section/cases'] = np.array(list(SECTION_CASES))


def results(name):
    return [(int(i), int(k), int(d), int(x)) for i, k, d, x in zip(*(out[f'section/{name}/{key}'].ravel() for key in ('idx', 'kind', 'delay', 'index')))]


assert results('clean') == [(30, 0, 0, -1)]
assert results('early-header') == [(30, 1, 10, 5)]                           # the wrong-delay branch: trace 30 belongs to the old window
assert results('offset-after') == [(30, 1, 10, 6)] and results('offset-before') == [(29, 1, 30, 4)]
assert [r[0] for r in results('ends')] == [30, 55] and out['section/ends/width'].ravel().tolist() == [11, 10]
assert [r[0] for r in results('end-skipped')] == [30] and results('three-delays') == []
assert out['section/peak-first-row/peak_idx'].ravel().tolist() == [0] and out['section/peak-last-row/peak_idx'].ravel().tolist() == [49]
assert out['section/tie/peak_idx'].ravel().tolist() == [20] and np.all(np.isfinite(out['section/negative-neighbour/maxima']))
assert out['section/negative-neighbour/maxima'][0, 1] < 0 and out['section/zero-reference/peak_val'].ravel().tolist() == [0.0]
assert closest[0] > 1e-3, closest
print(f'closest relative difference to 0.8: {closest[0]:.4f}')

for key, mod in (('correction', dcs), ('padding', dps)):
    flags = []
    for action in mod.define_input_args()._actions:
        if action.dest != 'help':
            flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default,
                              choices=None if action.choices is None else list(action.choices), nargs=action.nargs,
                              type=None if action.type is None else action.type.__name__, help=action.help))
    out[f'cli_flags/{key}'] = np.array(json.dumps(flags))
path = os.path.join(HERE, 'delrt.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
