"""Fixtures of step 1 (tests/golden/merge.npz) from the REFERENCE's get_files_to_merge and from pandas, the library its wrapper_merge_segys
leaves the merging to.

    python tests/golden/make_golden_merge.py /path/to/reference

The reference's module imports segyio at module level (its utils dask / xarray); empty stand-ins go into ``sys.modules`` first.
``get_files_to_merge`` is run unchanged on temporary files of chosen sizes.  ``wrapper_merge_segys`` needs segyio files, so the merge is
recorded as what pandas returns for the primitive operations it applies to the table of trace headers [N][91] -- written here in this
script's own words: both ``duplicated`` masks, and the table reindexed onto TRACE_SEQUENCE_LINE, interpolated and cast to int32.

The script asserts what the tests rely on (see the asserts), so that a weak fixture cannot pass silently; and that the NumPy restatement
(tests/helpers/merge_numpy.py) reproduces every recorded result."""
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, '..', 'helpers'))
for name in ('segyio', 'tqdm', 'dask', 'dask.array', 'xarray'):
    sys.modules[name] = types.ModuleType(name)

import merge_numpy as H  # noqa: E402
from pseudo_3D_interpolation import merge_segys as ms  # noqa: E402

ms.xprint = lambda *args, **kw: None
warnings.simplefilter('ignore', FutureWarning)                  # pandas on the reference's positional row[1]
out = {}

# ---- grouping -----------------------------------------------------------------------------------------------------------------------------------------
S, L = 1024, 4096                                               # bytes; the threshold is 2 kB
GROUP_CASES = {
    'none': [L, L, L],
    'middle': [L, S, L],
    'run-of-three': [L, S, S, S, L, L],
    'two-runs': [L, S, L, L, S, S, L],
    'first': [S, L, L],
    'last': [L, L, S],
    'run-to-the-end': [L, S, S],
}
for name, sizes in GROUP_CASES.items():
    with tempfile.TemporaryDirectory() as folder:
        paths = []
        for k, size in enumerate(sizes):
            paths.append(os.path.join(folder, f'{k:02d}_line.sgy'))
            with open(paths[-1], 'wb') as fh:
                fh.write(b'\0' * size)
        try:
            groups = [[paths.index(p) for p in g] for g in ms.get_files_to_merge(paths, fsize_kB=2, verbosity=0)]
            failed = False
        except Exception as err:  # noqa: BLE001 -- the reference cannot handle a list without a small file
            groups, failed = [], True
            print(f'grouping {name}: the reference raised {type(err).__name__}: {err}')
    out[f'group/{name}'] = np.array(json.dumps(dict(sizes=sizes, groups=groups, reference_failed=failed)))
    print(f'grouping {name}: {sizes} -> {groups}')
    expected = []
    k = 0
    while k < len(sizes):                                       # the rule the issue states: a run of small files plus the file behind it
        if sizes[k] == S:
            j = k
            while j + 1 < len(sizes) and sizes[j + 1] == S:
                j += 1
            expected.append(list(range(k, min(j + 2, len(sizes)))))
            k = j + 1
        else:
            k += 1
    assert groups == expected, (name, groups, expected)
assert json.loads(str(out['group/none']))['reference_failed'] and not json.loads(str(out['group/middle']))['reference_failed']
assert json.loads(str(out['group/last']))['groups'] == [[2]] and json.loads(str(out['group/run-to-the-end']))['groups'] == [[1, 2]]
out['group/cases'] = np.array(list(GROUP_CASES))

# ---- the header table -----------------------------------------------------------------------------------------------------------------------------------
NAMES = ['TRACE_SEQUENCE_LINE', 'TRACE_SEQUENCE_FILE'] + [f'word{j:02d}' for j in range(2, 91)]
BIG = 2**31 - 1
rng = np.random.default_rng(1)
LINE = [10, 12, 13, 14, 14, 15, 16, 16, 17, 21, 22, 24]        # TRACE_SEQUENCE_LINE in file order
N = len(LINE)
table = np.empty((N, 91), np.int64)
for j, w in enumerate(H.WIDTHS):
    table[:, j] = rng.integers(-2**31, 2**31, N) if w == 4 else rng.integers(-2**15, 2**15, N)
table[:, 0] = LINE
table[:, 1] = np.arange(1, N + 1)
table[4] = table[3]                                             # an exact pair, TRACE_SEQUENCE_FILE included: both go
table[7] = table[6]
table[7, 1] = 99                                                # a pair that differs in TRACE_SEQUENCE_FILE only: the second goes
four = np.flatnonzero(H.WIDTHS == 4)[2:]
table[8, four[0::2]], table[9, four[0::2]] = BIG, -BIG          # +-(2^31 - 1) across the gap of three rows 18 ... 20
table[8, four[1::2]], table[9, four[1::2]] = -BIG, BIG
table[8, four[-1]], table[9, four[-1]] = BIG, BIG - 1
two = np.flatnonzero(H.WIDTHS == 2)
table[0, two[0]], table[1, two[0]] = -32768, 32767
table[10, two[1]], table[11, two[1]] = -1, -2
table[0, four[0]], table[1, four[0]] = -5, -2                   # halves of negative numbers: the cast truncates toward zero
out['table'] = table.astype(np.int32)

df = pd.DataFrame(table.astype(np.int32), columns=NAMES)
df.set_index(df['TRACE_SEQUENCE_LINE'], inplace=True)
overlapping = df.duplicated(keep='last').to_numpy()
internal = df.duplicated(subset=[c for c in NAMES if c != 'TRACE_SEQUENCE_FILE'], keep='first').to_numpy()
mask = overlapping | internal
kept = df[~mask]
first, last = int(kept.iloc[0]['TRACE_SEQUENCE_LINE']), int(kept.iloc[-1]['TRACE_SEQUENCE_LINE'])
wide = kept.reindex(pd.RangeIndex(first, last + 1))
gaps = pd.isnull(wide).any(axis=1).to_numpy()
merged = wide.interpolate(method='linear').astype('int32')
merged['TRACE_SEQUENCE_FILE'] = np.arange(1, merged.shape[0] + 1)
merged = merged.to_numpy()
out['overlapping'], out['internal'], out['gaps'], out['merged'] = overlapping, internal, gaps, merged.astype(np.int32)
print('overlapping', overlapping.astype(int), '\ninternal   ', internal.astype(int), '\ngaps       ', gaps.astype(int))

# what the tests rely on
assert overlapping.tolist() == [i == 3 for i in range(N)] and internal.tolist() == [i in (4, 7) for i in range(N)]
assert gaps.tolist() == [r in (1, 4, 8, 9, 10, 13) for r in range(15)]         # after the first row, before the last, lengths 1 and 3
assert gaps[1] and gaps[-2] and not gaps[0] and not gaps[-1]
rows = dict(zip(range(first, last + 1), merged))
assert np.all(np.abs(rows[17][four[:-1]]) == BIG) and np.all(rows[17][four[:-1]] == -rows[21][four[:-1]])
assert np.all(rows[19][four[:-1]] == 0) and np.all(np.abs(rows[18][four[:-1]]) == 2**30 - 1)
assert rows[11][four[0]] == -3 and rows[23][two[1]] == -1                      # -3.5 -> -3, -1.5 -> -1: toward zero
for width in (2, 4):
    cols = np.flatnonzero(H.WIDTHS == width)[2:] if width == 4 else np.flatnonzero(H.WIDTHS == width)
    assert (merged[gaps][:, cols] < 0).any() and (merged[~gaps][:, cols] < 0).any(), width
assert merged[:, 1].tolist() == list(range(1, 16))

# the restatement reproduces pandas
headers = H.headers_of(table)
assert np.array_equal(H.words_of(headers), table)
h_over, h_int = H.duplicate_masks(headers)
assert np.array_equal(h_over, overlapping) and np.array_equal(h_int, internal)
src, lo, hi = H.plan(H.keys(headers)[0], h_over | h_int)
assert np.array_equal(src < 0, gaps)
assert np.array_equal(H.merged_words(table, src, lo, hi), merged)
out['src'], out['lo_row'], out['hi_row'] = src, lo, hi

flags = []
for action in ms.define_input_args()._actions:
    if action.dest != 'help':
        flags.append(dict(dest=action.dest, flags=list(action.option_strings), default=action.default,
                          choices=None if action.choices is None else list(action.choices), nargs=action.nargs,
                          type=None if action.type is None else action.type.__name__))
out['cli_flags'] = np.array(json.dumps(flags))
path = os.path.join(HERE, 'merge.npz')
np.savez_compressed(path, **out)
print(os.path.getsize(path), 'bytes')
