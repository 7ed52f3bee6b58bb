"""Host side of step 8 (CPU only): the NumPy restatement against the fixtures recorded from the reference's despike_2D, and the host logic of
functions/despike.py (window rows, runs from the packed mask, level assignment) against that restatement."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import despike_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd.functions import despike as D  # noqa: E402

G = load_golden('despike.npz')
CASES = [str(c) for c in G['cases']]


def parse(name):
    sec, window, ov, w, mode, thr, out = name.split('-')
    return G['section/' + sec], dict(window=int(window), dt=1.0, overlap=int(ov), ntraces=int(w), mode=mode, threshold=int(thr), out=out)


def test_fixture_set_covers_what_the_issue_asks():
    kws = [parse(n)[1] for n in CASES]
    assert {(k['mode'], k['out']) for k in kws} >= {(m, o) for m in ('mean', 'median', 'rms') for o in D.REPLACE_AMP_MODES}
    assert {k['ntraces'] for k in kws} >= {3, 5, 7, 21}
    assert {360 % D.window_rows(360, k['window'], 1.0, k['overlap'])[1] == 0 for k in kws} == {True, False}
    assert any(G[f'case/{n}/idx'].size == 0 for n in CASES) and sum(G[f'case/{n}/idx'].size > 0 for n in CASES) >= 30


@pytest.mark.parametrize('name', CASES)
def test_helper_equals_the_reference_bit_for_bit(name):
    a, kw = parse(name)
    idx, val = G[f'case/{name}/idx'], G[f'case/{name}/val']
    want = a.copy().ravel()
    want[idx] = val
    got = H.despike_2D(a, **kw)
    assert got.tobytes() == want.tobytes()


def pack(cand):
    """bool [ns][ntr] -> the kernel's mask uint64 [ntr][ceil(ns / 64)]."""
    ns, ntr = cand.shape
    bits = np.zeros((ntr, (ns + 63) // 64 * 64), np.uint8)
    bits[:, :ns] = cand.T
    return np.packbits(bits, axis=1, bitorder='little').view(np.uint64)


@pytest.mark.parametrize('name', ['spiky-110-10-5-mean-3-zeros', 'spiky-100-10-3-mean-2-zeros', 'spiky-100-10-21-median-6-median',
                                  'spiky-100-10-11-rms-2-scaled', 'quiet-100-10-5-mean-3-zeros'])
def test_runs_from_the_packed_mask(name):
    a, kw = parse(name)
    ns, ntr = a.shape
    M, dy, main_end, add_start = D.window_rows(ns, kw['window'], 1.0, kw['overlap'])
    assert (M, dy, main_end, add_start) == H.window_params(ns, kw['window'], 1.0, kw['overlap'])
    cand = H.candidates(a, kw['ntraces'], kw['mode'], kw['threshold'])
    examined = (np.arange(ns) < main_end) | (np.arange(ns) >= (ns if add_start is None else add_start))
    cand &= examined[:, None]
    counts = np.stack([cand[:main_end].sum(0), cand[add_start:].sum(0) if add_start is not None else np.zeros(ntr, int)]).astype(np.int32)
    rec = D.spikes_from_mask(pack(cand), counts, ns, M, main_end, add_start, kw['ntraces'], chunk=7)
    want = H.find_spikes(a, **{k: v for k, v in kw.items() if k != 'out'})
    assert [tuple(r[:5]) for r in rec.tolist()] == want
    h = kw['ntraces'] // 2
    assert all(r[5] == max(0, r[0] - h) and r[6] == min(ntr, r[0] + h + 1) for r in rec.tolist())


def rec(x, lo, hi, h=2, ntr=100, seg=(0, 100)):
    return (x, lo, hi, lo, hi - 1, max(seg[0], x - h), min(seg[1], x + h + 1), 0)


def test_level_assignment():
    assert D.assign_levels(np.zeros((0, 8), np.int32)).size == 0
    iso = [rec(10, 0, 50), rec(20, 0, 50), rec(30, 10, 40)]
    assert D.assign_levels(iso).tolist() == [0, 0, 0]
    assert D.assign_levels([rec(10, 0, 50), rec(10, 48, 90), rec(10, 89, 99), rec(10, 200, 220)]).tolist() == [0, 1, 2, 0]   # one trace, chained rows
    assert D.assign_levels([rec(10, 0, 50), rec(12, 40, 60), rec(13, 0, 30), rec(14, 55, 70)]).tolist() == [0, 1, 0, 2]        # within h = 2
    assert D.assign_levels([rec(10, 0, 50), rec(13, 0, 50)]).tolist() == [0, 0]                                               # 3 apart: no contact
    assert D.assign_levels([rec(10, 0, 50), rec(12, 50, 60)]).tolist() == [0, 0]                                              # rows touch, no overlap
    # a split boundary between traces 11 and 12: neither reads the other
    assert D.assign_levels([rec(11, 0, 50, seg=(0, 12)), rec(12, 0, 50, seg=(12, 100))]).tolist() == [0, 0]
    # clipped at the right edge: trace 99 reads 97 .. 99, trace 97 reads 95 .. 99
    assert D.assign_levels([rec(97, 0, 50), rec(99, 10, 20)]).tolist() == [0, 1]
    ordered, start = D.order_by_level([rec(10, 0, 50), rec(10, 48, 90), rec(20, 0, 9), rec(10, 89, 99)], [0, 1, 0, 2])
    assert ordered[:, 0].tolist() == [10, 20, 10, 10] and ordered[:, 1].tolist() == [0, 0, 48, 89] and start.tolist() == [0, 2, 3, 4]


def test_sequential_order_equals_levels_on_the_helper():
    """Replacing level by level (any order inside a level) gives what the reference's sequential loop gives."""
    a, kw = parse('spiky-110-10-5-mean-3-median')
    spikes = H.find_spikes(a, **{k: v for k, v in kw.items() if k != 'out'})
    recs = np.array([rec(x, lo, hi) for x, lo, hi, _, _ in spikes], np.int32)
    lev = D.assign_levels(recs)
    assert lev.max() >= 1
    want = H.replace(a.copy(), spikes, 5, 'mean', 3, 'median')
    got = a.copy()
    for l in range(lev.max() + 1):
        src = got.copy()                                        # every spike of the level reads the state before the level
        for k in np.nonzero(lev == l)[0][::-1]:
            tmp = H.replace(src.copy(), [spikes[k]], 5, 'mean', 3, 'median')
            x, lo, hi = spikes[k][:3]
            got[lo:hi, x] = tmp[lo:hi, x]
    assert got.tobytes() == want.tobytes()
    flat = a.copy()                                             # every spike at level 0: all read the untouched section
    for k in range(len(spikes)):
        tmp = H.replace(a.copy(), [spikes[k]], 5, 'mean', 3, 'median')
        x, lo, hi = spikes[k][:3]
        flat[lo:hi, x] = tmp[lo:hi, x]
    assert flat.tobytes() != want.tobytes()                     # ... which is not the reference's result: the fixture bites


def test_checks_of_the_reference():
    a = np.zeros((200, 20), np.float32)
    for kw, msg in [(dict(overlap=101), 'Overlap must be'), (dict(threshold=-1), 'Theshold must be positive'), (dict(ntraces=4), 'must be odd'),
                    (dict(mode='max'), 'Amplitude mode must be'), (dict(out='ones'), 'Output amplitude option')]:
        with pytest.raises(ValueError, match=msg):
            D.despike_2D(a, 100, 1.0, **kw)
    with pytest.raises(ValueError, match='does not fit'):
        D.despike_2D(a, 300, 1.0)
    assert D.split_bounds([0, 5, 5, 12, 20], 20).tolist() == [0, 5, 12, 20]


def test_moving_window_2D_is_the_view_the_reference_describes():
    from pseudo_3d_interpolation_amd.functions.filter import moving_window_2D
    a = np.arange(7 * 9, dtype=np.float32).reshape(7, 9)
    v = moving_window_2D(a, (3, 5), dx=1, dy=2)
    assert v.shape == (3, 5, 3, 5) and not v.flags.writeable and np.shares_memory(v, a)
    for i in range(3):
        for j in range(5):
            np.testing.assert_array_equal(v[i, j], a[2 * i:2 * i + 3, j:j + 5])
