"""NumPy restatement of what the step-5 kernels compute (csrc/p3d_static.hip), written for the tests and for tools/static_rate.py: plain and
slow, sections are samples x traces as in the reference."""
import numpy as np


def compensate_static(data, static_samples):
    """out[t][x] = data[t - s[x]][x] where that row exists, else 0."""
    data = np.asarray(data)
    ns, ntr = data.shape
    out = np.zeros_like(data)
    for x, s in enumerate(np.asarray(static_samples).tolist()):
        if s == 0:
            out[:, x] = data[:, x]
        elif 0 < s < ns:
            out[s:, x] = data[:ns - s, x]
        elif -ns < s < 0:
            out[:ns + s, x] = data[-s:, x]
    return out


def sta_lta_ratio(trace, nsta, nlta):
    """STA/LTA ratio of one trace with the running sums in double."""
    c = np.cumsum(np.asarray(trace, dtype=np.float64) ** 2)
    sta, lta = c.copy(), c.copy()
    sta[nsta:] -= c[:-nsta]
    lta[nlta:] -= c[:-nlta]
    sta /= nsta
    lta /= nlta
    sta[:nlta - 1] = 0
    ratio = np.zeros_like(c)
    np.divide(sta, lta, out=ratio, where=lta != 0)
    return ratio


def first_nonzero(data):
    """First non-zero sample of every trace, -1 for zero traces."""
    nz = data != 0
    return np.where(nz.any(axis=0), nz.argmax(axis=0), -1)


def detect(data, nsta, nlta, threshold=None, nso=None):
    """(first, threshold, raw crossings of all traces; 0 for zero traces)."""
    ns, ntr = data.shape
    first = first_nonzero(data)
    ratios = {}
    for x in np.flatnonzero(first >= 0):
        lo = first[x] if nso is not None else 0
        ratios[x] = sta_lta_ratio(data[lo:lo + (nso or ns), x], nsta, nlta)
    if threshold is None:
        threshold = max(r[nlta:2 * nlta].max() for r in ratios.values())
    raw = np.zeros(ntr, dtype=int)
    for x, r in ratios.items():
        raw[x] = int(np.argmax(r > threshold))
    return first, threshold, raw


def pick_peak(window, n):
    """Position inside ``window`` of the seafloor pick: the n largest amplitudes (ties: lowest position first), positions ascending,
    the group before the first gap (without its last member; the first position alone when the gap follows it; all without a gap),
    the largest amplitude of the group."""
    order = np.lexsort((np.arange(window.size), -window.astype(np.float64)))
    pos = np.sort(order[:min(n, window.size)])
    gaps = np.flatnonzero(np.diff(pos) > 1)
    group = pos if gaps.size == 0 else pos[:max(gaps[0], 1)]
    return int(group[np.argmax(window[group])])


def peaks(data, first, base, win, n, nso=None):
    """Picked row of every live trace's valid slice (windows clipped to the slice); -1 for zero traces."""
    ns, ntr = data.shape
    out = np.full(ntr, -1)
    for x in np.flatnonzero(first >= 0):
        start = first[x] if nso is not None else 0
        tr = data[start:start + (nso or ns), x]
        lo, hi = max(base[x] - win, 0), min(base[x] + win, tr.size - 1)
        out[x] = lo + pick_peak(tr[lo:hi + 1], n)
    return out
