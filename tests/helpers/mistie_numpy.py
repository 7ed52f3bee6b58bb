"""Brute-force NumPy statement of step 7's data-parallel parts, written for the tests (the package does not import it): every segment of
line i against every segment of line j in float64 with the textbook parametric form (t, u from cross products -- not the side tests of the
kernel), the same rules for touching, shared vertices, collinear overlaps and zero-length segments; ``np.argmin`` for the nearest vertex; the
'same'-mode correlation by direct sums in float64, the reference's shift rule and Pearson's r."""
import numpy as np


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _special(a0, a1, b0, b1):
    """Hits of a parallel, collinear or zero-length segment pair (scalar code)."""
    r, s = a1 - a0, b1 - b0
    rr, ss = float(r @ r), float(s @ s)
    if rr == 0 and ss == 0:
        return [a0] if np.array_equal(a0, b0) else []
    if rr == 0:
        along = float((a0 - b0) @ s)
        return [a0] if _cross(a0 - b0, s) == 0 and 0 <= along <= ss else []
    if ss == 0:
        along = float((b0 - a0) @ r)
        return [b0] if _cross(b0 - a0, r) == 0 and 0 <= along <= rr else []
    if _cross(b0 - a0, r) != 0 or _cross(b1 - a0, r) != 0:
        return []                                                   # parallel, apart
    ends = sorted([(float((b0 - a0) @ r), 1, b0), (float((b1 - a0) @ r), 1, b1)], key=lambda e: e[0])
    lo = max([(0.0, 0, a0), ends[0]], key=lambda e: (e[0], -e[1]))  # at equal position the vertex of line i
    hi = min([(rr, 0, a1), ends[1]], key=lambda e: (e[0], e[1]))
    if lo[0] > hi[0]:
        return []
    return [lo[2]] if lo[0] == hi[0] else [lo[2], hi[2]]


def segment_pair_hits(pi, pj):
    """Hits of all segments of line ``pi`` [n, 2] with all segments of line ``pj`` [m, 2]: rows (seg_i, seg_j, part, x, y) sorted, a point
    kept once (its first occurrence)."""
    pi, pj = np.asarray(pi, float).reshape(-1, 2), np.asarray(pj, float).reshape(-1, 2)
    if pi.shape[0] < 2 or pj.shape[0] < 2:
        return np.zeros((0, 5))
    a0, a1, b0, b1 = pi[:-1, None, :], pi[1:, None, :], pj[None, :-1, :], pj[None, 1:, :]
    r, s, qp = a1 - a0, b1 - b0, b0 - a0
    den = _cross(r, s) + np.zeros((pi.shape[0] - 1, pj.shape[0] - 1))
    sign = np.where(den < 0, -1.0, 1.0)
    tn, un, dn = sign * _cross(qp, s), sign * _cross(qp, r), sign * den
    plain = (den != 0) & (tn >= 0) & (tn <= dn) & (un >= 0) & (un <= dn)
    rows = []
    for si, sj in zip(*np.nonzero(plain)):
        if tn[si, sj] == 0:
            p = pi[si]
        elif tn[si, sj] == dn[si, sj]:
            p = pi[si + 1]
        elif un[si, sj] == 0:
            p = pj[sj]
        elif un[si, sj] == dn[si, sj]:
            p = pj[sj + 1]
        else:
            p = pi[si] + (tn[si, sj] / dn[si, sj]) * (pi[si + 1] - pi[si])
        rows.append((si, sj, 0, p[0], p[1]))
    for si, sj in zip(*np.nonzero(den == 0)):
        for part, p in enumerate(_special(pi[si], pi[si + 1], pj[sj], pj[sj + 1])):
            rows.append((si, sj, part, p[0], p[1]))
    rows.sort(key=lambda h: h[:3])
    seen, kept = set(), []
    for h in rows:
        if h[3:] not in seen:
            kept.append(h)
            seen.add(h[3:])
    return np.array(kept, float).reshape(-1, 5)


def crossings(points_split):
    """All lines against all later lines: rows (i, j, seg_i, seg_j, part, x, y) ordered by (i, j, seg_i, seg_j, part)."""
    out = []
    for i in range(len(points_split)):
        for j in range(i + 1, len(points_split)):
            for h in segment_pair_hits(points_split[i], points_split[j]):
                out.append((i, j) + tuple(h))
    return np.array(out, float).reshape(-1, 7)


def nearest(points_split, xy, line_idx):
    """(index [k, 2], distance [k, 2]) of the vertex of either line nearest to every point, by ``np.argmin`` over sqrt(dx^2 + dy^2)."""
    xy, line_idx = np.asarray(xy, float).reshape(-1, 2), np.asarray(line_idx).reshape(-1, 2)
    index, dist = np.zeros(line_idx.shape, np.int32), np.zeros(line_idx.shape)
    for c in range(xy.shape[0]):
        for side in range(2):
            p = np.asarray(points_split[line_idx[c, side]], float).reshape(-1, 2)
            dx, dy = p[:, 0] - xy[c, 0], p[:, 1] - xy[c, 1]
            d = np.sqrt(dx * dx + dy * dy)
            index[c, side] = np.argmin(d)
            dist[c, side] = d[index[c, side]]
    return index, dist


def correlate_same(a, b):
    """scipy.signal.correlate(a, b, mode='same') of two equally long 1-D arrays by direct sums in float64: lags -(n // 2) ... n - 1 - n // 2."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = a.size
    cc = np.zeros(n)
    for k in range(n):
        lag = k - n // 2
        l0, l1 = max(0, -lag), min(n, n - lag)
        cc[k] = np.dot(a[l0 + lag:l1 + lag], b[l0:l1])
    return cc


def shift_rule(cc):
    idx = np.argmax(cc) if np.abs(np.max(cc)) >= np.abs(np.min(cc)) else np.argmin(cc)
    return len(cc) // 2 - int(idx)


def xcorr(a, b):
    """(n, shift, coeff, cc) of two windows of equal length: zeros of either trace dropped, direct 'same' correlation, the shift rule,
    Pearson's r in float64 (NaN for a constant trace)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    keep = ~((a == 0) | (b == 0))
    a, b = a[keep], b[keep]
    cc = correlate_same(a, b)
    da, db = a - a.mean(), b - b.mean()
    with np.errstate(invalid='ignore', divide='ignore'):
        r = float(np.clip(np.sum(da * db) / (np.sqrt(np.sum(da * da)) * np.sqrt(np.sum(db * db))), -1, 1))
    return a.size, shift_rule(cc), r, cc


def compensate_mistie(data, mistie):
    """The reference's compensate_mistie on [nsamples][ntraces] data, float32."""
    m = int(np.around(mistie, 0))
    data = np.asarray(data, np.float32)
    out = np.zeros_like(data)
    ns = data.shape[0]
    if m < 0 and -m < ns:
        out[:ns + m] = data[-m:]
    elif m > 0 and m < ns:
        out[m:] = data[:ns - m]
    elif m == 0:
        out[:] = data
    return out
