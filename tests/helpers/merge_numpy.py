"""NumPy restatement of step 1 (csrc/p3d_merge.hip, csrc/p3d_merge_words.hpp, functions/merge.py), written from the definitions and
independent of the package: the width table of the 91 header words, the fingerprints of the keys kernel, the two duplicate masks (plain
loops over header bytes), the plan, the interpolated header table and the output records."""
import numpy as np

HDR = 240
RUNS = [(7, 4), (4, 2), (8, 4), (2, 2), (4, 4), (46, 2), (5, 4), (2, 2), (1, 4), (5, 2), (1, 4), (1, 2), (1, 4), (1, 2), (1, 2), (2, 4)]
WIDTHS = np.array([w for count, w in RUNS for _ in range(count)])
OFFSETS = np.concatenate([[0], np.cumsum(WIDTHS)[:-1]])
assert WIDTHS.size == 91 and WIDTHS.sum() == HDR
M64 = (1 << 64) - 1


def words_of(headers):
    """Headers uint8 [n][240] -> the 91 signed big-endian words, int64 [n][91]."""
    headers = np.ascontiguousarray(headers, dtype=np.uint8)
    out = np.empty((headers.shape[0], 91), np.int64)
    for j, (off, w) in enumerate(zip(OFFSETS, WIDTHS)):
        out[:, j] = np.ascontiguousarray(headers[:, off:off + w]).view('>i4' if w == 4 else '>i2').ravel()
    return out


def headers_of(words):
    """int [n][91] -> headers uint8 [n][240]; a word keeps its low 16 or 32 bits."""
    words = np.asarray(words, dtype=np.int64)
    out = np.empty((words.shape[0], HDR), np.uint8)
    for j, (off, w) in enumerate(zip(OFFSETS, WIDTHS)):
        low = (words[:, j] & ((1 << (8 * w)) - 1)).astype('>u4' if w == 4 else '>u2')
        out[:, off:off + w] = low.view(np.uint8).reshape(-1, w)
    return out


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys(records):
    """(tracl int32 [n], fp_full uint64 [n], fp_sub uint64 [n]) of records uint8 [n][reclen >= 240]."""
    headers = np.ascontiguousarray(np.asarray(records, dtype=np.uint8)[:, :HDR])
    dwords = headers.view('<u4').astype(np.uint64)                               # [n][60]
    lanes = (np.arange(60, dtype=np.uint64) + np.uint64(1)) << np.uint64(32)
    terms = splitmix64(lanes[None, :] | dwords)
    full = np.bitwise_xor.reduce(terms, axis=1)
    sub = full ^ terms[:, 1]
    tracl = np.ascontiguousarray(headers[:, :4]).view('>i4').ravel().astype(np.int32)
    return tracl, full, sub


def duplicate_masks(headers):
    """The two masks by their definitions: a record is an overlapping duplicate if a LATER record has the same 240 bytes, an internal one if an
    EARLIER record has the same bytes outside 5-8."""
    h = [bytes(row) for row in np.asarray(headers, dtype=np.uint8)[:, :HDR]]
    s = [row[:4] + row[8:] for row in h]
    n = len(h)
    overlapping = np.array([any(h[j] == h[i] for j in range(i + 1, n)) for i in range(n)], bool)
    internal = np.array([any(s[j] == s[i] for j in range(i)) for i in range(n)], bool)
    return overlapping, internal


def plan(tracl, mask):
    kept = [i for i in range(len(tracl)) if not mask[i]]
    line = [int(tracl[i]) for i in kept]
    if any(b <= a for a, b in zip(line, line[1:])):
        raise ValueError('TRACE_SEQUENCE_LINE does not increase strictly')
    nout = line[-1] - line[0] + 1
    src = np.full(nout, -1, np.int32)
    for i, t in zip(kept, line):
        src[t - line[0]] = i
    lo, hi = np.arange(nout, dtype=np.int32), np.arange(nout, dtype=np.int32)
    for r in range(nout):
        if src[r] < 0:
            lo[r] = max(q for q in range(r) if src[q] >= 0)
            hi[r] = min(q for q in range(r + 1, nout) if src[q] >= 0)
    return src, lo, hi


def interp_word(va, vb, a, b, r):
    """np.interp's arithmetic in IEEE double, then the C cast to int32 (toward zero)."""
    va, vb, a, b, r = (np.asarray(x, dtype=np.float64) for x in (va, vb, a, b, r))
    slope = (vb - va) / (b - a)
    return np.trunc(slope * (r - a) + va).astype(np.int64).astype(np.int32)


def merged_words(words, src, lo, hi):
    """The header table int32 [nout][91] of the merged file: survivors' words, gaps interpolated, TRACE_SEQUENCE_FILE (word 1) = 1 ... nout."""
    words = np.asarray(words, dtype=np.int64)
    nout = len(src)
    out = np.empty((nout, 91), np.int32)
    for r in range(nout):
        if src[r] >= 0:
            out[r] = words[src[r]]
        else:
            out[r] = interp_word(words[src[lo[r]]], words[src[hi[r]]], lo[r], hi[r], r)
    out[:, 1] = np.arange(1, nout + 1)
    return out


def merged_records(records, src, lo, hi):
    """Output records uint8 [nout][reclen]."""
    records = np.asarray(records, dtype=np.uint8)
    table = merged_words(words_of(records[:, :HDR]), src, lo, hi)
    out = np.zeros((len(src), records.shape[1]), np.uint8)
    out[:, :HDR] = headers_of(table)
    for r, s in enumerate(src):
        if s >= 0:
            out[r, HDR:] = records[s, HDR:]
            assert np.array_equal(np.delete(out[r, :HDR], np.s_[4:8]), np.delete(records[s, :HDR], np.s_[4:8]))
    return out


def merge(records):
    """records -> (out records, overlapping, internal, (src, lo, hi))."""
    overlapping, internal = duplicate_masks(records)
    tracl, _, _ = keys(records)
    src, lo, hi = plan(tracl, overlapping | internal)
    return merged_records(records, src, lo, hi), overlapping, internal, (src, lo, hi)
