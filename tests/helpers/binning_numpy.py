"""NumPy restatement of the step-10 stacking kernel (p3d_bin_stack): the CSR tables in, the slice-major cube out."""
import numpy as np


def padded(samples, off, length, shift, nt):
    """One trace on the cube's twt axis: sample i at i + shift, zeros elsewhere."""
    out = np.zeros(nt, np.float32)
    j = np.arange(nt)
    i = j - shift
    ok = (i >= 0) & (i < length)
    out[ok] = samples[off + i[ok]]
    return out


def bin_stack(samples, trace_off, trace_len, shift, bin_start, nil, nxl, nt, method='average', weight=None):
    out = np.zeros((nt, nil * nxl), np.float32)
    for b in range(nil * nxl):
        t0, t1 = int(bin_start[b]), int(bin_start[b + 1])
        if t1 == t0:
            continue
        stk = np.stack([padded(samples, trace_off[t], trace_len[t], shift[t], nt) for t in range(t0, t1)])
        if method == 'average':
            out[:, b] = (stk.astype(np.float64).sum(0) / (t1 - t0)).astype(np.float32)
        elif method == 'median':
            out[:, b] = np.median(stk, axis=0)
        elif method == 'nearest':
            out[:, b] = stk[0]
        else:
            out[:, b] = (stk.astype(np.float64) * np.asarray(weight[t0:t1])[:, None]).sum(0).astype(np.float32)
    return out.reshape(nt, nil, nxl)
