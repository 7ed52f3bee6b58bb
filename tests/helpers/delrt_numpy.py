"""NumPy restatement of what the step-3 / step-4 kernels compute (csrc/p3d_delrt.hip), written for the tests and the fixture generator: plain
and slow, sections are samples x traces as in the reference."""
import numpy as np


def pad(data, top, ns_out):
    """out[t][x] = data[t - top[x]][x] for top[x] <= t < top[x] + ns, else 0; out has ``ns_out`` rows."""
    data = np.asarray(data)
    ns, ntr = data.shape
    out = np.zeros((ns_out, ntr), data.dtype)
    for x, t in enumerate(np.asarray(top).tolist()):
        assert 0 <= t and t + ns <= ns_out
        out[t:t + ns, x] = data[:, x]
    return out


def windows(data, ref, n_traces, n_samples):
    """Per reference trace ``ref[c]``: (first row of its maximum, the maximum, the maxima of traces ref[c] - n_traces ... ref[c] + n_traces over
    the rows within n_samples // 2 of that row, cut at the ends of the trace).  The maxima are NOT clipped to the reference trace's."""
    data = np.asarray(data)
    ns = data.shape[0]
    ref = np.asarray(ref).ravel()
    peak_idx, peak_val = np.empty(ref.size, np.int32), np.empty(ref.size, data.dtype)
    maxima = np.empty((ref.size, 2 * n_traces + 1), data.dtype)
    for c, r in enumerate(ref.tolist()):
        assert r - n_traces >= 0 and r + n_traces < data.shape[1]
        trace = data[:, r]
        peak_idx[c] = trace.argmax()
        peak_val[c] = trace.max()
        lo, hi = max(peak_idx[c] - n_samples // 2, 0), min(peak_idx[c] + n_samples // 2 + 1, ns)
        maxima[c] = data[lo:hi, r - n_traces:r + n_traces + 1].max(axis=0)
    return peak_idx, peak_val, maxima


def packed_ref(m, n_traces):
    """The reference-trace indices of m packed subsets laid side by side."""
    return np.arange(m) * (2 * n_traces + 1) + n_traces
