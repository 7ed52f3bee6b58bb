"""Plain NumPy restatement of step 8 (despike_2D): detection per row over w adjacent traces, row coverage of the two views, the per-trace count
filter, runs, and the in-place replacement, with the two documented departures: a spike at x < h replaces its OWN trace from the
clipped neighbour window, and a split narrower than the window passes through unchanged.  Sections are [ns][ntr] like the reference's."""
import numpy as np


def rms(a, axis=None):
    n = a.size if axis is None else a.shape[axis]
    return np.sqrt(np.sum(a**2, axis=axis) / n)


FUNCS = {'mean': np.mean, 'median': np.median, 'rms': rms}


def window_params(ns, window, dt, overlap):
    """M, dy, main_end, add_start (None: no additional view)."""
    M = int(window / dt)
    ov = np.around(overlap / 100 * M, 0)
    ov = ov if ov >= 1 else 1
    dy = int(M - ov)
    if M > ns or M < 1 or dy < 1:
        raise ValueError(f'time window of {M} samples (step {dy}) does not fit a section of {ns} samples')
    main_end = ((ns - M) // dy) * dy + M
    add_start = ns - M if ns % dy != 0 else None
    return M, dy, main_end, add_start


def candidates(a, w, mode, threshold):
    """bool [ns][ntr]: |a| > threshold * f(|window|) for any of the windows of w adjacent traces that contain the sample."""
    func = FUNCS[mode]
    absa = np.abs(a)
    ns, ntr = a.shape
    cand = np.zeros(a.shape, bool)
    if ntr < w:
        return cand
    v = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(absa, w, axis=1))     # [ns][ntr - w + 1][w]
    tm = threshold * func(v, axis=-1)
    nwin = ntr - w + 1
    for k in range(w):
        cand[:, k:k + nwin] |= absa[:, k:k + nwin] > tm
    return cand


def find_spikes(a, window, dt, overlap=10, ntraces=5, mode='mean', threshold=2):
    """The spike list of one split: tuples (trace, lo, hi, first, last) in the reference's order (trace, first sample)."""
    ns, ntr = a.shape
    M, dy, main_end, add_start = window_params(ns, window, dt, overlap)
    cand = candidates(a, ntraces, mode, threshold)
    keep = np.zeros(a.shape, bool)
    views = [slice(0, main_end)] + ([slice(add_start, ns)] if add_start is not None else [])
    for rows in views:
        cnt = cand[rows].sum(axis=0)
        keep[rows] |= cand[rows] & (cnt > M * 0.1)[None, :]
    spikes = []
    for x in np.nonzero(keep.any(axis=0))[0]:
        t = np.nonzero(keep[:, x])[0]
        for run in np.split(t, np.nonzero(np.diff(t) > M * 0.05)[0] + 1):
            if run.size > M * 0.05:
                pad = int(run.size * 0.1)
                spikes.append((int(x), max(0, int(run[0]) - pad), min(ns, int(run[-1]) + pad + 1), int(run[0]), int(run[-1])))
    return spikes


def replace(a, spikes, ntraces, mode, threshold, out):
    """In place, in list order, each spike reading what the earlier ones wrote."""
    func = FUNCS[mode]
    h = ntraces // 2
    ntr = a.shape[1]
    for x, lo, hi, _, _ in spikes:
        c0, c1 = max(0, x - h), min(ntr, x + h + 1)
        win = a[lo:hi, c0:c1]
        amps = win[:, x - c0]
        new = {'scaled': lambda: amps / (amps.max() / func(np.abs(win), axis=1)) * np.blackman(hi - lo),
               'mode': lambda: func(win, axis=1),
               'threshold': lambda: func(win, axis=1) * threshold,
               'zeros': lambda: np.zeros_like(amps),
               'median': lambda: np.median(win, axis=1)}[out]()
        win[:, x - c0] = new.astype(a.dtype)
    return a


def despike_2D(array, window, dt, overlap=10, ntraces=5, mode='mean', threshold=2, out='scaled', splits=None, return_spikes=False):
    """Despiked copy of ``array`` [ns][ntr]; ``splits``: trace indices where a new split starts (each split is despiked on its own)."""
    a = np.array(array, copy=True)
    bounds = [0] + [int(s) for s in (splits if splits is not None else [])] + [a.shape[1]]
    found = []
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        if s1 - s0 < ntraces:
            continue
        part = a[:, s0:s1]
        spikes = find_spikes(part, window, dt, overlap, ntraces, mode, threshold)
        replace(part, spikes, ntraces, mode, threshold, out)
        found += [(x + s0, lo, hi, first, last) for x, lo, hi, first, last in spikes]
    return (a, found) if return_spikes else a
