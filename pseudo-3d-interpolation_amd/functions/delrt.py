"""Steps 3 and 4: check of the DelayRecordingTime (`delrt`) at the places where the recording window jumps, and zero padding of the traces
onto one time axis (mirror of the reference's ``correct_single_trace_DelayRecordingTime`` / ``check_DelayRecordingTime_changes`` and
``pad_trace_data``).

What touches the samples runs on the GPU (csrc/p3d_delrt.hip) on the trace-major layout of the SEG-Y file: the placement of the traces
in the padded section, and per delay change the peak of the reference trace and the maxima of its neighbours in the window around that
peak -- all changes of a file in one launch, only the traces of the subsets are uploaded.  The time axis, the top padding per run of
equal delays and the decision are NumPy on the host, with the reference's own expressions.  DESIGN.md 3.11 has the kernels and the
departures from the reference."""
import numpy as np

from .. import _ffi

MSG_MESSED_UP = '[ERROR]    Something is really messed up here. Check your data!'


# ---- step 4: padding ------------------------------------------------------------------------------------------------

def delay_changes(recording_delays):
    """Trace indices at which the delay changes, with a leading 0 (the reference's ``np.roll`` comparison and its sanity branch for a
    file whose first and last delays are equal)."""
    recording_delays = np.asarray(recording_delays)
    idx_delay = np.where(np.roll(recording_delays, 1) != recording_delays)[0]
    if idx_delay.size == 0 or idx_delay[0] != 0:
        idx_delay = np.insert(idx_delay, 0, 0, axis=0)
    return idx_delay


def pad_layout(recording_delays, dt, twt):
    """The host arithmetic of `pad_trace_data`: ``(twt_padded, top, idx_delay, min_delay, max_delay)`` with ``top`` int32, the number of
    zero samples above every trace.  The expressions are the reference's, kept as written so that float steps behave the same."""
    recording_delays = np.asarray(recording_delays)
    idx_delay = delay_changes(recording_delays)
    min_delay = recording_delays.min()
    max_delay = recording_delays.max()
    twt_padded = np.arange(min_delay, max_delay + (twt[-1] - twt[0]) + dt, dt)
    top = np.empty(recording_delays.size, np.int32)
    ends = np.append(idx_delay[1:], recording_delays.size)
    for first, last in zip(idx_delay, ends):
        top[first:last] = np.arange(min_delay, recording_delays[first], dt).size
    return twt_padded, top, idx_delay, min_delay, max_delay


def pad_trace_data(data, recording_delays, n_traces, dt, twt, verbosity=0, trace_major=False, device=0):
    """
    Pad traces recorded in window mode (fixed length, variable DelayRecordingTime) with zeros at top and bottom so that all share the
    time axis from the smallest delay to the largest delay plus the window length.

    data : samples x traces (traces x samples with ``trace_major=True``, the SEG-Y layout: no transpose then); ``recording_delays`` [ms]
    per trace, ``n_traces`` their number, ``dt`` [ms], ``twt`` the TWT of the samples of a trace.
    Returns ``(data_padded, twt_padded, n_samples_padded, (idx_delay, min_delay, max_delay))`` as the reference does; the padded data is
    float32 in the layout of the input.  A trace that does not fit the padded axis raises ``ValueError`` (the reference dies there in
    ``np.zeros`` with a negative size).
    """
    a = np.asarray(data)
    if a.ndim != 2 or a.size == 0:
        raise ValueError('Input array must be 2D (samples x traces).')
    section = np.ascontiguousarray(a if trace_major else a.T, dtype=np.float32)
    ntr, ns = section.shape
    recording_delays = np.asarray(recording_delays)
    if recording_delays.shape != (ntr,) or int(n_traces) != ntr:
        raise ValueError(f'{ntr} traces but {recording_delays.shape} delays and n_traces={n_traces}')
    twt_padded, top, idx_delay, min_delay, max_delay = pad_layout(recording_delays, dt, twt)
    n_samples_padded = len(twt_padded)
    if np.any(top + ns > n_samples_padded):
        x = int(np.argmax(top + ns > n_samples_padded))
        raise ValueError(f'trace {x}: {int(top[x])} samples of top padding and {ns} samples do not fit the padded axis of {n_samples_padded} samples')
    padded = _ffi.delrt_pad(section, top, n_samples_padded, device=device)
    return (padded if trace_major else np.ascontiguousarray(padded.T)), twt_padded, n_samples_padded, (idx_delay, min_delay, max_delay)


# ---- step 3: correction -----------------------------------------------------------------------------------------------

def decide_delay(maxima, peak_val, delrt_subset, n_traces, say=None):
    """The reference's decision for one delay change, from the device's results: ``maxima`` the window maximum of every trace of the
    subset (not yet clipped), ``peak_val`` the maximum of the reference trace (trace ``n_traces`` of the subset), ``delrt_subset`` the
    delays of the subset.  Returns ``(corrected delay, index within the subset of the trace it belongs to)`` or ``(None, None)``; raises
    ``RuntimeError`` where the reference exits ('... really messed up ...')."""
    say = say or (lambda *a, **k: None)
    tr_amp_maxima = np.array(maxima)
    delrt = np.asarray(delrt_subset)
    ref_tr_peak_val = tr_amp_maxima.dtype.type(peak_val)
    tr_amp_max_idx_trace = tr_amp_maxima[n_traces]
    tr_amp_maxima[tr_amp_maxima > tr_amp_max_idx_trace] = tr_amp_max_idx_trace
    with np.errstate(divide='ignore', invalid='ignore'):
        tr_amp_max_diff_rel = np.abs(tr_amp_maxima - ref_tr_peak_val) / ref_tr_peak_val     # in the data's float32
    tr_amp_similarity = np.where(tr_amp_max_diff_rel > 0.8, 1, 0).astype('int')
    delrt_similarity = np.where(delrt == delrt.max(), 1, 0)
    delrt_similarity_inv = np.abs(delrt_similarity - 1)

    r = tr_amp_similarity[n_traces]
    before, after = tr_amp_similarity[:n_traces], tr_amp_similarity[n_traces + 1:]
    if (np.all(before == r) and np.all(after != r)) or (np.all(before != r) and np.all(after == r)):
        if np.array_equal(tr_amp_similarity, delrt_similarity) or np.array_equal(tr_amp_similarity, delrt_similarity_inv):
            say('<<< No correction needed >>>', kind='debug')
            return None, None
        say('*** Incorrect DelayRecordingTime! ***', kind='warning')
        delrt_uniq = np.unique(delrt)
        ref_tr_delrt_corrected = delrt_uniq[delrt_uniq != delrt[n_traces]]
        idx_n_traces = n_traces
    elif [np.sum(before), np.sum(after)] in [[n_traces, 1], [1, n_traces]]:
        say('Eligible for adjusting offset trace', kind='debug')
        tr_amp_similarity = [int(v) for v in tr_amp_similarity]
        # the first two and the last two traces of the subset are equal pairs of either kind (boundary condition)
        if not all(x in [tr_amp_similarity[:2], tr_amp_similarity[-2:]] for x in [[1, 1], [0, 0]]):
            return None, None
        say('*** [OFFSET TRACE] Incorrect DelayRecordingTime! ***', kind='warning')
        idx_peak_amp_changes = np.where(np.roll(tr_amp_similarity, 1) != np.array(tr_amp_similarity))[0]
        n_after = len(idx_peak_amp_changes[idx_peak_amp_changes > n_traces])
        n_before = len(idx_peak_amp_changes[idx_peak_amp_changes < n_traces])
        if n_after < n_before:            # the fishy trace lies before the change of the delay
            idx_ = idx_peak_amp_changes[1]
        elif n_after > n_before:          # ... after it
            idx_ = idx_peak_amp_changes[-2]
        else:                             # two isolated traces with a false delay
            raise RuntimeError(MSG_MESSED_UP)
        delrt_uniq = np.unique(delrt)
        ref_tr_delrt_corrected = delrt_uniq[delrt_uniq != delrt[idx_]]
        idx_n_traces = int(idx_)
    else:
        return None, None

    if len(ref_tr_delrt_corrected) > 1:
        say('Found more than one DelayRecordingTime to choose from. No changes applied.', kind='error')
        return None, None
    return ref_tr_delrt_corrected[0], idx_n_traces


def correct_single_trace_DelayRecordingTime(idx, data, delrt, fldr, n_traces=5, n_samples=120, verbosity=0, device=0):
    """
    Correct delay of the trace at a delay change by comparing the maximum amplitude of the reference trace with the maxima of ``n_traces``
    neighbours to each side within ``n_samples`` samples around it (parameters and return value of the reference's function).

    data : samples x (2 n_traces + 1) traces, the subset around change ``idx`` (``idx`` and ``fldr`` are not used, as there); ``delrt``
    the delays of the subset.  Returns ``(corrected delay, index of the trace within the subset)`` or ``(None, None)``.
    """
    a = np.asarray(data)
    if a.ndim != 2 or a.shape[1] != 2 * n_traces + 1:
        raise ValueError(f'the data subset must hold {2 * n_traces + 1} traces (samples x traces), got an array of shape {a.shape}')
    subset = np.ascontiguousarray(a.T, dtype=np.float32)[None]
    _, peak_val, maxima = _ffi.delrt_windows(subset, n_samples, device=device)
    return decide_delay(maxima[0], peak_val[0], delrt, n_traces, say=_say(verbosity))


def _say(verbosity):
    from functools import partial

    from .utils import xprint
    return partial(xprint, verbosity=verbosity)


def delay_change_subsets(delrt, tracecount, n_traces, say=None):
    """The delay changes that the reference examines, by its skip rules: ``[(idx, first trace, one past the last trace)]``.  A change is
    left out when it has too few neighbours -- the reference's own inequality, which lets the subset of a change ``n_traces`` before the
    end of the file through one trace short -- or when its subset holds more than two different delays."""
    say = say or (lambda *a, **k: None)
    delrt = np.asarray(delrt)
    kept = []
    for idx in delay_changes(delrt)[1:]:
        idx = int(idx)
        lo, hi = idx - n_traces, idx + n_traces + 1
        if lo < 0 or hi > tracecount + 1:
            say(f'Not enough neighboring traces for idx: {idx} [{lo}:{hi}] with >{tracecount}< total traces. Skipped data subset.', kind='warning')
            continue
        if len(np.unique(delrt[lo:hi])) > 2:
            say(f'Too many different `delrt` for idx: {idx} [{lo}:{hi}]. Skipped data subset.', kind='warning')
            continue
        kept.append((idx, lo, min(hi, tracecount)))
    return kept


def correct_delay_changes(section_or_file, delrt, n_traces=5, n_samples=120, say=None, device=0):
    """
    Examine every delay change of a profile: ``section_or_file`` a trace-major section [ntr][ns] or an open ``SegyFile``, ``delrt`` the
    delay of every trace.  The subsets of all changes that pass the reference's skip rules (`delay_change_subsets`) go to the device in
    one launch; the delays are read once, before the loop, as in the reference, so the changes are independent.
    Returns ``[(idx, trace_to_fix, old, new)]``: the change, the trace whose delay is wrong (``idx - n_traces +`` the index the decision
    names), its delay and the corrected one.
    """
    delrt = np.asarray(delrt)
    traces = section_or_file.traces if hasattr(section_or_file, 'traces') else lambda rows: np.asarray(section_or_file)[rows]
    tracecount = delrt.size
    kept = delay_change_subsets(delrt, tracecount, n_traces, say)
    if not kept:
        return []
    width = 2 * n_traces + 1
    # a subset that is one trace short is filled up with its last trace; that column is dropped again before the decision
    rows = np.array([np.minimum(np.arange(lo, lo + width), hi - 1) for _, lo, hi in kept])
    subsets = np.asarray(traces(rows.ravel()), dtype=np.float32)
    subsets = subsets.reshape(len(kept), width, subsets.shape[-1])
    _, peak_val, maxima = _ffi.delrt_windows(subsets, n_samples, device=device)
    fixes = []
    for c, (idx, lo, hi) in enumerate(kept):
        new, at = decide_delay(maxima[c, :hi - lo], peak_val[c], delrt[lo:hi], n_traces, say)
        if new is not None:
            fixes.append((idx, lo + at, delrt[lo + at], new))
    return fixes
