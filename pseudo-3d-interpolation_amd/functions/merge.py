"""Step 1 -- merging short SEG-Y files with their neighbours: the grouping and the bookkeeping of the reference's merge_segys.py on the host,
the work per record on the GPU (HIP unit ``p3d_merge``).

Grouping (`files_to_merge`): runs of consecutive files below the size threshold, each run together with the file that follows it.

Merging (`merge_segys`): the trace records of a group (240-byte header + samples, any sample format) go to the device once.  There every
header is fingerprinted (`_ffi.merge_keys_dev`); the host finds the duplicates from the fingerprints and confirms them byte by byte
(`duplicate_masks`), lays the survivors out along TRACE_SEQUENCE_LINE (`merge_plan`), and the device gathers the output records, interpolates
the headers of the gap traces and zeroes their samples (`_ffi.merge_records_dev`).

The duplicate rule is the reference's ``duplicated(keep='last') | duplicated(subset=all but TRACE_SEQUENCE_FILE, keep='first')`` over all 91
header words, which tile the 240 bytes: byte equality of the headers, and byte equality with bytes 5-8 left out.  One consequence is kept:
two records whose headers are byte-identical, TRACE_SEQUENCE_FILE included, are BOTH dropped (the first by the first test, the second by the
second); `merge_segys` warns with their number."""
import os

import numpy as np

from .. import _ffi
from .header import add_processing_info_header, get_textual_header, write_textual_header
from .segy import BIN_BYTES, TEXT_BYTES, TRACE_HEADER_BYTES, SegyFile
from .segy_cli import remove_existing
from .utils import xprint

MSG_BINARY = 'Specified SEG-Y files have different binary headers. No easy merging possible, please check your data!'
TRACR = slice(4, 8)                                             # TRACE_SEQUENCE_FILE, bytes 5-8
DOWNLOAD_BYTES = 256 << 20


def files_to_merge(files, fsize_kB=2000, verbosity=0):
    """The groups of files to merge, as lists of paths: every run of consecutive files smaller than ``fsize_kB`` (``os.path.getsize / 1024 <``)
    together with the file behind the run; a run at the end of the list stands alone.  No small file: an empty list."""
    files = list(files)
    small = [k for k, path in enumerate(files) if os.path.getsize(path) / 1024 < fsize_kB]
    xprint(f'Found < {len(small)} > files smaller than {fsize_kB} KB', kind='info', verbosity=verbosity)
    runs = []
    for k in small:
        if runs and runs[-1][1] == k - 1:
            runs[-1][1] = k
        else:
            runs.append([k, k])
    xprint(f'Remaining < {len(runs)} > files after groupby', kind='info', verbosity=verbosity)
    groups = [files[first:last + 2] for first, last in runs]
    xprint(f'Prepared < {len(groups)} > merged files', kind='info', verbosity=verbosity)
    return groups


def _rows(a):
    """[n][m] bytes as n opaque values that compare equal exactly when the rows do."""
    a = np.ascontiguousarray(a)
    return a.view(np.dtype((np.void, a.shape[1]))).ravel()


def _classes(values):
    """Class number of every value (equal values share one) and the size of every class."""
    _, inverse, counts = np.unique(values, return_inverse=True, return_counts=True)
    return inverse.ravel(), counts


def _exact_classes(headers, fingerprints, drop=None):
    """Classes of byte-identical headers (``drop``: a slice of bytes left out of the comparison).  With ``fingerprints`` only the records
    whose fingerprint occurs more than once are compared byte by byte; all others are classes of their own."""
    n = headers.shape[0]
    keep = np.ones(TRACE_HEADER_BYTES, bool)
    if drop is not None:
        keep[drop] = False
    if fingerprints is None:
        return _classes(_rows(headers[:, keep]))
    inverse, counts = _classes(np.asarray(fingerprints))
    crowd = np.flatnonzero(counts[inverse] > 1)
    classes = np.arange(n)                                      # a record alone in its fingerprint class: its own class
    if crowd.size:
        sub, _ = _classes(_rows(headers[crowd][:, keep]))
        first = np.full(sub.max() + 1, n)
        np.minimum.at(first, sub, crowd)
        classes[crowd] = first[sub]                             # named by the first member, a record number: no clash with the others
    _, inverse, counts = np.unique(classes, return_inverse=True, return_counts=True)
    return inverse.ravel(), counts


def duplicate_masks(headers, fp_full=None, fp_sub=None):
    """``(overlapping, internal)``: the reference's two duplicate masks over the 240-byte trace headers uint8 [n][240] --
    ``duplicated(keep='last')`` on whole headers and ``duplicated(keep='first')`` on headers without TRACE_SEQUENCE_FILE (bytes 5-8).

    ``fp_full`` / ``fp_sub`` (uint64 [n], from `_ffi.merge_keys`) only narrow the search: records that share a fingerprint are confirmed by
    comparing their header bytes, so a collision can never drop a trace."""
    headers = np.ascontiguousarray(headers, dtype=np.uint8)
    if headers.ndim != 2 or headers.shape[1] != TRACE_HEADER_BYTES:
        raise ValueError(f'headers are [n][{TRACE_HEADER_BYTES}] bytes')
    n = headers.shape[0]
    index = np.arange(n)
    full, full_counts = _exact_classes(headers, fp_full)
    last = np.full(full_counts.size, -1)
    np.maximum.at(last, full, index)
    overlapping = index != last[full]
    sub, sub_counts = _exact_classes(headers, fp_sub, drop=TRACR)
    first = np.full(sub_counts.size, n)
    np.minimum.at(first, sub, index)
    internal = index != first[sub]
    return overlapping, internal


def lost_traces(headers, overlapping):
    """The number of traces of which every copy is dropped: the different headers among the records that ``overlapping`` marks.  A header that
    occurs k > 1 times is marked k - 1 times there, and its last copy is an internal duplicate of the first."""
    marked = np.ascontiguousarray(np.asarray(headers, dtype=np.uint8)[np.asarray(overlapping, dtype=bool)])
    return int(np.unique(_rows(marked)).size) if marked.shape[0] else 0


def merge_plan(tracl, mask):
    """``(src, lo_row, hi_row)``, int32 [nout]: the survivors (``~mask``) reindexed onto TRACE_SEQUENCE_LINE from the first to the last one.
    Row r holds record ``src[r]`` (the survivor with ``tracl == tracl_first + r``) or is a gap (``src[r]`` = -1) between the nearest rows that
    hold records, ``lo_row[r] < r < hi_row[r]`` (for a row with a record both are r).  The survivors' TRACE_SEQUENCE_LINE must increase strictly
    in file order -- the only case in which the reference keeps headers and samples aligned -- else ``ValueError``."""
    tracl = np.asarray(tracl, dtype=np.int64).ravel()
    mask = np.asarray(mask, dtype=bool).ravel()
    if tracl.shape != mask.shape:
        raise ValueError(f'{tracl.size} TRACE_SEQUENCE_LINE values but {mask.size} mask entries')
    kept = np.flatnonzero(~mask)
    if kept.size == 0:
        raise ValueError('no trace is left after the duplicates are dropped')
    line = tracl[kept]
    if np.any(np.diff(line) <= 0):
        at = int(np.flatnonzero(np.diff(line) <= 0)[0])
        raise ValueError(f'TRACE_SEQUENCE_LINE must increase strictly along the merged files: record {int(kept[at + 1])} holds {int(line[at + 1])} '
                         f'behind {int(line[at])}')
    nout = int(line[-1] - line[0]) + 1
    if nout > np.iinfo(np.int32).max:
        raise ValueError(f'TRACE_SEQUENCE_LINE {int(line[0])} ... {int(line[-1])} spans {nout} traces')
    rows = np.arange(nout)
    src = np.full(nout, -1, np.int64)
    src[line - line[0]] = kept
    lo_row = np.maximum.accumulate(np.where(src >= 0, rows, -1))
    hi_row = np.minimum.accumulate(np.where(src >= 0, rows, nout)[::-1])[::-1]
    return src.astype(np.int32), lo_row.astype(np.int32), hi_row.astype(np.int32)


def _trace_bytes(segy):
    """The trace records of an open `SegyFile` as a read-only map uint8 [ntraces][reclen]."""
    reclen = segy.reclen
    raw = np.memmap(segy.path, np.uint8, 'r')
    start = raw.size - segy.ntraces * reclen
    return raw[start:].reshape(segy.ntraces, reclen), start


def merge_segys(file_list, txt_suffix='merge', device=0, verbosity=0):
    """Merge the SEG-Y files of ``file_list`` into ``<dir of the first>/<stem of the first>_<txt_suffix><ext>`` and write ``<stem>_<txt_suffix>.parts``
    next to it; returns the path of the merged file.

    The binary headers (400 bytes) must be equal, else ``IOError``.  Duplicate traces are dropped (module docstring), the survivors are put in
    the order of TRACE_SEQUENCE_LINE, missing numbers become gap traces (header words interpolated linearly and cut to int32, samples zero), and
    TRACE_SEQUENCE_FILE counts 1 ... n.  Samples are moved as bytes, so every sample format the reader knows (1, 2, 3, 5, 8) is merged bit-exactly.
    The textual header is the first file's with the line ``MERGED: <file stems>``; binary and extended textual headers are the first file's.
    The whole group, input and output records, is resident on the device; a group that does not fit raises ``MemoryError``."""
    say = lambda *a, **kw: xprint(*a, verbosity=verbosity, **kw)  # noqa: E731
    file_list = list(file_list)
    if not file_list:
        raise ValueError('no files to merge')
    first_file = file_list[0]
    folder, filename = os.path.split(first_file)
    stem, ext = os.path.splitext(filename)
    out_name = f'{stem}_{txt_suffix}{ext}'
    out_file = os.path.join(folder, out_name)

    maps, counts, binary, head = [], [], None, None
    for path in file_list:
        say(f'Processing file < {os.path.basename(path)} >', kind='info')
        segy = SegyFile(path)
        records, start = _trace_bytes(segy)
        with open(path, 'rb') as fh:
            top = fh.read(start)
        if binary is None:
            binary, head = top[TEXT_BYTES:TEXT_BYTES + BIN_BYTES], top
        elif top[TEXT_BYTES:TEXT_BYTES + BIN_BYTES] != binary:
            raise IOError(MSG_BINARY)
        maps.append(records)
        counts.append(segy.ntraces)
    nsrc, reclen = int(sum(counts)), maps[0].shape[1]
    if nsrc == 0:
        raise ValueError('the files to merge hold no trace')
    if nsrc > np.iinfo(np.int32).max:
        raise MemoryError(f'{nsrc} traces are more than one merge handles')

    def room(nbytes, what):
        free, _ = _ffi.device_mem_info(device)
        if nbytes > free:
            raise MemoryError(f'{what} ({nbytes} bytes) do not fit the free memory of device {device} ({free} bytes): a group is merged as a whole, '
                              'it is not streamed')

    say('Merge trace headers', kind='debug')
    room(nsrc * (reclen + 20), f'the {nsrc} records of the group')
    bufs = []
    try:
        drec = _ffi.DeviceArray((nsrc, reclen), np.uint8, device)
        bufs.append(drec)
        first = 0
        for records in maps:
            drec.upload(records, first)
            first += records.shape[0]
        dtracl, dfull, dsub = (_ffi.DeviceArray((nsrc,), dt, device) for dt in (np.int32, np.uint64, np.uint64))
        bufs += [dtracl, dfull, dsub]
        _ffi.merge_keys_dev(drec.ptr, nsrc, reclen, dtracl.ptr, dfull.ptr, dsub.ptr, device)
        tracl, fp_full, fp_sub = dtracl.download(), dfull.download(), dsub.download()

        headers = np.concatenate([records[:, :TRACE_HEADER_BYTES] for records in maps])
        overlapping, internal = duplicate_masks(headers, fp_full, fp_sub)
        lost = lost_traces(headers, overlapping)
        del headers
        mask = overlapping | internal
        if mask.any():
            say(f'Removed < {np.count_nonzero(mask)} > duplicates', kind='debug')
        if lost:
            say(f'< {lost} > trace(s) occur more than once with byte-identical headers (TRACE_SEQUENCE_FILE included): every copy is dropped, '
                'as by the reference', kind='warning')
        src, lo_row, hi_row = merge_plan(tracl, mask)
        nout = src.size
        if np.any(src < 0):
            say('Interpolate gaps in merged trace header', kind='debug')
            say('Fill gaps with zero traces', kind='debug')

        say('Merge seismic data', kind='debug')
        room(nout * (reclen + 12), f'the {nout} merged records beside the {nsrc} of the input')
        dout = _ffi.DeviceArray((nout, reclen), np.uint8, device)
        bufs.append(dout)
        _ffi.merge_records_dev(drec.ptr, nsrc, reclen, src, lo_row, hi_row, dout.ptr, device)

        say('Write merged SEG-Y to disk', kind='debug')
        remove_existing(out_file, say)
        with open(out_file, 'wb') as fh:
            fh.write(head)
            fh.truncate(len(head) + nout * reclen)
        merged = np.memmap(out_file, np.uint8, 'r+', offset=len(head), shape=(nout, reclen))
        step = max(1, DOWNLOAD_BYTES // reclen)
        for row in range(0, nout, step):
            count = min(step, nout - row)
            dout.download(row, count, out=merged[row:row + count])
        merged.flush()
        del merged
    finally:
        for buf in bufs:
            buf.free()

    info = ','.join(os.path.splitext(os.path.basename(path))[0] for path in file_list)
    write_textual_header(out_file, add_processing_info_header(get_textual_header(out_file), info, prefix='MERGED'))

    with open(os.path.join(folder, f'{stem}_{txt_suffix}.parts'), 'w', newline='\n') as fh:
        fh.write(f'The merged SEG-Y file < {out_name} > contains the following files:\n')
        for path, ntr in zip(file_list, counts):
            fh.write(f'    - {os.path.basename(path)}    {ntr:>6d} trace(s)\n')
        fh.write(f'Trace duplicates (different files):    {np.count_nonzero(overlapping):>3d}\n')
        fh.write(f'Trace duplicates (within single file): {np.count_nonzero(internal):>3d}\n')
    return out_file
