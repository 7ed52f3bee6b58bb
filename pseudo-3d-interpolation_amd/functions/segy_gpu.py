"""SEG-Y trace records on the GPU (HIP unit ``p3d_segy``): float32 sections <-> big-endian records of a 240-byte header and ``ns`` samples.

``encode_records`` / ``decode_records`` convert arrays; ``write_cube_segy`` writes a 3-D cube as a SEG-Y file (step 16) and ``read_segy_gpu`` reads a
file (step 9), both in chunks of about ``chunk_bytes`` of records, so a file larger than device memory converts as well.  The sample
conversions are bit-identical to ``functions/segy.py``; that module stays the host reader and writer of all other steps.

The header words known here are ``segy.TRACE_FIELDS`` and the four that step 16 adds (``EXTRA_FIELDS``)."""
import os

import numpy as np

from .. import _ffi
from . import segy as S

# name: (1-based byte, big-endian dtype) -- the words segy.TRACE_FIELDS does not hold
EXTRA_FIELDS = {
    'CDP': (21, '>i4'),
    'NStackedTraces': (33, '>i2'),
    'INLINE_3D': (189, '>i4'),
    'CROSSLINE_3D': (193, '>i4'),
}
FIELDS = {**S.TRACE_FIELDS, **EXTRA_FIELDS}
# binary-header words beside segy.BIN_FIELDS: name: (1-based byte in the file, dtype)
BIN_EXTRA = {
    'IntervalOriginal': (3219, '>u2'),
    'SortingCode': (3229, '>i2'),
    'MeasurementSystem': (3255, '>i2'),
}
BIN_ALL = {**S.BIN_FIELDS, **BIN_EXTRA}
CHUNK_BYTES = 256 << 20
MAX_COLUMNS = 16


def _field(name):
    if name not in FIELDS:
        raise KeyError(f'{name!r} is not one of the trace-header fields {sorted(FIELDS)}')
    byte, dt = FIELDS[name]
    return byte - 1, np.dtype(dt)


def header_columns(headers, ntr):
    """``headers`` (field name -> one value per trace, or a scalar for all traces) as ``(constants, names, table, values)``: the scalars as
    {name: int}, and the per-trace words as the kernel's table of (byte offset, width) with int32 values [ncolumns][ntr].  Values that do not
    fit their word raise ``OverflowError`` here, on the host, as ``segy.update_headers`` does."""
    constants, names, table, values = {}, [], [], []
    for name, v in (headers or {}).items():
        off, dt = _field(name)
        v = np.asarray(v)
        if v.dtype.kind not in 'iub':
            if not np.all(np.isfinite(v)) or np.any(v != np.rint(v)):
                raise ValueError(f'{name}: header words are integers')
        info = np.iinfo(dt)
        if v.size and (v.min() < info.min or v.max() > info.max):
            raise OverflowError(f'{name}: values outside the range of a {info.bits}-bit header word')
        if v.ndim == 0:
            constants[name] = int(v)
            continue
        if v.shape != (ntr,):
            raise ValueError(f'{ntr} traces, got {v.shape} values for {name}')
        names.append(name)
        table.append((off, dt.itemsize))
        values.append(v.astype(np.int32))
    if len(names) > MAX_COLUMNS:
        raise ValueError(f'{len(names)} per-trace header words (at most {MAX_COLUMNS}); words that are the same for all traces go in as scalars')
    return constants, names, table, (np.stack(values) if values else np.zeros((0, ntr), np.int32))


def header_template(constants=None, template=None):
    """240 header bytes: ``template`` (zeros by default) with the words of ``constants`` (field name -> int) written into it."""
    out = np.zeros(S.TRACE_HEADER_BYTES, np.uint8) if template is None else np.array(template, np.uint8)
    if out.shape != (S.TRACE_HEADER_BYTES,):
        raise ValueError(f'the header template holds {S.TRACE_HEADER_BYTES} bytes')
    for name, v in (constants or {}).items():
        off, dt = _field(name)
        out[off:off + dt.itemsize] = np.frombuffer(np.array(v, dt).tobytes(), np.uint8)
    return out


def encode_records(section, layout, fmt, template=None, columns=None, device=0):
    """SEG-Y trace records uint8 [ntr][240 + 4 ns] of ``section``: float32 [ntr][ns] (``layout`` 'trace') or [ns][ntr] ('slice', a
    ('twt', 'iline', 'xline') cube with the two line axes flattened), samples in format 1 (IBM) or 5 (IEEE).  Every header is ``template`` (240
    bytes, zeros by default) overlaid with ``columns``: field name -> one integer per trace (or a scalar)."""
    section = np.asarray(section)
    if section.ndim != 2:
        raise ValueError('the section is [ntraces][nsamples] or [nsamples][ntraces]')
    if layout not in _ffi.SEGY_LAYOUT:
        raise ValueError(f"layout {layout!r} (one of {sorted(_ffi.SEGY_LAYOUT)})")
    ntr = section.shape[0] if layout == 'trace' else section.shape[1]
    constants, _, table, values = header_columns(columns, ntr)
    return _ffi.segy_encode(section, layout, fmt, header_template(constants, template), table, values, device=device)


def decode_records(raw, ns, fmt, fields=(), device=0):
    """``(samples float32 [ntr][ns], {name: int64 array})`` of trace records ``raw`` uint8 [ntr][240 + ns x bytes(fmt)] in sample format 1, 2, 3, 5 or
    8; ``fields`` names the header words to scrape (at most 16 per call)."""
    fields = list(fields)
    table = []
    for name in fields:
        off, dt = _field(name)
        table.append((off, dt.itemsize, int(dt.kind == 'i')))
    samples, words = _ffi.segy_decode(raw, ns, fmt, table, device=device)
    out = {}
    for name, row in zip(fields, words):
        unsigned4 = FIELDS[name][1] == '>u4'
        out[name] = (row.view(np.uint32) if unsigned4 else row).astype(np.int64)
    return samples, out


def file_headers(ns, dt_ms, fmt, text='', binary=None):
    """The 3600 bytes in front of the traces: the textual header (EBCDIC, cut or padded to 3200 characters) and the binary header with Interval,
    Samples, Format, SEGYRevision, TraceFlag and ExtendedHeaders as ``segy.write_segy`` sets them, plus the words of ``binary`` (``BIN_ALL`` names)."""
    txt = text.encode('cp500', 'replace')[:S.TEXT_BYTES].ljust(S.TEXT_BYTES, ' '.encode('cp500'))
    binh = np.zeros(S.BIN_BYTES, np.uint8)
    words = {**(binary or {}), 'Interval': int(round(dt_ms * 1000)), 'Samples': ns, 'Format': fmt, 'SEGYRevision': 0x0100, 'TraceFlag': 1,
             'ExtendedHeaders': 0}
    for name, v in words.items():
        if name not in BIN_ALL:
            raise KeyError(f'{name!r} is not one of the binary-header fields {sorted(BIN_ALL)}')
        byte, dt = BIN_ALL[name]
        info = np.iinfo(np.dtype(dt))
        if not info.min <= v <= info.max:
            raise OverflowError(f'{name}: {v} is outside the range of a {info.bits}-bit binary-header word')
        lo = byte - 1 - S.TEXT_BYTES
        binh[lo:lo + np.dtype(dt).itemsize] = np.frombuffer(np.array(v, dt).tobytes(), np.uint8)
    return txt + binh.tobytes()


def _chunks(n, per):
    per = max(int(per), 1)
    return [(a, min(a + per, n)) for a in range(0, n, per)]


def write_cube_segy(path, cube_array, dims, headers=None, dt_ms=1.0, fmt=1, text='', binary=None, chunk_bytes=CHUNK_BYTES, device=0):
    """Write a cube as a 3-D SEG-Y file, one trace per (iline, xline) in C order.  ``cube_array`` is float32 with ``dims``
    ('iline', 'xline', 'twt') or ('twt', 'iline', 'xline'); neither is transposed on the host: the kernel reads both layouts.  ``headers``: field
    name -> [nil][nxl] or flat per-trace integers, or a scalar for all traces.  The file headers are written first, then the output file is
    mapped and filled chunk by chunk: whole inlines, about ``chunk_bytes`` of records each."""
    dims = tuple(dims)
    cube_array = np.asarray(cube_array)
    if cube_array.ndim != 3:
        raise ValueError('the cube has three axes')
    if dims == ('iline', 'xline', 'twt'):
        nil, nxl, ns = cube_array.shape
    elif dims == ('twt', 'iline', 'xline'):
        ns, nil, nxl = cube_array.shape
    else:
        raise ValueError(f"cube dimensions {dims}: ('iline', 'xline', 'twt') or ('twt', 'iline', 'xline')")
    if not 1 <= ns <= 65535:
        raise ValueError(f'{ns} samples per trace do not fit the 16-bit sample count of the SEG-Y headers (1 ... 65535)')
    if fmt not in (1, 5):
        raise ValueError(f'sample format {fmt}: 1 (IBM) or 5 (IEEE)')
    ntr, reclen = nil * nxl, S.TRACE_HEADER_BYTES + 4 * ns
    flat = {k: (np.asarray(v).reshape(-1) if np.ndim(v) else v) for k, v in (headers or {}).items()}
    constants, names, table, values = header_columns(flat, ntr)
    template = header_template(constants)
    head = file_headers(ns, dt_ms, fmt, text, binary)
    with open(path, 'wb') as fh:
        fh.write(head)
        fh.truncate(len(head) + ntr * reclen)
    if ntr == 0:
        return path
    out = np.memmap(path, np.uint8, 'r+', offset=len(head), shape=(ntr, reclen))
    for a, b in _chunks(nil, chunk_bytes // (nxl * reclen)):
        if dims[0] == 'iline':
            section, layout = cube_array[a:b].reshape(-1, ns), 'trace'
        else:
            section, layout = cube_array[:, a:b, :].reshape(ns, -1), 'slice'         # rows of whole inlines: a copy of runs, no transpose
        out[a * nxl:b * nxl] = _ffi.segy_encode(section, layout, fmt, template, table, values[:, a * nxl:b * nxl], device=device)
    out.flush()
    del out
    return path


def read_segy_gpu(path, fields=(), chunk_bytes=CHUNK_BYTES, device=0):
    """``(samples float32 [ntr][ns], {name: int64 array}, SegyFile)`` of a SEG-Y file: the records of ``SegyFile``'s memory map decoded on the
    device in chunks of about ``chunk_bytes``; ``fields`` names the header words to scrape."""
    src = S.SegyFile(path)
    fields = list(fields)
    ntr, ns, reclen = src.ntraces, src.ns, src._dtype.itemsize
    samples = np.empty((ntr, ns), np.float32)
    words = {name: np.empty(ntr, np.int64) for name in fields}
    if ntr:
        raw = np.memmap(path, np.uint8, 'r', offset=os.path.getsize(path) - ntr * reclen, shape=(ntr, reclen))
        for a, b in _chunks(ntr, chunk_bytes // reclen):
            samples[a:b], got = decode_records(raw[a:b], ns, src.format, fields, device=device)
            for name in fields:
                words[name][a:b] = got[name]
        del raw
    return samples, words, src
