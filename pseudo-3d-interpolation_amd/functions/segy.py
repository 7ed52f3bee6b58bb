"""Minimal SEG-Y reader and writer (NumPy only).

Layout: a 3200-byte textual header (EBCDIC or ASCII), a 400-byte binary header, ``n`` 3200-byte extended textual headers (binary
header bytes 3505-3506), then fixed-length traces of a 240-byte header and ``ns`` samples, all big-endian.  Sample formats 1 (IBM
float), 2 (int32), 3 (int16), 5 (IEEE float) and 8 (int8).  The file is memory-mapped as one structured array per trace, so headers
and samples are read without copying the file; samples are converted to float32 on access.

Trace header fields (1-based byte positions, the ones step 10 scrapes): 1 TRACE_SEQUENCE_LINE, 5 TRACE_SEQUENCE_FILE, 9 FieldRecord,
71 SourceGroupScalar, 73 SourceX, 77 SourceY, 109 DelayRecordingTime, 115 TRACE_SAMPLE_COUNT, 117 TRACE_SAMPLE_INTERVAL (microseconds); the ones
step 5 reads and writes: 61 SourceWaterDepth, 69 ElevationScalar, 103 TotalStaticApplied, 233 UnassignedInt1, 237 UnassignedInt2; the ones step 2
adds: 81 GroupX, 85 GroupY, 89 CoordinateUnits, 181 CDP_X, 185 CDP_Y; the recording time step 6 reads: 157 YearDataRecorded, 159 DayOfYear, 161 HourOfDay,
163 MinuteOfHour, 165 SecondOfMinute.  Step 4 writes a copy of a file with another trace length (`write_resized`)."""
import os

import numpy as np

TEXT_BYTES, BIN_BYTES, TRACE_HEADER_BYTES = 3200, 400, 240

# name: (1-based byte, big-endian dtype)
TRACE_FIELDS = {
    'TRACE_SEQUENCE_LINE': (1, '>i4'),
    'TRACE_SEQUENCE_FILE': (5, '>i4'),
    'FieldRecord': (9, '>i4'),
    'SourceWaterDepth': (61, '>i4'),
    'ElevationScalar': (69, '>i2'),
    'SourceGroupScalar': (71, '>i2'),
    'SourceX': (73, '>i4'),
    'SourceY': (77, '>i4'),
    'GroupX': (81, '>i4'),
    'GroupY': (85, '>i4'),
    'CoordinateUnits': (89, '>i2'),
    'TotalStaticApplied': (103, '>i2'),
    'DelayRecordingTime': (109, '>i2'),
    'TRACE_SAMPLE_COUNT': (115, '>u2'),
    'TRACE_SAMPLE_INTERVAL': (117, '>u2'),
    'YearDataRecorded': (157, '>i2'),
    'DayOfYear': (159, '>i2'),
    'HourOfDay': (161, '>i2'),
    'MinuteOfHour': (163, '>i2'),
    'SecondOfMinute': (165, '>i2'),
    'CDP_X': (181, '>i4'),
    'CDP_Y': (185, '>i4'),
    'UnassignedInt1': (233, '>i4'),
    'UnassignedInt2': (237, '>i4'),
}
# binary header: name: (1-based byte in the file, dtype)
BIN_FIELDS = {
    'Interval': (3217, '>u2'),
    'Samples': (3221, '>u2'),
    'SamplesOriginal': (3223, '>u2'),
    'Format': (3225, '>i2'),
    'SEGYRevision': (3501, '>u2'),
    'TraceFlag': (3503, '>i2'),
    'ExtendedHeaders': (3505, '>i2'),
}
SAMPLE_DTYPE = {1: '>u4', 2: '>i4', 3: '>i2', 5: '>f4', 8: 'i1'}


def ibm2ieee(words):
    """IBM System/360 single-precision words (uint32) -> float32: (-1)^s * 0.m (24 bits) * 16^(e - 64)."""
    u = np.asarray(words, dtype=np.uint32)
    sign = np.where(u >> 31, -1.0, 1.0)
    expo = ((u >> 24) & 0x7F).astype(np.int64)
    mant = (u & 0x00FFFFFF).astype(np.float64)
    return (sign * np.ldexp(mant, 4 * (expo - 64) - 24)).astype(np.float32)


def ieee2ibm(values):
    """float32 -> IBM words (uint32), mantissa rounded to nearest; |x| beyond the IBM range saturates, below it flushes to 0."""
    x = np.asarray(values, dtype=np.float64)
    a = np.abs(x)
    out = np.zeros(x.shape, np.uint32)
    nz = a > 0
    e = np.zeros(x.shape, np.int64)
    # a = m * 16^e with 1/16 <= m < 1
    e[nz] = np.floor(np.log2(a[nz]) / 4).astype(np.int64) + 1
    m = np.zeros(x.shape)
    m[nz] = np.ldexp(a[nz], -4 * e[nz])
    lo = nz & (m < 1.0 / 16)                 # log2 rounding at the edges
    e[lo] -= 1
    m[lo] *= 16
    hi = nz & (m >= 1.0)
    e[hi] += 1
    m[hi] /= 16
    mant = np.rint(np.ldexp(m, 24)).astype(np.int64)
    carry = mant >= (1 << 24)
    mant[carry] >>= 4
    e[carry] += 1
    biased = e + 64
    over = nz & (biased > 127)
    under = nz & (biased < 0)
    mant[over], biased[over] = 0xFFFFFF, 127
    ok = nz & ~under
    sign = (x < 0).astype(np.uint32) << 31
    out[ok] = (sign[ok] | (biased[ok].astype(np.uint32) << 24) | mant[ok].astype(np.uint32))
    return out


def _trace_dtype(ns, fmt):
    names, formats, offsets = [], [], []
    for name, (byte, dt) in TRACE_FIELDS.items():
        names.append(name)
        formats.append(dt)
        offsets.append(byte - 1)
    names.append('data')
    formats.append((SAMPLE_DTYPE[fmt], (ns,)))
    offsets.append(TRACE_HEADER_BYTES)
    return np.dtype({'names': names, 'formats': formats, 'offsets': offsets,
                     'itemsize': TRACE_HEADER_BYTES + ns * np.dtype(SAMPLE_DTYPE[fmt]).itemsize})


def _decode_text(raw):
    if raw[:1] == b'C' or raw[:1].isascii() and raw[:1].isalnum():
        return raw.decode('ascii', 'replace')
    return raw.decode('cp500', 'replace')


class SegyFile:
    """A memory-mapped SEG-Y file: ``text`` (str), ``binary`` (dict), ``headers`` (structured array of the trace-header fields),
    ``traces(rows)`` float32 samples [len(rows)][ns], ``dt`` (ms) and ``ns`` from the binary header."""

    def __init__(self, path):
        self.path = path
        with open(path, 'rb') as f:
            head = f.read(TEXT_BYTES + BIN_BYTES)
        if len(head) < TEXT_BYTES + BIN_BYTES:
            raise ValueError(f'{path}: shorter than the SEG-Y file headers')
        self.text = _decode_text(head[:TEXT_BYTES])
        self.binary = {k: int(np.frombuffer(head, dt, 1, b - 1)[0]) for k, (b, dt) in BIN_FIELDS.items()}
        fmt = self.binary['Format']
        if fmt not in SAMPLE_DTYPE:
            raise NotImplementedError(f'{path}: sample format {fmt} (supported: {sorted(SAMPLE_DTYPE)})')
        self.format, self.ns = fmt, self.binary['Samples']
        self.dt = self.binary['Interval'] / 1000.0
        start = TEXT_BYTES + BIN_BYTES + TEXT_BYTES * max(self.binary['ExtendedHeaders'], 0)
        self._dtype = _trace_dtype(self.ns, fmt)
        nbytes = np.memmap(path, np.uint8, 'r').size - start
        if nbytes < 0 or nbytes % self._dtype.itemsize:
            raise ValueError(f'{path}: {nbytes} trace bytes are not a whole number of {self._dtype.itemsize}-byte traces')
        self.reclen = self._dtype.itemsize                       # bytes of one trace record, header included
        self.ntraces = nbytes // self.reclen
        self._mm = np.memmap(path, self._dtype, 'r', offset=start, shape=(self.ntraces,))

    @property
    def headers(self):
        return self._mm[list(TRACE_FIELDS)]

    def header(self, name):
        return np.asarray(self._mm[name]).astype(np.int64)

    def traces(self, rows=None):
        raw = self._mm['data'] if rows is None else self._mm['data'][np.asarray(rows)]
        if self.format == 1:
            return ibm2ieee(raw)
        return np.asarray(raw).astype(np.float32)


def field_at(byte, missing_ok=False):
    """Name of the reader's trace-header field (``TRACE_FIELDS``) that starts at 1-based ``byte``; without one a ``KeyError``, or ``None``
    with ``missing_ok``."""
    for name, (b, _) in TRACE_FIELDS.items():
        if b == byte:
            return name
    if missing_ok:
        return None
    raise KeyError(f'no trace-header field at byte {byte}')


def header_words(segy, byte):
    """The trace-header word at 1-based ``byte`` of every trace.  A byte that starts one of the reader's named fields (``TRACE_FIELDS``) is
    read with that field's width; any other byte is read as a big-endian int16, the width of the delay time and its neighbours."""
    name = field_at(byte, missing_ok=True)
    if name is not None:
        return segy.header(name)
    if not 1 <= byte <= 239:
        raise ValueError(f'--byte_delay {byte} is outside the 240-byte trace header')
    raw = np.memmap(segy.path, np.uint8, 'r')
    start = raw.size - segy.ntraces * segy._dtype.itemsize
    rows = raw[start:].reshape(segy.ntraces, segy._dtype.itemsize)[:, byte - 1:byte + 1]
    return np.ascontiguousarray(rows).view('>i2').ravel().astype(np.int64)


def scaled_coordinates(scalar, x, y):
    """The header scalar rule of the reference (cube_binning_3D.py:657-668): the sign of the FIRST trace's scalar decides for all;
    negative: divide by |scalar|, otherwise multiply (a scalar of 0 gives 0, as there).  This is binning's rule; `functions.header.scale_coordinates`
    is the other one of the reference (reprojection's: a scalar of 0 leaves the coordinates as stored, and ``CoordinateUnits`` is honoured)."""
    scalar = np.asarray(scalar, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if scalar.size and scalar[0] < 0:
        return x / np.abs(scalar), y / np.abs(scalar)
    return x * scalar, y * scalar


def write_segy(path, data, dt_ms, fmt=5, headers=None, text='', binary=None):
    """Write float samples ``data`` [ntraces][ns] as a SEG-Y file (revision 1, fixed-length traces).  ``headers``: optional dict of
    trace-header field arrays (TRACE_FIELDS names); TRACE_SEQUENCE_LINE / _FILE default to 1 ... n, sample count and interval to the
    file's.  ``binary``: optional dict of further binary-header values (BIN_FIELDS names, e.g. SamplesOriginal); all others are zero."""
    data = np.asarray(data, dtype=np.float32)
    if data.ndim != 2:
        raise ValueError('data is [ntraces][nsamples]')
    ntr, ns = data.shape
    dtype = _trace_dtype(ns, fmt)
    rec = np.zeros(ntr, dtype)
    rec['TRACE_SEQUENCE_LINE'] = np.arange(1, ntr + 1)
    rec['TRACE_SEQUENCE_FILE'] = np.arange(1, ntr + 1)
    rec['TRACE_SAMPLE_COUNT'] = ns
    rec['TRACE_SAMPLE_INTERVAL'] = int(round(dt_ms * 1000))
    for k, v in (headers or {}).items():
        rec[k] = v
    if fmt == 1:
        rec['data'] = ieee2ibm(data)
    elif fmt == 5:
        rec['data'] = data
    else:
        info = np.iinfo(np.dtype(SAMPLE_DTYPE[fmt]))
        rec['data'] = np.clip(np.rint(data), info.min, info.max)
    txt = text.encode('cp500', 'replace')[:TEXT_BYTES].ljust(TEXT_BYTES, ' '.encode('cp500'))
    binh = np.zeros(BIN_BYTES, np.uint8)
    for k, v in {**(binary or {}), 'Interval': int(round(dt_ms * 1000)), 'Samples': ns, 'Format': fmt, 'SEGYRevision': 0x0100, 'TraceFlag': 1,
                 'ExtendedHeaders': 0}.items():
        b, dt = BIN_FIELDS[k]
        binh[b - 1 - TEXT_BYTES:b - 1 - TEXT_BYTES + np.dtype(dt).itemsize] = np.frombuffer(np.array(v, dt).tobytes(), np.uint8)
    with open(path, 'wb') as f:
        f.write(txt)
        f.write(binh.tobytes())
        f.write(rec.tobytes())
    return path


def _encode_samples(data, fmt):
    """float32 samples as the values of sample format ``fmt``: IBM words (1), IEEE floats (5), or integers rounded and clipped to the format's range."""
    if fmt == 1:
        return ieee2ibm(data)
    if fmt == 5:
        return data
    info = np.iinfo(np.dtype(SAMPLE_DTYPE[fmt]))
    return np.clip(np.rint(data), info.min, info.max)


def update_samples(path, data):
    """Overwrite the samples of an existing SEG-Y file in place with ``data`` [ntraces][ns] (float), encoded in the file's own sample
    format; the file, binary and trace headers are not touched.  IBM (1) and IEEE (5) floats and the integer formats are supported."""
    src = SegyFile(path)
    data = np.asarray(data, dtype=np.float32)
    if data.shape != (src.ntraces, src.ns):
        raise ValueError(f'{path}: holds {src.ntraces} traces of {src.ns} samples, got an array of shape {data.shape}')
    start = TEXT_BYTES + BIN_BYTES + TEXT_BYTES * max(src.binary['ExtendedHeaders'], 0)
    fmt, dtype = src.format, src._dtype
    del src
    mm = np.memmap(path, dtype, 'r+', offset=start, shape=(data.shape[0],))
    mm['data'] = _encode_samples(data, fmt)
    mm.flush()
    del mm
    return path


def update_headers(path, fields):
    """Overwrite trace-header words of an existing SEG-Y file in place: ``fields`` maps TRACE_FIELDS names to one value per trace (or a
    scalar for all traces).  Values must fit the field's width; samples and all other header bytes are not touched."""
    src = SegyFile(path)
    ntr, dtype = src.ntraces, src._dtype
    start = TEXT_BYTES + BIN_BYTES + TEXT_BYTES * max(src.binary['ExtendedHeaders'], 0)
    del src
    columns = {}
    for name, values in fields.items():
        if name not in TRACE_FIELDS:
            raise KeyError(f'{name!r} is not one of the trace-header fields {sorted(TRACE_FIELDS)}')
        values = np.broadcast_to(np.asarray(values), (ntr,)) if np.ndim(values) == 0 else np.asarray(values)
        if values.shape != (ntr,):
            raise ValueError(f'{path}: holds {ntr} traces, got {values.shape} values for {name}')
        info = np.iinfo(np.dtype(TRACE_FIELDS[name][1]))
        if values.size and (values.min() < info.min or values.max() > info.max):
            raise OverflowError(f'{name}: values outside the range of a {info.bits}-bit header word')
        columns[name] = values
    mm = np.memmap(path, dtype, 'r+', offset=start, shape=(ntr,))
    for name, values in columns.items():
        mm[name] = values
    mm.flush()
    del mm
    return path


def write_header_words(path, byte, rows, values):
    """Set the trace-header word at 1-based ``byte`` of traces ``rows`` to ``values``: with the width of the reader's named field that starts
    there, else as a big-endian int16 (the rule `header_words` reads by)."""
    segy = SegyFile(path)
    ntr, size = segy.ntraces, segy._dtype.itemsize
    name = field_at(byte, missing_ok=True)
    if name is not None:
        words = segy.header(name)
        del segy
        words[np.asarray(rows)] = values
        return update_headers(path, {name: words})
    del segy
    info = np.iinfo(np.int16)
    if np.min(values) < info.min or np.max(values) > info.max:
        raise OverflowError(f'byte {byte}: values outside the range of a 16-bit header word')
    raw = np.memmap(path, np.uint8, 'r+')
    start = raw.size - ntr * size
    packed = np.asarray(values).astype('>i2').reshape(-1, 1).view(np.uint8)
    raw[start:].reshape(ntr, size)[np.asarray(rows), byte - 1:byte + 1] = packed
    raw.flush()
    del raw
    return path


def write_resized(src_path, dst_path, data, fields=None):
    """Write ``data`` [ntraces][ns_new] (float) as the samples of a copy of the SEG-Y file ``src_path`` whose traces get a new length (step 4:
    zero-padded traces).  The textual header, the binary header, the extended textual headers and every 240-byte trace header are copied
    verbatim from the source but for: binary header ``Samples`` = ns_new and ``SamplesOriginal`` = the source's sample count; trace header
    ``TRACE_SAMPLE_COUNT`` = ns_new and the words of ``fields`` (TRACE_FIELDS names -> one value per trace or a scalar).  The samples are
    encoded in the source's own format.  A sample count beyond the 16 bits of the header words is an error."""
    src = SegyFile(src_path)
    data = np.asarray(data, dtype=np.float32)
    if data.ndim != 2 or data.shape[0] != src.ntraces:
        raise ValueError(f'{src_path}: holds {src.ntraces} traces, got an array of shape {data.shape}')
    ns_new = data.shape[1]
    if not 1 <= ns_new <= 65535:
        raise ValueError(f'{ns_new} samples per trace do not fit the 16-bit sample count of the SEG-Y headers (at most 65535)')
    if os.path.exists(dst_path) and os.path.samefile(src_path, dst_path):
        raise ValueError('a file cannot be resized in place: the output must be another file')
    start = TEXT_BYTES + BIN_BYTES + TEXT_BYTES * max(src.binary['ExtendedHeaders'], 0)
    fmt, ntr, ns_old, old_size = src.format, src.ntraces, src.ns, src._dtype.itemsize
    del src
    raw = np.memmap(src_path, np.uint8, 'r')
    head = np.array(raw[:start])
    for name, value in (('Samples', ns_new), ('SamplesOriginal', ns_old)):
        byte, dt = BIN_FIELDS[name]
        head[byte - 1:byte - 1 + np.dtype(dt).itemsize] = np.frombuffer(np.array(value, dt).tobytes(), np.uint8)
    dtype = _trace_dtype(ns_new, fmt)
    out = np.empty((ntr, dtype.itemsize), np.uint8)
    out[:, :TRACE_HEADER_BYTES] = raw[start:].reshape(ntr, old_size)[:, :TRACE_HEADER_BYTES]
    del raw
    rec = out.view(dtype).reshape(ntr)
    words = {'TRACE_SAMPLE_COUNT': ns_new}
    for name, values in (fields or {}).items():
        if name not in TRACE_FIELDS:
            raise KeyError(f'{name!r} is not one of the trace-header fields {sorted(TRACE_FIELDS)}')
        info = np.iinfo(np.dtype(TRACE_FIELDS[name][1]))
        if np.min(values) < info.min or np.max(values) > info.max:
            raise OverflowError(f'{name}: values outside the range of a {info.bits}-bit header word')
        words[name] = values
    for name, values in words.items():
        rec[name] = values
    rec['data'] = _encode_samples(data, fmt)
    with open(dst_path, 'wb') as f:
        f.write(head.tobytes())
        out.tofile(f)
    return dst_path
