"""The SEG-Y codec kernels (csrc/p3d_segy.hip) against the project's host codec functions/segy.py, byte for byte and bit for bit.

Shapes (ntr, ns): (1, 1), (3, 5), (31, 67), (33, 128), (65, 1027), (200, 3) -- below and across the 64 x 64 transpose tile in both directions, records
of 60 + ns words with ns % 4 == 0 (16-byte stores and loads) and ns % 4 != 0 (4-byte ones), more than one workgroup along traces and along words.
Samples: the edge list of test_segy_codec_host.py (zeros, subnormals, FLT_MIN / FLT_MAX, powers of 16, mantissas that round up, NaN, +-Inf)
followed by random bit patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_segy_codec_host import edge_words

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import segy as S
from pseudo_3d_interpolation_amd.functions import segy_gpu as G

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 5), (31, 67), (33, 128), (65, 1027), (200, 3)]
TEMPLATE = ((np.arange(240) * 7 + 13) % 256).astype(np.uint8)                   # 7 is coprime to 256: 240 distinct bytes
COLUMNS = [(0, 4), (20, 4), (70, 2), (114, 2), (188, 4), (236, 4)]
FIELDS = [(0, 4, 1), (20, 4, 1), (70, 2, 1), (114, 2, 0), (188, 4, 1), (236, 4, 0)]
assert np.unique(TEMPLATE).size == 240


def sample_bits(ntr, ns, seed):
    edges = edge_words()
    bits = np.random.default_rng(seed).integers(0, 2**32, ntr * ns, dtype=np.uint64).astype(np.uint32)
    n = min(edges.size, bits.size)
    bits[:n] = edges[:n]
    return bits.reshape(ntr, ns)


def column_values(ntr, seed):
    rng = np.random.default_rng(seed)
    vals = np.stack([rng.integers(-2**31, 2**31, ntr) if w == 4 else rng.integers(-2**15, 2**15, ntr) for _, w in COLUMNS]).astype(np.int32)
    vals[:, 0] = [-1, -2**31, -2, -2**15, 2**31 - 1, -123456789]
    return vals


def host_ibm(bits):
    """segy.ieee2ibm where it is defined (finite values; NaN gives 0 there too); +-Inf by the definition of include/p3d.h."""
    x = bits.view(np.float32)
    want = np.zeros(bits.shape, np.uint32)
    finite = np.isfinite(x)
    want[finite] = S.ieee2ibm(x[finite])
    want[x == np.inf], want[x == -np.inf] = 0x7FFFFFFF, 0xFFFFFFFF
    return want


def host_records(bits, fmt, values):
    """The records assembled with NumPy: the template, the columns as big-endian words, the samples through segy.ieee2ibm."""
    ntr, ns = bits.shape
    rec = np.empty((ntr, 240 + 4 * ns), np.uint8)
    rec[:, :240] = TEMPLATE
    for (off, width), v in zip(COLUMNS, values):
        rec[:, off:off + width] = v.astype('>i4' if width == 4 else '>i2').view(np.uint8).reshape(ntr, width)
    rec[:, 240:] = (host_ibm(bits) if fmt == 1 else bits).astype('>u4').view(np.uint8).reshape(ntr, 4 * ns)
    return rec


@pytest.mark.parametrize("fmt", [1, 5])
@pytest.mark.parametrize("layout", ["trace", "slice"])
@pytest.mark.parametrize("ntr,ns", SHAPES)
def test_encode_is_byte_identical_to_the_host_assembly(ntr, ns, layout, fmt):
    bits, values = sample_bits(ntr, ns, 100 * ntr + ns), column_values(ntr, ntr)
    section = bits.view(np.float32) if layout == "trace" else np.ascontiguousarray(bits.T).view(np.float32)
    got = _ffi.segy_encode(section, layout, fmt, TEMPLATE, COLUMNS, values)
    want = host_records(bits, fmt, values)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    plain = _ffi.segy_encode(section, layout, fmt, TEMPLATE, [], [])             # no columns: the template alone
    assert np.array_equal(plain[:, :240], np.broadcast_to(TEMPLATE, (ntr, 240))) and np.array_equal(plain[:, 240:], want[:, 240:])


def segy_file(path, raw, ns, fmt):
    binh = np.zeros(400, np.uint8)
    for name, v in (("Samples", ns), ("Format", fmt), ("Interval", 1000)):
        byte, dt = S.BIN_FIELDS[name]
        binh[byte - 3201:byte - 3201 + 2] = np.frombuffer(np.array(v, dt).tobytes(), np.uint8)
    with open(path, "wb") as fh:
        fh.write(b" " * 3200 + binh.tobytes() + raw.tobytes())
    return S.SegyFile(str(path))


@pytest.mark.parametrize("fmt", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("ntr,ns", SHAPES)
def test_decode_is_bit_identical_to_segyfile(tmp_path, ntr, ns, fmt):
    bps = _ffi.SEGY_SAMPLE_BYTES[fmt]
    raw = np.random.default_rng(1000 * fmt + ntr + ns).integers(0, 256, (ntr, 240 + ns * bps), dtype=np.uint8)
    if bps == 4:
        raw[:, 240:] = sample_bits(ntr, ns, fmt).astype('>u4').view(np.uint8).reshape(ntr, 4 * ns)
    with np.errstate(over="ignore"):
        want = segy_file(tmp_path / "f.sgy", raw, ns, fmt).traces()
    got, words = _ffi.segy_decode(raw, ns, fmt, FIELDS)
    assert got.shape == (ntr, ns) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for (off, width, signed), row in zip(FIELDS, words):
        dt = ('>i' if signed else '>u') + str(width)
        ref = np.array([np.frombuffer(raw[x].tobytes(), dt, 1, off)[0] for x in range(ntr)])
        assert np.array_equal(row.view(np.uint32) if dt == '>u4' else row, ref), (off, width, signed)
    alone, none = _ffi.segy_decode(raw, ns, fmt, [])
    assert none.shape == (0, ntr) and np.array_equal(alone.view(np.uint32), want.view(np.uint32))


def test_a_million_random_ibm_words_decode_bit_identically():
    words = np.random.default_rng(42).integers(0, 2**32, 2**20, dtype=np.uint64).astype(np.uint32)
    raw = np.zeros((1024, 240 + 4096), np.uint8)
    raw[:, 240:] = words.astype('>u4').view(np.uint8).reshape(1024, 4096)
    got, _ = _ffi.segy_decode(raw, 1024, 1, [])
    with np.errstate(over="ignore"):
        want = S.ibm2ieee(words).view(np.uint32)
    assert np.array_equal(got.view(np.uint32).ravel(), want)
    assert np.isinf(got).mean() > 0.2                                            # bits, not allclose: a quarter of the words are beyond float32


def test_no_traces_is_a_no_op():
    assert _ffi.segy_encode(np.zeros((0, 8), np.float32), "trace", 1, TEMPLATE, COLUMNS, np.zeros((6, 0), np.int32)).shape == (0, 272)
    assert _ffi.segy_encode(np.zeros((8, 0), np.float32), "slice", 5, TEMPLATE, [], []).shape == (0, 272)
    samples, words = _ffi.segy_decode(np.zeros((0, 240 + 16), np.uint8), 8, 3, FIELDS)
    assert samples.shape == (0, 8) and words.shape == (6, 0)
    _ffi.segy_encode_dev(None, 0, 8, "trace", 1, None, [], None, None)           # nothing is touched
    _ffi.segy_decode_dev(None, 0, 8, 1, [], None, None)


def test_refusals_reach_the_caller_before_anything_is_launched():
    sec = np.zeros((4, 8), np.float32)
    for kw in (dict(fmt=2), dict(columns=[(0, 4), (3, 2)]), dict(columns=[(238, 4)]), dict(columns=[(0, 3)]), dict(columns=[(4 * k, 2) for k in range(17)])):
        cols = kw.get("columns", [])
        with pytest.raises(_ffi.P3DError):
            _ffi.segy_encode(sec, "trace", kw.get("fmt", 1), TEMPLATE, cols, np.zeros((len(cols), 4), np.int32))
    with pytest.raises(_ffi.P3DError):
        _ffi.segy_decode(np.zeros((4, 240 + 32), np.uint8), 8, 4, [])
    with pytest.raises(_ffi.P3DError):
        _ffi.check(_ffi.lib().p3d_segy_encode(0, _ffi._ptr(sec), 4, 8, 2, 1, _ffi._ptr(TEMPLATE), None, 0, None, _ffi._ptr(np.zeros((4, 272), np.uint8))))


def test_dev_entries_on_device_arrays_agree_with_the_host_entries():
    ntr, ns = 65, 1027
    bits, values = sample_bits(ntr, ns, 5), column_values(ntr, 5)
    bufs = [_ffi.DeviceArray(s, d) for s, d in (((ntr, ns), np.float32), ((240,), np.uint8), (values.shape, np.int32), ((ntr, 240 + 4 * ns), np.uint8),
                                                ((ntr, ns), np.float32), ((len(FIELDS), ntr), np.int32))]
    try:
        dsec, dtmpl, dval, drec, dback, dwords = bufs
        dsec.upload(bits.view(np.float32)), dtmpl.upload(TEMPLATE), dval.upload(values)
        _ffi.segy_encode_dev(dsec.ptr, ntr, ns, "trace", 1, dtmpl.ptr, COLUMNS, dval.ptr, drec.ptr)
        rec = drec.download()
        assert np.array_equal(rec, _ffi.segy_encode(bits.view(np.float32), "trace", 1, TEMPLATE, COLUMNS, values))
        _ffi.segy_decode_dev(drec.ptr, ntr, ns, 1, FIELDS, dback.ptr, dwords.ptr)
        samples, words = _ffi.segy_decode(rec, ns, 1, FIELDS)
        assert np.array_equal(dback.download().view(np.uint32), samples.view(np.uint32)) and np.array_equal(dwords.download(), words)
        with pytest.raises(_ffi.P3DError):
            _ffi.segy_encode_dev(dsec.ptr + 4, ntr - 1, ns, "trace", 1, dtmpl.ptr, COLUMNS, dval.ptr, drec.ptr)      # not at a 16-byte boundary
    finally:
        for b in bufs:
            b.free()


TORCH_CHILD = r"""
import sys
import torch                                      # first: this process uses torch.cuda, see _ffi._preload_torch_hip
import numpy as np
sys.path.insert(0, sys.argv[1])
from pseudo_3d_interpolation_amd import _ffi
ntr, ns = 33, 128
rng = np.random.default_rng(3)
sec = rng.standard_normal((ns, ntr)).astype(np.float32)
tmpl = rng.integers(0, 256, 240, dtype=np.uint8)
cols, vals = [(4, 4), (70, 2)], rng.integers(-30000, 30000, (2, ntr)).astype(np.int32)
fields = [(4, 4, 1), (70, 2, 1)]
dev = torch.device("cuda:0")
tsec, ttmpl, tvals = (torch.from_numpy(a).to(dev) for a in (sec, tmpl, vals))
trec = torch.empty((ntr, 240 + 4 * ns), dtype=torch.uint8, device=dev)
tback, twords = torch.empty((ntr, ns), dtype=torch.float32, device=dev), torch.empty((2, ntr), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
for fmt in (1, 5):
    _ffi.segy_encode_dev(tsec.data_ptr(), ntr, ns, "slice", fmt, ttmpl.data_ptr(), cols, tvals.data_ptr(), trec.data_ptr())
    rec = _ffi.segy_encode(sec, "slice", fmt, tmpl, cols, vals)
    assert np.array_equal(trec.cpu().numpy(), rec), fmt
    _ffi.segy_decode_dev(trec.data_ptr(), ntr, ns, fmt, fields, tback.data_ptr(), twords.data_ptr())
    samples, words = _ffi.segy_decode(rec, ns, fmt, fields)
    assert np.array_equal(tback.cpu().numpy().view(np.uint32), samples.view(np.uint32)), fmt
    assert np.array_equal(twords.cpu().numpy(), words) and np.array_equal(words, vals), fmt
print("TORCH OK")
"""


def test_dev_entries_on_torch_tensors_agree_with_the_host_entries():
    """In a process of its own: one that uses torch.cuda has to import torch before the library binds its HIP runtime."""
    pytest.importorskip("torch")
    res = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TORCH OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def test_chunked_cube_file_equals_the_one_chunk_file(tmp_path):
    nil, nxl, ns = 7, 5, 37
    rng = np.random.default_rng(9)
    cube = rng.standard_normal((ns, nil, nxl)).astype(np.float32)
    headers = {"TRACE_SEQUENCE_FILE": np.arange(1, nil * nxl + 1), "INLINE_3D": np.repeat(np.arange(nil) + 100, nxl).reshape(nil, nxl),
               "CDP_X": rng.integers(-2**31, 2**31, (nil, nxl)), "NStackedTraces": rng.integers(0, 200, (nil, nxl)), "TRACE_SAMPLE_COUNT": ns}
    reclen = 240 + 4 * ns
    one = G.write_cube_segy(str(tmp_path / "one.sgy"), cube, ("twt", "iline", "xline"), headers, 0.5, fmt=1, text="C 1 TEST")
    many = G.write_cube_segy(str(tmp_path / "many.sgy"), cube, ("twt", "iline", "xline"), headers, 0.5, fmt=1, text="C 1 TEST",
                             chunk_bytes=3 * nxl * reclen)                       # 3 + 3 + 1 inlines
    other = G.write_cube_segy(str(tmp_path / "other.sgy"), np.ascontiguousarray(cube.transpose(1, 2, 0)), ("iline", "xline", "twt"), headers, 0.5, fmt=1,
                              text="C 1 TEST", chunk_bytes=2 * nxl * reclen)     # 2 + 2 + 2 + 1
    blob = open(one, "rb").read()
    assert len(blob) == 3600 + nil * nxl * reclen and open(many, "rb").read() == blob and open(other, "rb").read() == blob
    f = S.SegyFile(one)
    assert f.ns == ns and f.format == 1 and f.ntraces == nil * nxl and f.header("CDP_X").tolist() == headers["CDP_X"].ravel().tolist()
    assert np.array_equal(f.traces(), S.ibm2ieee(S.ieee2ibm(cube.reshape(ns, -1).T)))
    samples, words, _ = G.read_segy_gpu(one, ["INLINE_3D", "NStackedTraces", "TRACE_SAMPLE_COUNT"], chunk_bytes=4 * reclen)
    assert np.array_equal(samples, f.traces()) and words["INLINE_3D"].tolist() == headers["INLINE_3D"].ravel().tolist()
    assert words["NStackedTraces"].tolist() == headers["NStackedTraces"].ravel().tolist() and set(words["TRACE_SAMPLE_COUNT"].tolist()) == {ns}
    with pytest.raises(OverflowError):
        G.write_cube_segy(str(tmp_path / "bad.sgy"), cube, ("twt", "iline", "xline"), {"CDP_X": np.full((nil, nxl), 2**31)}, 0.5)
