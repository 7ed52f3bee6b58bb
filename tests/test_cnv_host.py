"""Host side of steps 9 and 16 (no GPU): the coordinate-scalar rule against the reference's own function (tests/golden/cnv.npz, recorded by
tests/golden/make_golden_cnv.py), both parsers with the reference's flags and defaults, the 40-card textual header, the overflow refusal of header
words, and the library's refusals that are decided before a device is looked for."""
import os

import numpy as np
import pytest

from conftest import load_golden

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd import cnv_segy2netcdf as cli9
from pseudo_3d_interpolation_amd import cube_cnv_netcdf2segy_3D as cli16
from pseudo_3d_interpolation_amd.functions import segy as S
from pseudo_3d_interpolation_amd.functions import segy_gpu as G
from pseudo_3d_interpolation_amd.functions.header import check_coordinate_scalar

needs_lib = pytest.mark.skipif(not os.path.isfile(_ffi.LIB_PATH), reason="libp3d_hip.so not built")


def test_coordinate_scalar_follows_the_reference():
    g = load_golden("cnv.npz")
    asked = [str(a) for a in g["asked"]]
    assert asked.count("auto") >= 10 and {"-1000", "-100", "-10", "0", "10", "100", "1000", "None"} <= set(asked)
    for a, x, y, scalar, mult in zip(asked, g["x"], g["y"], g["scalar"], g["mult"]):
        want = None if a == "None" else a if a == "auto" else int(a)
        got = check_coordinate_scalar(want, xcoords=np.array([[x, x + 1.0]]), ycoords=np.array([[y, y + 1.0]]))
        assert (float(got[0]), float(got[1])) == (float(scalar), float(mult)), (a, x, y, got)
    # the digit count is read off the text of the FIRST coordinate, so a leading minus sign counts: -23456.5 behaves as a 6-digit easting
    assert check_coordinate_scalar("auto", np.array([-23456.5]), np.array([1.5])) == check_coordinate_scalar("auto", np.array([123456.5]), np.array([1.5]))
    assert check_coordinate_scalar("auto", np.array([[1.5, 1e9]]), np.array([[2.5, 1e9]]))[1] == 10 ** 8
    with pytest.raises(ValueError):
        check_coordinate_scalar("automatic", np.array([1.5]), np.array([1.5]))


def test_step16_parser_has_the_flags_of_the_reference():
    p = cli16.define_input_args()
    a = p.parse_args(["cube.nc", "--params_netcdf", "nc.yml"])
    assert (a.path_cube, a.params_netcdf, a.path_segy, a.scalar_coords, a.verbose, a.format) == ("cube.nc", "nc.yml", None, "auto", 0, 1)
    a = p.parse_args(["cube.nc", "--params_netcdf", "nc.yml", "--path_segy", "o.sgy", "--scalar_coords", "-100", "-V", "--format", "5"])
    assert (a.path_segy, a.scalar_coords, a.verbose, a.format) == ("o.sgy", -100, 1, 5)
    for s in (-1000, -100, -10, 0, 10, 100, 1000):                               # the integers the reference lists (and rejects: type=str)
        assert p.parse_args(["c", "--params_netcdf", "y", "--scalar_coords", str(s)]).scalar_coords == s
    for bad in (["cube.nc"], ["c", "--params_netcdf", "y", "--scalar_coords", "5"], ["c", "--params_netcdf", "y", "--format", "2"],
                ["c", "--params_netcdf", "y", "-V", "3"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_step9_parser_has_the_flags_of_the_reference():
    p = cli9.define_input_args()
    a = p.parse_args(["lines"])
    assert (a.path_input, a.output_dir, a.suffix, a.filename_suffix, a.nprocesses, a.verbose, a.file_type) == ("lines", None, "sgy", None, 4, 0, "nc")
    a = p.parse_args(["list.txt", "-o", "out", "-s", "segy", "-fns", "despk", "--nprocesses", "8", "-V", "2", "--file_type", "npz"])
    assert (a.output_dir, a.suffix, a.filename_suffix, a.nprocesses, a.verbose, a.file_type) == ("out", "segy", "despk", 8, 2, "npz")
    with pytest.raises(SystemExit):
        p.parse_args(["lines", "--file_type", "zarr"])


def test_textual_header_holds_the_forty_cards():
    text = cli16.textual_header("2024-02-29T12:00:00", "someone", 100, "2024-01-01: STEP A\n2024-01-02: STEP B")
    assert len(text) == 3200
    cards = [text[k:k + 80] for k in range(0, 3200, 80)]
    assert [c[:4] for c in cards] == [f"C{k:02d} " for k in range(1, 41)]
    body = {k + 1: c[4:].rstrip() for k, c in enumerate(cards)}
    want = {1: "3D SEG-Y CONVERTED FROM NETCDF USING PSEUDO_3D_INTERPOLATION_AMD", 4: "EVOKER: someone", 10: "*** PROCESSING STEPS ***",
            11: "2024-01-01: STEP A", 12: "2024-01-02: STEP B", 35: "*** BYTE LOCATION OF KEY HEADERS ***", 36: "CDP: 21  FOLD: 33",
            37: "CDP UTM-X: 181 CDP UTM-Y: 185 ALL COORDS SCALED BY: 100", 38: "INLINE: 189, XLINE: 193", 40: "END TEXTUAL HEADER"}
    for k in range(1, 41):
        if k != 3:                                                               # the timestamp card
            assert body[k] == want.get(k, ""), k
    assert body[3].startswith("CREATION: ")
    assert text.encode("cp500").decode("cp500") == text
    # no text attribute: cards 11 ... 34 stay empty; a long line is cut to the 75 characters the reference fills; many lines run on into the later cards
    bare = cli16.textual_header("t", "u", 0.1)
    assert all(not bare[80 * k + 4:80 * k + 80].strip() for k in range(10, 34)) and "SCALED BY: 0.1" in bare
    long = cli16.textual_header("t", "u", 1, "\n".join(["x" * 90] + [f"line {k}" for k in range(40)]))
    assert len(long) == 3200 and long[80 * 10 + 4:80 * 11] == "x" * 75 + " " and long[80 * 39 + 4:].rstrip() == "line 28"
    assert isinstance(cli16.user_name(), str) and cli16.user_name()


def test_trace_headers_of_a_small_cube():
    iline, xline, twt = np.array([10, 12, 14]), np.array([5.0, 6.0]), np.array([20.0, 20.5, 21.0, 21.5])
    x = np.array([[500000.25, 500001.5], [500002.5, 500003.5], [-1.25, 0.0]])
    w = cli16.trace_headers(iline, xline, x, x + 1000, -100, 100, np.arange(6).reshape(3, 2), twt, 0.5)
    assert w["CDP"].tolist() == [1, 2, 3, 4, 5, 6] == w["TRACE_SEQUENCE_LINE"].tolist() == w["TRACE_SEQUENCE_FILE"].tolist()
    assert w["INLINE_3D"].tolist() == [10, 10, 12, 12, 14, 14] and w["CROSSLINE_3D"].tolist() == [5, 6, 5, 6, 5, 6]
    assert w["CDP_X"].tolist() == [50000025, 50000150, 50000250, 50000350, -125, 0] and w["CDP_Y"][0] == 50100025
    assert (w["SourceGroupScalar"], w["DelayRecordingTime"], w["TRACE_SAMPLE_COUNT"], w["TRACE_SAMPLE_INTERVAL"]) == (-100, 20, 4, 500)
    assert w["NStackedTraces"].tolist() == [0, 1, 2, 3, 4, 5]
    assert "DelayRecordingTime" not in cli16.trace_headers(iline, xline, x, x, 0, 1, None, twt + 40000, 0.5)        # beyond 16 bits: left at 0
    with pytest.raises(ValueError):
        cli16.trace_headers(np.array([1.5, 2.5, 3.5]), xline, x, x, 0, 1, None, twt, 0.5)


def test_header_words_that_do_not_fit_are_refused_on_the_host():
    x = np.array([[412345.25, 412346.25]])
    scalar, factor = check_coordinate_scalar(-1000, x, x)
    ok = cli16.trace_headers([1], [1, 2], x, x, scalar, factor, None, [0.0], 1.0)
    constants, names, table, values = G.header_columns(ok, 2)
    assert values.dtype == np.int32 and values.shape == (len(names), 2) and constants["SourceGroupScalar"] == -1000
    assert table[names.index("CDP_X")] == (180, 4) and values[names.index("CDP_X")].tolist() == [412345250, 412346250]
    big = cli16.trace_headers([1], [1, 2], x * 10, x, scalar, factor, None, [0.0], 1.0)                            # 4 123 452 500 > 2^31 - 1
    with pytest.raises(OverflowError):
        G.header_columns(big, 2)
    with pytest.raises(OverflowError):
        G.header_columns({"NStackedTraces": np.array([1, 40000])}, 2)
    with pytest.raises(OverflowError):
        G.header_columns({"SourceGroupScalar": -100000000}, 2)                   # what 'auto' gives for sub-unit coordinates
    with pytest.raises(KeyError):
        G.header_columns({"NoSuchWord": 1}, 2)
    with pytest.raises(ValueError):
        G.header_columns({"CDP": np.array([1.5, 2.0])}, 2)
    assert set(G.EXTRA_FIELDS) == {"CDP", "NStackedTraces", "INLINE_3D", "CROSSLINE_3D"} and not set(G.EXTRA_FIELDS) & set(S.TRACE_FIELDS)
    assert [G.FIELDS[k][0] for k in ("CDP", "NStackedTraces", "INLINE_3D", "CROSSLINE_3D")] == [21, 33, 189, 193]
    tmpl = G.header_template({"TRACE_SAMPLE_COUNT": 40000, "SourceGroupScalar": -100})
    assert tmpl[114:116].tolist() == [0x9C, 0x40] and tmpl[70:72].tolist() == [0xFF, 0x9C] and tmpl.sum() == 0x9C + 0x40 + 0xFF + 0x9C
    head = G.file_headers(37, 0.5, 1, "C01 X", {"IntervalOriginal": 250, "SortingCode": 2, "MeasurementSystem": 1})
    assert len(head) == 3600 and head[:5].decode("cp500") == "C01 X"
    assert [int.from_bytes(head[b - 1:b + 1], "big") for b in (3217, 3219, 3221, 3225, 3229, 3255, 3501, 3503)] == [500, 250, 37, 1, 2, 1, 0x0100, 1]


def test_seisnc_without_h5py_is_a_clear_import_error(tmp_path):
    from pseudo_3d_interpolation_amd.functions.backends import h5py_enabled
    if h5py_enabled:
        pytest.skip("h5py is installed: the .seisnc writer is available")
    with pytest.raises(ImportError, match="--file_type npz"):
        cli9.convert(str(tmp_path / "missing.sgy"), str(tmp_path), "nc")          # decided before the file is opened


@needs_lib
def test_the_library_refuses_bad_arguments_without_a_device():
    sec, tmpl = np.zeros((2, 3), np.float32), np.zeros(240, np.uint8)
    cases = [lambda: _ffi.segy_decode(np.zeros((1, 240), np.uint8), 0, 5, []),
             lambda: _ffi.segy_decode(np.zeros((1, 240 + 4 * 65536), np.uint8), 65536, 5, []),
             lambda: _ffi.segy_decode(np.zeros((1, 244), np.uint8), 1, 4, []),
             lambda: _ffi.segy_decode(np.zeros((1, 244), np.uint8), 1, 5, [(4 * k, 2, 1) for k in range(17)]),
             lambda: _ffi.segy_decode(np.zeros((1, 244), np.uint8), 1, 5, [(8, 4, 1), (10, 2, 0)]),
             lambda: _ffi.segy_encode(np.zeros((2, 0), np.float32), "trace", 1, tmpl, [], []),
             lambda: _ffi.segy_encode(np.zeros((2, 65536), np.float32), "trace", 1, tmpl, [], []),
             lambda: _ffi.segy_encode(sec, "trace", 4, tmpl, [], []),
             lambda: _ffi.segy_encode(sec, "trace", 1, tmpl, [(4 * k, 4) for k in range(17)], np.zeros((17, 2), np.int32)),
             lambda: _ffi.segy_encode(sec, "trace", 1, tmpl, [(0, 4), (2, 2)], np.zeros((2, 2), np.int32)),
             lambda: _ffi.segy_encode(sec, "trace", 1, tmpl, [(238, 4)], np.zeros((1, 2), np.int32)),
             lambda: _ffi.check(_ffi.lib().p3d_segy_encode(0, _ffi._ptr(sec), 2, 3, 2, 1, _ffi._ptr(tmpl), None, 0, None, _ffi._ptr(np.zeros(504, np.uint8))))]
    for k, call in enumerate(cases):
        with pytest.raises(_ffi.P3DError) as err:
            call()
        assert err.value.code == _ffi.P3D_ERR_INVALID, (k, str(err.value))
    assert _ffi.lib().p3d_abi_version() == 1
