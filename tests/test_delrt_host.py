"""Steps 3 and 4 without a GPU: the decision of the correction against the whole recorded decision table of the reference, the host arithmetic of
the padding against the fixtures, `write_resized`, both parsers against the reference's flag lists, output naming and the skip path, and the two
documented departures of step 3 (with the device call replaced by its NumPy restatement, tests/helpers/delrt_numpy.py).  Fixtures:
tests/golden/delrt.npz (make_golden_delrt.py).  The reference's ``sys.exit`` ('... really messed up ...') never fired while the table was
recorded (``table/exit_fired`` is 0: with the boundary condition met, the offset trace always lies on one side), so the RuntimeError that stands
for it here is raised by no recorded row."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import delrt_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd import delrt_correction_segy as cli3  # noqa: E402
from pseudo_3d_interpolation_amd import delrt_padding_segy as cli4  # noqa: E402
from pseudo_3d_interpolation_amd.functions import delrt as D  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy_cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions.header import get_textual_header  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'delrt.npz'))
DT = 0.25


def numpy_windows(subsets, n_samples, device=0):
    """`_ffi.delrt_windows` on the CPU."""
    m, width, _ = subsets.shape
    data = subsets.reshape(m * width, -1).T
    return H.windows(data, H.packed_ref(m, width // 2), width // 2, n_samples)


def test_decision_matches_the_reference_on_the_whole_table():
    t = {k: G[f'table/{k}'] for k in ('n_traces', 'width', 'maxima', 'peak_val', 'delrt', 'kind', 'delay', 'index')}
    assert int(G['table/exit_fired']) == 0 and t['kind'].size > 2000 and set(t['kind'].tolist()) == {0, 1}
    assert set(zip(t['n_traces'].tolist(), t['width'].tolist())) == {(1, 3), (1, 2), (2, 5), (2, 4), (3, 7), (3, 6)}
    for r in range(t['kind'].size):
        n, w = int(t['n_traces'][r]), int(t['width'][r])
        maxima = t['maxima'][r, :w].copy()
        got = D.decide_delay(maxima, t['peak_val'][r], t['delrt'][r, :w], n)
        want = (None, None) if t['kind'][r] == 0 else (t['delay'][r], t['index'][r])
        assert got == want, (r, n, w, t['maxima'][r, :w], t['delrt'][r, :w], got, want)
        assert np.array_equal(maxima, t['maxima'][r, :w])          # the caller's array is not clipped in place
    found = t['kind'] == 1
    assert np.any(t['index'][found] < t['n_traces'][found]) and np.any(t['index'][found] > t['n_traces'][found]) and np.any(t['index'][found] == t['n_traces'][found])


@pytest.mark.parametrize('name', [str(n) for n in G['pad/cases']])
def test_padding_host_arithmetic(name):
    c = {k: G[f'pad/{name}/{k}'] for k in ('delays', 'ns', 'dt', 'twt_padded', 'n_samples_padded', 'idx_delay', 'min_delay', 'max_delay', 'top')}
    ns, dt = int(c['ns']), float(c['dt'])
    twt = np.arange(ns) * dt + c['delays'][0]
    twt_padded, top, idx_delay, dmin, dmax = D.pad_layout(c['delays'], dt, twt)
    assert twt_padded.tobytes() == c['twt_padded'].tobytes() and len(twt_padded) == int(c['n_samples_padded'])
    assert top.dtype == np.int32 and np.array_equal(top, c['top']) and np.array_equal(idx_delay, c['idx_delay'])
    assert dmin == c['min_delay'] and dmax == c['max_delay']
    data = G['pad/section'][:ns, :top.size].copy()
    data[-1] = np.where(data[-1] == 0, 1 / 512, data[-1])
    assert H.pad(data, top, len(twt_padded)).tobytes() == G[f'pad/{name}/data_padded'].tobytes()       # the restatement is the reference's padding


def test_padding_host_checks():
    assert D.delay_changes(np.array([5, 5, 5])).tolist() == [0] and D.delay_changes(np.array([5, 7, 5])).tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match='do not fit the padded axis'):        # a time axis that is too short for the delays: no device call
        D.pad_trace_data(np.ones((8, 3), np.float32), np.array([0, 4, 0]), 3, 1.0, np.arange(4.0))
    with pytest.raises(ValueError):
        D.pad_trace_data(np.ones((8, 3), np.float32), np.array([0, 4]), 3, 1.0, np.arange(8.0))
    with pytest.raises(ValueError):
        D.pad_trace_data(np.ones(8, np.float32), np.array([0]), 1, 1.0, np.arange(8.0))


@pytest.mark.parametrize('fmt', [1, 3, 5])
def test_write_resized_round_trip(tmp_path, fmt):
    rng = np.random.default_rng(fmt)
    ntr, ns, ns_new = 7, 11, 19
    data = rng.integers(-200, 200, (ntr, ns)).astype(np.float32) * (1 if fmt == 3 else 0.125)
    text = 'C 1 SOME CLIENT'.ljust(80) + 'C 2 LINE 7'.ljust(80)
    src = S.write_segy(str(tmp_path / 'a.sgy'), data, DT, fmt=fmt, text=text, binary={'ExtendedHeaders': 0},
                       headers={'DelayRecordingTime': np.arange(ntr) + 10, 'FieldRecord': np.arange(ntr) + 100, 'SourceX': np.arange(ntr) * 1000})
    raw = bytearray(open(src, 'rb').read())
    size = 240 + ns * np.dtype(S.SAMPLE_DTYPE[fmt]).itemsize
    for x in range(ntr):                                            # bytes of the trace headers that the reader has no name for
        raw[3600 + x * size + 180:3600 + x * size + 232] = bytes((x * 7 + k) % 251 for k in range(52))
    raw[3300:3320] = bytes(range(20))                              # ... and of the binary header
    open(src, 'wb').write(bytes(raw))
    new = np.zeros((ntr, ns_new), np.float32)
    new[:, 3:3 + ns] = data
    dst = S.write_resized(src, str(tmp_path / 'b.sgy'), new, fields={'DelayRecordingTime': 10})
    a, b = S.SegyFile(src), S.SegyFile(dst)
    assert b.ns == ns_new and b.ntraces == ntr and b.format == fmt and b.binary['SamplesOriginal'] == ns and b.binary['Samples'] == ns_new
    assert b.traces().tobytes() == new.tobytes() and a.traces().tobytes() == data.tobytes()
    assert b.header('TRACE_SAMPLE_COUNT').tolist() == [ns_new] * ntr and b.header('DelayRecordingTime').tolist() == [10] * ntr
    out = open(dst, 'rb').read()
    size_new = 240 + ns_new * np.dtype(S.SAMPLE_DTYPE[fmt]).itemsize
    assert len(out) == 3600 + ntr * size_new
    head_a, head_b = bytearray(raw[:3600]), bytearray(out[:3600])
    for lo in (3220, 3222):                                         # Samples, SamplesOriginal
        head_a[lo:lo + 2] = head_b[lo:lo + 2] = b'\0\0'
    assert head_a == head_b
    for x in range(ntr):
        ha, hb = bytearray(raw[3600 + x * size:3600 + x * size + 240]), bytearray(out[3600 + x * size_new:3600 + x * size_new + 240])
        for lo in (108, 114):                                       # DelayRecordingTime, TRACE_SAMPLE_COUNT
            ha[lo:lo + 2] = hb[lo:lo + 2] = b'\0\0'
        assert ha == hb, x
    with pytest.raises(ValueError, match='65535'):
        S.write_resized(src, str(tmp_path / 'c.sgy'), np.zeros((ntr, 65536), np.float32))
    with pytest.raises(ValueError):
        S.write_resized(src, str(tmp_path / 'c.sgy'), np.zeros((ntr + 1, ns_new), np.float32))
    with pytest.raises(ValueError, match='in place'):
        S.write_resized(src, src, new)
    assert not os.path.exists(tmp_path / 'c.sgy')


def test_write_resized_keeps_extended_textual_headers(tmp_path):
    data = np.arange(12, dtype=np.float32).reshape(3, 4)
    src = S.write_segy(str(tmp_path / 'a.sgy'), data, DT)
    raw = open(src, 'rb').read()
    ext = bytes((k * 13) % 256 for k in range(3200))
    head = bytearray(raw[:3600])
    head[3504:3506] = (1).to_bytes(2, 'big')
    open(src, 'wb').write(bytes(head) + ext + raw[3600:])
    assert S.SegyFile(src).traces().tobytes() == data.tobytes()
    dst = S.write_resized(src, str(tmp_path / 'b.sgy'), np.pad(data, ((0, 0), (0, 2))))
    out = open(dst, 'rb').read()
    assert out[3600:6800] == ext and S.SegyFile(dst).traces().tobytes() == np.pad(data, ((0, 0), (0, 2))).tobytes()


@pytest.mark.parametrize('key,cli,count', [('correction', cli3, 10), ('padding', cli4, 7)])
def test_cli_flags_are_the_reference_list(key, cli, count):
    want = json.loads(str(G[f'cli_flags/{key}']))
    got = [a for a in cli.define_input_args()._actions if a.dest != 'help']
    assert [a.dest for a in got] == [w['dest'] for w in want] and len(want) == count
    for a, w in zip(got, want):
        assert list(a.option_strings) == w['flags'] and a.default == w['default'] and a.nargs == w['nargs'], w['dest']
        assert (None if a.choices is None else list(a.choices)) == w['choices'] and (None if a.type is None else a.type.__name__) == w['type']
        assert a.help == w['help']
    assert cli.define_input_args().description == {'correction': 'Fix incorrect "DelayRecordingTime" in SEG-Y file(s).',
                                                   'padding': 'Pad time delays in SEG-Y file(s) using "DelayRecordingTime".'}[key]


def test_console_scripts_are_registered():
    cfg = open(os.path.join(ROOT, 'setup.cfg')).read()
    assert '03_correct_delrt = pseudo_3d_interpolation_amd.delrt_correction_segy:main' in cfg
    assert '04_pad_delrt = pseudo_3d_interpolation_amd.delrt_padding_segy:main' in cfg


def write(path, section, delrt, **kw):
    ntr = section.shape[1]
    return S.write_segy(str(path), section.T, DT, headers={'DelayRecordingTime': delrt, 'FieldRecord': np.arange(ntr) + 100}, **kw)


def test_output_naming_and_skip_of_a_file_with_one_delay(tmp_path, capsys):
    data = G['section/clean/data']
    src = write(tmp_path / 'line.sgy', data, 10)
    before = open(src, 'rb').read()
    for cli, msg in ((cli3, 'Skipped: Identical "DelayRecordingTime" for whole SEG-Y file'), (cli4, 'Continuous "DelayRecordingTime" for whole SEG-Y file --> skipped!')):
        with pytest.raises(SystemExit):
            cli.main(['x', src, '-V', '1'])
        assert msg in capsys.readouterr().out
        assert os.listdir(tmp_path) == ['line.sgy'] and open(src, 'rb').read() == before
    assert cli3.check_varying_DelayRecordingTimes(src) is False and cli3.check_varying_DelayRecordingTimes(src, byte_delay=9) is True
    args4 = cli4.define_input_args().parse_args([src])
    quiet = lambda *a, **k: None  # noqa: E731
    assert segy_cli.output_target(src, args4, 'pad')[0] == str(tmp_path / 'line_pad.sgy')
    out = tmp_path / 'out'
    out.mkdir()
    assert segy_cli.output_target(src, cli4.define_input_args().parse_args([src, '-o', str(out), '--txt_suffix', 'p']), 'pad')[0] == str(out / 'line_p.sgy')
    with pytest.raises(FileNotFoundError):
        segy_cli.output_target(src, cli4.define_input_args().parse_args([src, '-o', str(tmp_path / 'missing')]), 'pad')
    args3 = cli3.define_input_args().parse_args([src, '-o', str(out)])
    assert segy_cli.copied_target(src, args3, 'delrt', quiet)[0] == str(out / 'line_delrt.sgy') and open(out / 'line_delrt.sgy', 'rb').read() == before
    assert segy_cli.copied_target(src, cli3.define_input_args().parse_args([src, '-i', '-o', str(out)]), 'delrt', quiet)[0] == src
    assert segy_cli.copied_target(src, cli3.define_input_args().parse_args([src, '--txt_suffix', 'fix']), 'delrt', quiet)[0] == str(tmp_path / 'line_fix.sgy')
    with pytest.raises(FileNotFoundError):
        cli3.main(['x', str(tmp_path / 'missing.sgy')])


def test_skip_rules_are_the_reference_inequality():
    ends = G['section/ends/delrt']
    assert D.delay_change_subsets(ends, ends.size, 5) == [(30, 25, 36), (55, 50, 60)]           # 55 = ntr - n_traces passes, one trace short
    assert [i for i, _, _ in D.delay_change_subsets(G['section/end-skipped/delrt'], 60, 5)] == [30]
    assert D.delay_change_subsets(G['section/three-delays/delrt'], 60, 5) == []
    said = []
    D.delay_change_subsets(ends, ends.size, 5, say=lambda *a, **k: said.append((a[0], k['kind'])))
    assert said == [('Not enough neighboring traces for idx: 3 [-2:9] with >60< total traces. Skipped data subset.', 'warning')]


@pytest.mark.parametrize('name', [str(n) for n in G['section/cases']])
def test_full_path_on_the_numpy_restatement(monkeypatch, name):
    """`correct_delay_changes` with the device call replaced: the host side (subsets, filled-up column, decision) against the reference's results."""
    monkeypatch.setattr(_ffi, 'delrt_windows', numpy_windows)
    data, delrt = G[f'section/{name}/data'], G[f'section/{name}/delrt']
    n_traces, n_samples = (int(v) for v in G[f'section/{name}/window'])
    fixes = D.correct_delay_changes(np.ascontiguousarray(data.T), delrt, n_traces, n_samples)
    want = [(int(i), int(i) - n_traces + int(x), int(delrt[int(i) - n_traces + int(x)]), int(d))
            for i, k, d, x in zip(*(G[f'section/{name}/{key}'] for key in ('idx', 'kind', 'delay', 'index'))) if k == 1]
    assert [tuple(int(v) for v in f) for f in fixes] == want


def test_departures_copy_is_corrected_and_the_named_trace_is_written(monkeypatch, tmp_path):
    """The reference leaves a copy untouched (it writes only with --inplace) and writes header[idx]; here the copy carries the correction, at
    the trace the decision names: idx + 1 for the offset trace behind the change."""
    monkeypatch.setattr(_ffi, 'delrt_windows', numpy_windows)
    data, delrt = G['section/offset-after/data'], G['section/offset-after/delrt']
    assert G['section/offset-after/idx'].tolist() == [30] and G['section/offset-after/index'].tolist() == [6] and G['section/offset-after/delay'].tolist() == [10]
    src = write(tmp_path / 'line.sgy', data, delrt)
    keep = str(tmp_path / 'keep.sgy')
    shutil.copy2(src, keep)
    fixes = cli3.wrapper_delrt_correction_segy(src, cli3.define_input_args().parse_args([src]))
    assert [tuple(int(v) for v in f) for f in fixes] == [(30, 31, 30, 10)]
    want = delrt.copy()
    want[31] = 10
    a, b = S.SegyFile(keep), S.SegyFile(str(tmp_path / 'line_delrt.sgy'))
    assert b.header('DelayRecordingTime').tolist() == want.tolist() and b.header('DelayRecordingTime')[30] == 30
    assert open(src, 'rb').read() == open(keep, 'rb').read()                                     # the input is not touched
    assert b.traces().tobytes() == a.traces().tobytes() and open(b.path, 'rb').read()[3200:3600] == open(keep, 'rb').read()[3200:3600]
    for k in S.TRACE_FIELDS:
        if k != 'DelayRecordingTime':
            assert np.array_equal(a.header(k), b.header(k)), k
    assert any(line.rstrip().endswith(': DELRT FIX (BYTE:109)') for line in get_textual_header(b.path).split('\n'))


def test_correction_at_another_header_byte(monkeypatch, tmp_path):
    """--byte_delay names a byte without a field of its own (here 111, a 16-bit word): read and written as big-endian int16."""
    monkeypatch.setattr(_ffi, 'delrt_windows', numpy_windows)
    data, delrt = G['section/early-header/data'], G['section/early-header/delrt']
    src = write(tmp_path / 'line.sgy', data, 0)
    raw = np.memmap(src, np.uint8, 'r+')
    size = 240 + data.shape[0] * 4
    raw[3600:].reshape(-1, size)[:, 110:112] = delrt.astype('>i2').reshape(-1, 1).view(np.uint8)
    raw.flush()
    del raw
    fixes = cli3.wrapper_delrt_correction_segy(src, cli3.define_input_args().parse_args([src, '-i', '--byte_delay', '111']))
    assert [tuple(int(v) for v in f) for f in fixes] == [(30, 30, 30, 10)]
    seg = S.SegyFile(src)
    want = delrt.copy()
    want[30] = 10
    assert S.header_words(seg, 111).tolist() == want.tolist() and set(seg.header('DelayRecordingTime').tolist()) == {0}
    assert seg.traces().tobytes() == np.ascontiguousarray(data.T).tobytes()
