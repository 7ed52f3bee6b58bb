"""Step 6 end to end on the GPU: ``06_compensate_tide`` on a synthetic profile of 40 traces x 200 samples at 50 microseconds whose positions are
thousandths of arc-seconds across the 0 / 360 degree seam, with the synthetic model of tests/helpers/tide_numpy.py written into ``tmp_path``.  The
samples must EQUAL the input shifted by the exact offsets of the mpmath fixture (tests/golden/tide.npz holds no offset within 1e-4 samples of a
rounding tie); the last four traces repeat the positions of traces 5 ... 8 at later times and get the tide of the FIRST trace at their position."""
import datetime
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import tide_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import tide_compensation_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions.header import get_textual_header  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'tide.npz'))
NTR, NS = 40, 200
OFFSET, TIDE = G['cli/offset'], G['cli/tide']


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('model'))
    H.make_model(folder, constituents=H.CONSTITUENTS[:8])
    return folder


def write(path, fmt=5, **changed):
    data = np.random.default_rng(6).integers(-2000, 2000, (NTR, NS)).astype(np.float32)
    headers = {'SourceX': G['cli/lon_mas'], 'SourceY': G['cli/lat_mas'], 'CoordinateUnits': 2, 'SourceGroupScalar': 1, 'FieldRecord': np.arange(NTR) + 100,
               'YearDataRecorded': G['cli/year'], 'DayOfYear': G['cli/day'], 'HourOfDay': G['cli/hour'], 'MinuteOfHour': G['cli/minute'],
               'SecondOfMinute': G['cli/second'], 'DelayRecordingTime': 10}
    headers.update(changed)
    return S.write_segy(str(path), data, 0.05, fmt=fmt, headers=headers, text='C 1 CLIENT'.ljust(80) + 'C 2 LINE'.ljust(80))


def check(src_bytes, dst):
    """Samples shifted by the fixture's offsets, every header byte the input's, the dated line in the textual header."""
    size = 240 + NS * 4
    fmt = int(np.frombuffer(src_bytes[3224:3226], '>i2')[0])
    b = open(dst, 'rb').read()
    assert len(src_bytes) == len(b) and src_bytes[3200:3600] == b[3200:3600]
    ta, tb = (np.frombuffer(v[3600:], np.uint8).reshape(NTR, size) for v in (src_bytes, b))
    assert np.array_equal(ta[:, :240], tb[:, :240])
    words = '>u4' if fmt == 1 else '>f4'
    before, after = (np.ascontiguousarray(v[:, 240:]).view(words).reshape(NTR, NS) for v in (ta, tb))
    assert np.array_equal(after.T, H.shift_section(before.T, OFFSET))             # whole words moved, zeros (all bits 0 in both formats) filled in
    assert len(set(OFFSET.tolist())) > 5 and OFFSET.min() < 0 < OFFSET.max()
    lines = [line[3:].rstrip() for line in get_textual_header(dst).split('\n')]
    assert f' {datetime.date.today().isoformat()}: TIDE COMPENSATION' in lines and lines[0] == ' CLIENT'


@pytest.mark.parametrize('fmt', [5, 1])
def test_samples_equal_the_shift_by_the_exact_offsets(tmp_path, model, fmt):
    src = write(tmp_path / 'line.sgy', fmt)
    before = open(src, 'rb').read()
    with pytest.raises(SystemExit):
        cli.main(['06_compensate_tide', src, model, '--write_aux'])
    assert sorted(os.listdir(tmp_path)) == ['line.sgy', 'line_tide.sgy', 'line_tide.tid'] and open(src, 'rb').read() == before
    check(before, str(tmp_path / 'line_tide.sgy'))
    text = open(tmp_path / 'line_tide.tid').read().split('\n')
    assert text[0] == 'tracl,tracr,fldr,time,tide_m,tide_ms,tide_samples' and text[-1] == '' and len(text) == NTR + 2
    for k, line in enumerate(text[1:-1]):
        tracl, tracr, fldr, time, tide_m, tide_ms, samples = line.split(',')
        assert (int(tracl), int(tracr), int(fldr), time) == (k + 1, k + 1, 100 + k, str(G['cli/time_used'][k]))
        assert abs(float(tide_m) - TIDE[k]) <= 5.1e-7 and abs(float(tide_ms) - TIDE[k] / 0.75) <= 5.1e-4 and int(samples) == OFFSET[k], line
        assert len(tide_m.split('.')[1]) == 6 and len(tide_ms.split('.')[1]) == 3 and '.' not in samples


def test_traces_at_one_position_get_the_tide_of_the_first(tmp_path, model):
    src = write(tmp_path / 'line.sgy')
    assert np.array_equal(G['cli/lon_mas'][36:], G['cli/lon_mas'][5:9]) and not np.array_equal(G['cli/second'][36:], G['cli/second'][5:9])
    with pytest.raises(SystemExit):
        cli.main(['06_compensate_tide', src, model, '--write_aux', '--txt_suffix', 'tc', '-V', '2'])
    assert sorted(os.listdir(tmp_path)) == ['line.sgy', 'line_tc.sgy', 'line_tc.tid']
    assert np.array_equal(OFFSET[36:], OFFSET[5:9])
    before, after = S.SegyFile(src).traces(), S.SegyFile(str(tmp_path / 'line_tc.sgy')).traces()
    assert np.array_equal(after[36:].T, H.shift_section(before[36:].T, OFFSET[5:9]))
    rows = open(tmp_path / 'line_tc.tid').read().split('\n')[1:-1]
    assert [r.split(',')[3:] for r in rows[36:]] == [r.split(',')[3:] for r in rows[5:9]]     # the time and the tide of the first trace there


def test_inplace_supersedes_the_output_directory(tmp_path, model):
    src = write(tmp_path / 'line.sgy')
    before = open(src, 'rb').read()
    other = tmp_path / 'out'
    other.mkdir()
    with pytest.raises(SystemExit):
        cli.main(['06_compensate_tide', src, model, '--inplace', '-o', str(other), '--write_aux'])
    assert sorted(os.listdir(tmp_path)) == ['line.sgy', 'line.tid', 'out'] and os.listdir(other) == []
    check(before, src)


def test_list_of_two_files_into_an_output_directory(tmp_path, model):
    d, out = tmp_path / 'lines', tmp_path / 'out'
    d.mkdir()
    out.mkdir()
    one, two = write(d / 'a.sgy'), write(d / 'b.sgy')
    (d / 'list.txt').write_text('a.sgy\nb.sgy\n')
    cli.main(['06_compensate_tide', str(d / 'list.txt'), model, '-o', str(out), '-V', '1'])
    assert sorted(os.listdir(out)) == ['a_tide.sgy', 'b_tide.sgy']
    for src in (one, two):
        check(open(src, 'rb').read(), str(out / os.path.basename(src).replace('.sgy', '_tide.sgy')))
    logs = [n for n in os.listdir(d) if n.endswith('.log')]
    log = open(d / logs[0]).read()
    assert len(logs) == 1 and logs[0].endswith('_tide_compensation_segy.log') and '\x1b' not in log
    assert 'Processing total of < 2 > files' in log and 'Processing file < b.sgy >' in log and 'Forced source CRS to be geographic' in log


def test_a_trace_on_land_or_without_a_time_raises_and_leaves_no_copy(tmp_path, model):
    lon, lat = G['cli/lon_mas'].copy(), G['cli/lat_mas'].copy()
    lon[[3, 17]], lat[[3, 17]] = 10 * 3600000 + 1234, 70 * 3600000 + 4321           # inside the dry block of the model (5 ... 15 E, 65 ... 75 N)
    src = write(tmp_path / 'land.sgy', SourceX=lon, SourceY=lat)
    with pytest.raises(ValueError, match='land.sgy: 2 of 40 traces'):
        cli.main(['06_compensate_tide', src, model])
    day = G['cli/day'].copy()
    day[7] = 0
    src2 = write(tmp_path / 'notime.sgy', DayOfYear=day)
    with pytest.raises(ValueError, match='trace #7 .*day of year 0'):
        cli.main(['06_compensate_tide', src2, model])
    assert sorted(os.listdir(tmp_path)) == ['land.sgy', 'notime.sgy']
