"""Step 2 end to end on the GPU: ``02_reproject_segy`` on a synthetic profile of 300 traces x 16 samples whose source coordinates are thousandths
of arc-seconds (tests/golden/reproject.npz, make_golden_reproject.py).  The header integers must EQUAL the exact ones of the mpmath oracle for
every scalar (the fixture holds no value within 1e-6 m of a rounding tie), samples and every other header byte must be the input's; one run with
``--smooth`` and one over a ``.txt`` list of two files."""
import datetime
import os

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import reproject_segy as cli
from pseudo_3d_interpolation_amd.functions import segy as S
from pseudo_3d_interpolation_amd.functions.header import get_textual_header

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'reproject.npz'))
NTR, NS = 300, 16
COMMON = ['--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760']
CHANGED = ['SourceX', 'SourceY', 'CoordinateUnits', 'SourceGroupScalar']


def write(path):
    data = np.random.default_rng(5).standard_normal((NTR, NS)).astype(np.float32)
    headers = {'SourceX': G['hdr/lon_mas'], 'SourceY': G['hdr/lat_mas'], 'CoordinateUnits': 2, 'SourceGroupScalar': 1, 'FieldRecord': np.arange(NTR) + 100,
               'CDP_X': np.arange(NTR) * 3, 'GroupY': 7 - np.arange(NTR), 'DelayRecordingTime': 10}
    return S.write_segy(str(path), data, 0.25, headers=headers, text='C 1 CLIENT'.ljust(80) + 'C 2 LINE'.ljust(80))


def check(src, dst, x, y, scalar, smoothed=False):
    out = S.SegyFile(dst)
    assert np.array_equal(out.header('SourceX'), x) and np.array_equal(out.header('SourceY'), y)
    assert set(out.header('CoordinateUnits').tolist()) == {1} and set(out.header('SourceGroupScalar').tolist()) == {scalar}
    a, b = open(src, 'rb').read(), open(dst, 'rb').read()
    assert len(a) == len(b) and a[3200:3600] == b[3200:3600]
    size = 240 + NS * 4
    ta, tb = (np.frombuffer(v[3600:], np.uint8).reshape(NTR, size).copy() for v in (a, b))
    for name in CHANGED:
        byte, dt = S.TRACE_FIELDS[name]
        ta[:, byte - 1:byte - 1 + np.dtype(dt).itemsize] = tb[:, byte - 1:byte - 1 + np.dtype(dt).itemsize] = 0
    assert np.array_equal(ta, tb)                                   # samples and all other header bytes
    lines = [line[3:].rstrip() for line in get_textual_header(dst).split('\n')]
    assert ' CRS (PROJECTED): EPSG:32760' in lines and lines[0] == ' CLIENT'
    assert f' {datetime.date.today().isoformat()}: REPROJECT (BYTES:73 77)' + (' SMOOTHED' if smoothed else '') in lines


@pytest.mark.parametrize('scalar', G['hdr/scalars'].tolist())
def test_header_integers_equal_the_oracle(tmp_path, scalar):
    src = write(tmp_path / 'line.sgy')
    before = open(src, 'rb').read()
    with pytest.raises(SystemExit):
        cli.main(['02_reproject_segy', src, *COMMON, '--scalar_coords', str(scalar)])
    assert sorted(os.listdir(tmp_path)) == ['line.sgy', 'line_reproj.sgy'] and open(src, 'rb').read() == before
    check(src, str(tmp_path / 'line_reproj.sgy'), G[f'hdr/{scalar}/x'], G[f'hdr/{scalar}/y'], scalar)


def test_smooth_run(tmp_path):
    src = write(tmp_path / 'line.sgy')
    with pytest.raises(SystemExit):
        cli.main(['02_reproject_segy', src, *COMMON, '--smooth', '--txt_suffix', 'sm'])
    check(src, str(tmp_path / 'line_sm.sgy'), G['hdr/smooth11/x'], G['hdr/smooth11/y'], -100, smoothed=True)


def test_list_of_two_files(tmp_path):
    d = tmp_path / 'lines'
    d.mkdir()
    one, two = write(d / 'a.sgy'), write(d / 'b.sgy')
    out = tmp_path / 'out'
    out.mkdir()
    (d / 'list.txt').write_text('a.sgy\nb.sgy\n')
    cli.main(['02_reproject_segy', str(d / 'list.txt'), *COMMON, '-o', str(out), '-sc', '-1000', '-V', '1'])
    assert sorted(os.listdir(out)) == ['a_reproj.sgy', 'b_reproj.sgy']
    for src in (one, two):
        check(src, str(out / os.path.basename(src).replace('.sgy', '_reproj.sgy')), G['hdr/-1000/x'], G['hdr/-1000/y'], -1000)
    logs = [n for n in os.listdir(d) if n.endswith('.log')]
    log = open(d / logs[0]).read()
    assert len(logs) == 1 and logs[0].endswith('_reproject_segy.log') and '\x1b' not in log
    assert 'Processing total of < 2 > files' in log and 'Processing file < b.sgy >' in log
