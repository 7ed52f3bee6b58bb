"""Step 5 end to end: ``05_correct_static`` on SEG-Y files written from the fixture sections (tests/golden/static.npz): samples against the
NumPy shift of the fixture's static_samples, header words 103 / 233 / 237, the ``.sta`` file, the textual header, the kinds of input and output."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import static_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import static_correction_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions.header import get_textual_header  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'static.npz'))
DT, DELAY = 0.25, 40


def flags(name):
    p = json.loads(str(G[f'case/{name}/params']))
    d, s = p['detect'], p['static']
    out = ['--win_samples', str(d['win']), '--win_median', str(d['win_median']), '--n_amp_samples', str(d['n']), '--win_sg', str(s['win_sg']),
           '--limit_shift', str(s['limit_samples']), '--limit_depressions', *[str(v) for v in s['limit_depressions']]]
    for key in ('nsta', 'nlta'):
        if d[key] is not None:
            out += [f'--{key}', str(d[key])]
    if s['win_mad'] is not None:
        out += ['--win_mad', str(s['win_mad'])]
    return p['section'], out


def write(path, section, fmt=5, **kw):
    ntr = section.shape[1]
    return S.write_segy(str(path), section.T, DT, fmt=fmt, headers={'DelayRecordingTime': DELAY, 'FieldRecord': np.arange(ntr) + 100}, **kw)


def check(src, dst, name, seafloor=False, start=None):
    a, b = S.SegyFile(src), S.SegyFile(dst)
    samples, idx = G[f'case/{name}/static_samples'], G[f'case/{name}/idx_amp']
    want = H.compensate_static(a.traces().T, samples).T
    assert np.count_nonzero(samples) > 10 and b.traces().tobytes() == want.tobytes() and a.format == b.format
    assert np.array_equal(b.header('TotalStaticApplied'), (samples * DT * 1000).astype('int32')) and set(b.header('UnassignedInt1').tolist()) == {-1000}
    twt = DELAY + np.arange(a.ns) * DT
    twt_seafloor = twt[idx + (0 if start is None else start)]
    assert np.array_equal(b.header('UnassignedInt2'), (twt_seafloor * 1000).astype('int32') if seafloor else np.zeros(a.ntraces, int))
    for k in ('TRACE_SEQUENCE_LINE', 'FieldRecord', 'DelayRecordingTime', 'TRACE_SAMPLE_COUNT', 'TRACE_SAMPLE_INTERVAL'):
        assert np.array_equal(a.header(k), b.header(k))
    assert open(src, 'rb').read()[3200:3600] == open(dst, 'rb').read()[3200:3600]
    lines = [line.rstrip() for line in get_textual_header(dst).split('\n')]
    assert any(line.endswith(': STATIC CORRECTION:amp (byte:103) with SCALAR (byte:233)') for line in lines)
    assert any(line.endswith(': -> SEAFLOOR (byte:237) with SCALAR (byte:233)') for line in lines) == seafloor
    return samples, twt_seafloor


@pytest.mark.parametrize('name,fmt', [('A', 5), ('A', 1), ('B-mid', 5)])
def test_single_file_with_aux_and_seafloor(tmp_path, name, fmt):
    sec, argv = flags(name)
    src = write(tmp_path / 'line.sgy', G['section/' + sec], fmt=fmt)
    out = tmp_path / 'out'
    out.mkdir()
    with pytest.raises(SystemExit):
        cli.main(['05_correct_static', src, '-o', str(out), '--write_aux', '--write_seafloor2trace', *argv])
    assert sorted(os.listdir(out)) == ['line_static.sgy', 'line_static.sta'] and sorted(os.listdir(tmp_path)) == ['line.sgy', 'out']
    samples, twt_seafloor = check(src, str(out / 'line_static.sgy'), name, seafloor=True)
    rows = open(out / 'line_static.sta').read().split('\n')
    assert rows[0] == 'tracl,tracr,fldr,static_samples,static_ms,seafloor_ms' and rows[-1] == '' and len(rows) == samples.size + 2
    assert rows[1:-1] == [f'{k + 1},{k + 1},{k + 100},{samples[k]:d},{samples[k] * DT:.3f},{twt_seafloor[k]:.2f}' for k in range(samples.size)]


def test_inplace_list_and_directory(tmp_path):
    sec, argv = flags('A')
    d = tmp_path / 'lines'
    d.mkdir()
    one, two, three = (write(d / f'l{k}.sgy', G['section/A']) for k in range(3))
    keep = str(tmp_path / 'original.sgy')
    shutil.copy2(one, keep)
    with pytest.raises(SystemExit):
        cli.main(['05_correct_static', one, '--inplace', '--use_delay', *argv])       # one delay time: --use_delay changes nothing
    check(keep, one, 'A')
    assert sorted(os.listdir(d)) == ['l0.sgy', 'l1.sgy', 'l2.sgy']
    (d / 'list.txt').write_text('l1.sgy\n')
    out = tmp_path / 'out'
    out.mkdir()
    cli.main(['05_correct_static', str(d / 'list.txt'), '-o', str(out), '--txt_suffix', 'st', *argv])
    check(two, str(out / 'l1_st.sgy'), 'A')
    logs = [n for n in os.listdir(d) if n.endswith('.log')]
    assert len(logs) == 1 and 'static_correction_segy' in logs[0] and '\x1b' not in open(d / logs[0]).read()
    os.remove(d / logs[0])
    os.remove(d / 'list.txt')
    shutil.copy2(keep, one)
    cli.main(['05_correct_static', str(d), '-o', str(out), '-V', '1', *argv])
    assert sorted(n for n in os.listdir(out) if n.endswith('.sgy')) == ['l0_static.sgy', 'l1_st.sgy', 'l1_static.sgy', 'l2_static.sgy']
    for src in (one, two, three):
        check(src, str(out / os.path.basename(src).replace('.sgy', '_static.sgy')), 'A')
    log = open(d / [n for n in os.listdir(d) if n.endswith('.log')][0]).read()
    assert 'Processing total of < 3 > files' in log and 'Failed' not in log


def test_zero_filled_traces_by_original_sample_count(tmp_path):
    start, extra = G['pad/start'], int(G['pad/extra'])
    data = G['section/A']
    padded = np.zeros((data.shape[0] + extra, data.shape[1]), np.float32)
    for k, s in enumerate(start):
        padded[s:s + data.shape[0], k] = data[:, k]
    assert 'pad' not in str(tmp_path)
    src = write(tmp_path / 'line.sgy', padded, binary={'SamplesOriginal': data.shape[0]})
    _, argv = flags('A-pad')
    with pytest.raises(SystemExit):
        cli.main(['05_correct_static', src, '-o', str(tmp_path), '--write_seafloor2trace', *argv])
    check(src, str(tmp_path / 'line_static.sgy'), 'A-pad', seafloor=True, start=start)


def test_water_depth_mode(tmp_path):
    c = {k: G[f'case/A/{k}'] for k in ('gs_in', 'static_samples')}
    p = json.loads(str(G['case/A/params']))['static']
    depth_cm = c['gs_in'] * 25                                                         # 0.25 m per sample index, stored in cm
    src = S.write_segy(str(tmp_path / 'line.sgy'), G['section/A'].T, DT, headers={'SourceWaterDepth': depth_cm, 'ElevationScalar': -100})
    with pytest.raises(SystemExit):
        cli.main(['05_correct_static', src, '-o', str(tmp_path), '-m', 'swdep', '--write_aux', '--limit_shift', '4', '--limit_depressions', '10', '6', '2'])
    from pseudo_3d_interpolation_amd.functions import static as st
    depth = depth_cm / 100
    static = st.get_static(depth, **dict(p, limit_samples=4))
    samples = np.around(st.depth2samples(static, dt=DT / 1000), 0).astype(np.int32)
    b = S.SegyFile(str(tmp_path / 'line_static.sgy'))
    assert np.count_nonzero(samples) > 10 and b.traces().tobytes() == H.compensate_static(G['section/A'], samples).T.tobytes()
    assert np.array_equal(b.header('TotalStaticApplied'), (samples * DT * 1000).astype('int32'))
    rows = open(tmp_path / 'line_static.sta').read().split('\n')
    assert rows[0].endswith(',swdep_m') and rows[1] == f'1,1,0,{samples[0]:d},{samples[0] * DT:.3f},{depth[0]:.2f}'
    assert any(line.rstrip().endswith('STATIC CORRECTION:swdep (byte:103) with SCALAR (byte:233)') for line in get_textual_header(b.path).split('\n'))
