"""Step 8 end to end: ``08_despike`` on synthetic SEG-Y profiles (the survey of the step-10 test plus noise and planted bursts, IEEE and IBM
files, delay times that change along the lines), samples against the NumPy restatement, headers byte for byte, and step 10 on the result."""
import os
import shutil
import sys

import numpy as np
import pytest

from test_gpu_binning_cli import configs, write_survey

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import despike_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import cube_binning_3D as cb  # noqa: E402
from pseudo_3d_interpolation_amd import despiking_2D_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions.header import get_textual_header  # noqa: E402

pytestmark = pytest.mark.gpu
FLAGS = ['-wti', '20', '-wtr', '5', '-t', '6', '-m', 'median', '-oa', 'median']
KW = dict(window=20, dt=0.5, overlap=10, ntraces=5, mode='median', threshold=6.0, out='median')
TRACE_BYTES = 240 + 120 * 4


def noisy_survey(tmp_path):
    d, corners = write_survey(tmp_path)
    rng = np.random.default_rng(11)
    for k, name in enumerate(sorted(os.listdir(d))):
        path = str(d / name)
        x = S.SegyFile(path).traces() + 0.05 * rng.standard_normal((S.SegyFile(path).ntraces, 120)).astype(np.float32)
        for trace, r0 in ((0, 10), (17, 30), (39, 60), (40, 64), (100 + k, 80), (x.shape[0] - 1, 20)):
            x[trace, r0:r0 + 16] = (3.0 * (1 + 0.1 * rng.random(16)) * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
        S.update_samples(path, x)
    return d, corners


def check_file(src, dst, use_delay):
    a, b = S.SegyFile(src), S.SegyFile(dst)
    delrt = a.header('DelayRecordingTime')
    splits = np.nonzero(delrt[1:] != delrt[:-1])[0] + 1 if use_delay else None
    want, spikes = H.despike_2D(a.traces().T, splits=splits, return_spikes=True, **KW)
    assert len(spikes) >= 5 and {0, a.ntraces - 1} <= {x for x, *_ in spikes}
    if use_delay:
        assert len(splits) >= 2 and len(set(delrt.tolist())) >= 2
    want = want.T
    if a.format == 1:
        want = S.ibm2ieee(S.ieee2ibm(want))
    assert b.traces().tobytes() == want.tobytes()
    raw_a, raw_b = open(src, 'rb').read(), open(dst, 'rb').read()
    assert len(raw_a) == len(raw_b) and raw_a[3200:3600] == raw_b[3200:3600]
    assert all(raw_a[3600 + k * TRACE_BYTES:3840 + k * TRACE_BYTES] == raw_b[3600 + k * TRACE_BYTES:3840 + k * TRACE_BYTES] for k in range(a.ntraces))
    lines = get_textual_header(dst).split('\n')
    assert lines[0].startswith(get_textual_header(src).split('\n')[0].rstrip()) and any(line.rstrip().endswith(': DESPIKE') for line in lines)


def test_directory_with_delay_splits_then_step_10(tmp_path):
    d, corners = noisy_survey(tmp_path)
    out = tmp_path / 'despiked'
    out.mkdir()
    cli.main(['08_despike', str(d), '--use_delay', '-o', str(out), '-V', '1'] + FLAGS)
    names = sorted(n for n in os.listdir(d) if n.endswith('.sgy'))
    assert sorted(os.listdir(out)) == sorted([n.replace('.sgy', '_despk.sgy') for n in names] + [n for n in os.listdir(out) if n.endswith('.yml')])
    assert len([n for n in os.listdir(out) if n.endswith('argparse_parameter.yml')]) == 1
    logs = [n for n in os.listdir(d) if n.endswith('.log')]
    assert len(logs) == 1 and '\x1b' not in open(d / logs[0]).read() and 'Processing total of < 7 > files' in open(d / logs[0]).read()
    assert any(S.SegyFile(str(d / n)).format == 1 for n in names)
    for n in names:
        check_file(str(d / n), str(out / n.replace('.sgy', '_despk.sgy')), use_delay=True)
    for n in os.listdir(out):
        if n.endswith('.yml'):
            os.remove(out / n)
    argv = [*configs(tmp_path, corners, 'average'), '--file_type', 'npz']
    _, clean = cb.main(['10', str(out), *argv, '--path_coords', str(out), '--output_dir', str(tmp_path / 'cube_clean')], return_dataset=True)
    for n in logs:
        os.remove(d / n)
    _, raw = cb.main(['10', str(d), *argv, '--path_coords', str(d), '--output_dir', str(tmp_path / 'cube_raw')], return_dataset=True)
    amp, amp_raw = clean.data_vars['amp'], raw.data_vars['amp']
    # step 10 takes the despiked files as they are: same geometry and fold as from the raw files, other amplitudes where a burst was stacked
    # (the burst of trace 17 lies at 55 ... 83 ms in every file, inside the cube's 50 ... 90 ms)
    np.testing.assert_array_equal(clean.data_vars['fold'], raw.data_vars['fold'])
    assert clean.data_vars['fold'].max() > 1 and amp.shape == amp_raw.shape and np.isfinite(amp).all() and np.abs(amp).max() > 0.5
    assert (amp != amp_raw).any()


def test_single_file_inplace_and_list(tmp_path):
    d, _ = noisy_survey(tmp_path)
    first, second, third = [str(d / n) for n in sorted(os.listdir(d))[:3]]
    with pytest.raises(SystemExit):
        cli.main(['08_despike', first] + FLAGS)                         # a copy next to the input
    check_file(first, first.replace('.sgy', '_despk.sgy'), use_delay=False)
    keep = str(tmp_path / 'original.sgy')
    shutil.copy2(second, keep)
    with pytest.raises(SystemExit):
        cli.main(['08_despike', second, '--inplace', '--use_delay', '--byte_delay', '109'] + FLAGS)
    check_file(keep, second, use_delay=True)
    (d / 'list.txt').write_text(os.path.basename(third) + '\n')
    cli.main(['08_despike', str(d / 'list.txt'), '--txt_suffix', 'clean'] + FLAGS)
    check_file(third, third.replace('.sgy', '_clean.sgy'), use_delay=False)


def test_nothing_removed_deletes_the_copy(tmp_path):
    rng = np.random.default_rng(3)
    p = S.write_segy(str(tmp_path / 'quiet.sgy'), rng.standard_normal((60, 120)).astype(np.float32), 0.5)
    before = open(p, 'rb').read()
    with pytest.raises(SystemExit):
        cli.main(['08_despike', p, '-wti', '20', '-wtr', '5', '-t', '50', '-m', 'mean'])
    assert os.listdir(tmp_path) == ['quiet.sgy'] and open(p, 'rb').read() == before
