"""Step 10 end to end: synthetic SEG-Y profiles (crossing lines over a rotated grid, a dipping and a flat reflector, delay times that
vary per file and along the lines) written with functions/segy.py, binned by ``cube_binning_3D.main``, checked bin by bin against the
padded traces, and the ``_twt-il-xl`` cube fed unchanged to steps 12 and 13."""
import os

import numpy as np
import pytest
import yaml

from helpers.binning_numpy import padded
from pseudo_3d_interpolation_amd import cube_apply_FFT, cube_binning_3D as cb, cube_POCS_interpolation_3D as step13
from pseudo_3d_interpolation_amd.cube_io import open_cube
from pseudo_3d_interpolation_amd.functions import binning as B
from pseudo_3d_interpolation_amd.functions import segy as S
from pseudo_3d_interpolation_amd.functions.backends import h5py_enabled
from pseudo_3d_interpolation_amd.functions.transform import Affine

pytestmark = pytest.mark.gpu
ANGLE, CENTRE, DT, NS = 30.0, np.array([5000.0, 8000.0]), 0.5, 120
WKT = 'PROJCRS["WGS 84 / UTM zone 60S",ID["EPSG",32760]]'


def model(x, y, t):
    """Ricker pulses on a reflector dipping along the rotated x axis and on a flat one."""
    u = (x - CENTRE[0]) * np.cos(np.deg2rad(ANGLE)) + (y - CENTRE[1]) * np.sin(np.deg2rad(ANGLE))
    out = np.zeros(np.broadcast(x, t).shape)
    for tr, amp in ((65.0 + 0.03 * u, 1.0), (80.0 + 0 * u, -0.6)):
        a = (np.pi * 60.0 * (t - tr) / 1000.0) ** 2
        out += amp * (1 - 2 * a) * np.exp(-a)
    return out


def write_survey(tmp_path):
    rng = np.random.default_rng(7)
    d = tmp_path / 'segy'
    d.mkdir()
    rot = Affine().rotate_around(ANGLE, tuple(CENTRE))
    nav = []
    for k in range(7):
        phi = np.deg2rad(ANGLE + [0, 90, 45, -30, 10, 100, 60][k])
        off = rng.uniform(-120, 120)
        s = np.arange(-240, 240, 2.7)
        p = np.column_stack((s * np.cos(phi) - off * np.sin(phi), s * np.sin(phi) + off * np.cos(phi))) + CENTRE
        xy = np.round(p * 100) / 100
        delay = (40 + 3 * k + (np.arange(len(s)) // 40) * 2).astype(np.int64)
        t = delay[:, None] + DT * np.arange(NS)[None, :]
        data = model(xy[:, :1], xy[:, 1:], t).astype(np.float32)
        hdr = dict(SourceX=np.round(xy[:, 0] * 100), SourceY=np.round(xy[:, 1] * 100), SourceGroupScalar=-100, DelayRecordingTime=delay,
                   FieldRecord=np.arange(len(s)) + 1)
        S.write_segy(str(d / f'line_{k:02d}_UTM60S.sgy'), data, DT, fmt=1 if k == 3 else 5, headers=hdr, text=f'C 1 line {k}')
        nav.append(xy)
    half = 160.0
    corners = rot.transform(np.array([[-half, -half], [-half, half], [half, half], [half, -half]]) + CENTRE)
    return d, corners


def configs(tmp_path, corners, method):
    (tmp_path / 'netcdf.yml').write_text(yaml.safe_dump({'attrs_time': {
        'cube': {'history': 'segy;', 'text': 'TOPAS'}, 'amp': {'units': '-'}, 'env': {'units': '-'}, 'fold': {'long_name': 'fold'},
        'twt': {'units': 'ms'}, 'iline': {'long_name': 'inline'}, 'xline': {'long_name': 'crossline'}, 'x': {'units': 'm'}}}))
    (tmp_path / 'crs.yml').write_text(yaml.safe_dump(WKT))
    (tmp_path / 'cube').mkdir(exist_ok=True)
    (tmp_path / 'cube' / 'setup.yml').write_text(yaml.safe_dump(dict(
        extent_cube={k: [float(v) for v in c] for k, c in zip(('ll', 'ul', 'ur', 'lr'), corners)}, rotation_angle=ANGLE,
        rotation_center=[float(v) for v in CENTRE], bin_size=10, twt_limits=[50, 90], stacking_method=method, factor_dist=1.0,
        name='synth', long_name='synthetic cube', spatial_ref=WKT)))
    return ['--params_netcdf', str(tmp_path / 'netcdf.yml'), '--params_spatial_ref', str(tmp_path / 'crs.yml'), '--params_cube_setup',
            str(tmp_path / 'cube' / 'setup.yml')]


def expected(d, corners, method):
    files = sorted(os.path.join(d, f) for f in os.listdir(d))
    segys = [S.SegyFile(f) for f in files]
    x, y = S.scaled_coordinates(np.concatenate([s.header('SourceGroupScalar') for s in segys]),
                                np.concatenate([s.header('SourceX') for s in segys]), np.concatenate([s.header('SourceY') for s in segys]))
    delays = np.concatenate([s.header('DelayRecordingTime') for s in segys]).astype(float)
    data = np.concatenate([s.traces() for s in segys])
    fwd = Affine().rotate_around(-ANGLE, tuple(CENTRE))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bins, ilxl = B.get_cube_parameter(fwd, fwd.inverse(), np.column_stack((x, y)), (10, 10), corners)
    il, xl = np.unique(bins['il']), np.unique(bins['xl'])
    twt = B.twt_axis(50, 90, DT)
    sh = B.trace_shifts(delays, twt[0], DT)
    cube = np.zeros((twt.size, il.size, xl.size), np.float32)
    fold = np.zeros((il.size, xl.size), np.int64)
    cx, cy = bins['x'].reshape(il.size, xl.size), bins['y'].reshape(il.size, xl.size)
    for i, a in enumerate(il):
        for j, b in enumerate(xl):
            idx = np.flatnonzero((ilxl[:, 0] == a) & (ilxl[:, 1] == b))
            fold[i, j] = idx.size
            if not idx.size:
                continue
            stk = np.stack([padded(data[t], 0, NS, sh[t], twt.size) for t in idx])
            if method == 'average':
                cube[:, i, j] = stk.astype(np.float64).mean(0)
            else:
                dist = np.hypot(x[idx] - cx[i, j], y[idx] - cy[i, j])
                cube[:, i, j] = stk[np.argmin(dist)]
    return cube, fold, twt, il, xl


@pytest.mark.parametrize('method', ['average', 'nearest'])
def test_cli_synthetic_survey(tmp_path, method):
    d, corners = write_survey(tmp_path)
    out = tmp_path / 'out'
    cube, cube_twt = cb.main(['10', str(d), *configs(tmp_path, corners, method), '--path_coords', str(d), '--output_dir', str(out),
                              '--file_type', 'npz', '--write_aux'], return_dataset=True)
    base = f'synth_{method}_10x10m_0+5ms'
    assert sorted(p for p in os.listdir(out) if p.endswith('.npz')) == [f'{base}.npz', f'{base}_twt-il-xl.npz']
    assert os.path.exists(out / f'aux_synth_{method}_10x10m_bins.txt') and os.path.exists(out / f'aux_synth_{method}_10x10m_extent_corner_points.txt')
    want, fold, twt, il, xl = expected(d, corners, method)
    c = open_cube(str(out / f'{base}_twt-il-xl.npz'))
    assert list(c.data_vars) == ['amp', 'fold', 'x', 'y']
    assert c.dims['amp'] == ('twt', 'iline', 'xline') and c.data_vars['amp'].shape == (twt.size, 32, 32)
    np.testing.assert_array_equal(c.coords['twt'], twt)
    np.testing.assert_array_equal(c.coords['iline'], il)
    np.testing.assert_array_equal(c.data_vars['fold'], np.minimum(fold, 255).astype(np.uint8))
    assert c.data_vars['fold'].dtype == np.uint8 and 5 < fold.astype(bool).mean() * 100 < 60 and fold.max() > 1
    got = c.data_vars['amp']
    if method == 'nearest':
        np.testing.assert_array_equal(got, want)
    else:
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    t = open_cube(str(out / f'{base}.npz'))
    assert t.dims['amp'] == ('iline', 'xline', 'twt')
    np.testing.assert_array_equal(t.data_vars['amp'], np.transpose(got, (1, 2, 0)))
    assert c.var_attrs['fold']['coverage_perc'] == round(np.count_nonzero(fold) / fold.size * 100, 2)
    assert c.attrs['history'] == 'segy;cube_binning_3D: create sparse 3D volume;'
    assert c.attrs['text'].startswith('TOPAS\n=== 3D PROCESSING ===\n') and c.attrs['text'].endswith(f'3D BINNING {method} ILINE:10 XLINE:10 UNIT:METER')
    assert c.attrs['epsg'] == 32760 and c.attrs['long_name'] == 'synthetic cube' and c.attrs['stacking_method'] == method
    assert c.coord_attrs['twt'] == {'units': 'ms', 'dt': 0.5} and c.coord_attrs['iline']['bin_il'] == 10
    # the dipping reflector: the covered traces peak near 65 + 0.03 u ms
    assert np.abs(got).max() > 0.5


def test_steps_12_and_13_on_binned_cube(tmp_path):
    d, corners = write_survey(tmp_path)
    cb.main(['10', str(d), *configs(tmp_path, corners, 'average'), '--path_coords', str(d), '--file_type', 'npz',
             '--attribute', 'env'])
    path = str(d / 'synth_average_env_10x10m_0+5ms_twt-il-xl.npz')
    c = open_cube(path)
    assert 'env' in c.data_vars and list(c.data_vars)[0] == 'env'
    nc = tmp_path / 'params12.yml'
    nc.write_text(yaml.safe_dump({'attrs_freq': {'data': {'units': 'amplitude'}, 'new_dim': {'units': 'kHz'}}}))
    cube_apply_FFT.main(['12', path, '--params_netcdf', str(nc), '--compute_real'])
    freq = [p for p in os.listdir(d) if 'freq' in p and p.endswith('.npz')]
    assert len(freq) == 1
    f = open_cube(str(d / freq[0]))
    assert np.all(np.isfinite(f.data_vars[[v for v in f.data_vars if v != 'fold'][0]]))
    metadata = dict(transform_kind='wavelet', wavelet='db4', niter=4, eps=0, thresh_op='soft', thresh_model='linear', decay_kind='values',
                    p_max=0.9, p_min=0.05, alpha=1.0, sqrt_decay=False, version='regular', verbose=False)
    pocs = tmp_path / 'pocs.yml'
    pocs.write_text(yaml.safe_dump({'dim': 'twt', 'var': 'env', 'batch_chunk': 40, 'n_workers': 1, 'processes': True, 'threads_per_worker': 1,
                                    'memory_limit': '2GB', 'output_runtime_results': False, 'metadata': metadata}))
    step13.main(['13', path, '--path_pocs_parameter', str(pocs)])
    res = [p for p in os.listdir(d) if 'WAVELET' in p and p.endswith('.npz')]
    assert res
    icube = open_cube(str(d / sorted(res, key=len)[0]))
    y = icube.data_vars['env_interp']
    assert y.shape == c.data_vars['env'].shape and np.all(np.isfinite(y))
    covered = c.data_vars['fold'] > 0
    assert np.abs(y[:, ~covered]).max() > 0                  # the gaps were filled


def test_cli_netcdf(tmp_path):
    if not h5py_enabled:
        pytest.skip('netCDF needs h5py or xarray')
    d, corners = write_survey(tmp_path)
    cb.main(['10', str(d), *configs(tmp_path, corners, 'median'), '--path_coords', str(d)])
    c = open_cube(str(d / 'synth_median_10x10m_0+5ms_twt-il-xl.nc'))
    assert c.data_vars['amp'].shape[1:] == (32, 32) and c.data_vars['fold'].max() > 1
