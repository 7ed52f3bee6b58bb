"""Step 11 end to end: ``cube_preprocessing_3D.main`` on small cubes, checked against the golden-tested functions composed in the
reference's order, and step 12 run on its envelope output."""
import datetime
import os

import numpy as np
import pytest
import yaml

from pseudo_3d_interpolation_amd import cube_apply_FFT, cube_preprocessing_3D as cp
from pseudo_3d_interpolation_amd.cube_io import Cube, open_cube, save_cube
from pseudo_3d_interpolation_amd.functions import filter as F
from pseudo_3d_interpolation_amd.functions import signal as S
from pseudo_3d_interpolation_amd.functions.backends import h5py_enabled

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'preproc.npz'))
NT, NIL, NXL = GOLD['chain/x'].shape
ATTRS_TIME = {'amp': {'long_name': 'amplitude', 'units': '-'}, 'env': {'long_name': 'envelope', 'units': '-'}}


def make_cube(tmp_path, ext='.npz'):
    x = GOLD['chain/x'].copy()                  # one all-zero trace at (iline 1, xline 2)
    twt = GOLD['chain/twt'].copy()              # ms, dt 0.2
    cube = Cube({'amp': x, 'fold': np.ones((NIL, NXL), np.float32)}, {'amp': ('twt', 'iline', 'xline'), 'fold': ('iline', 'xline')},
                {'twt': twt, 'iline': np.arange(NIL), 'xline': np.arange(NXL)}, {'history': 'binning;', 'text': 'made'},
                {'amp': {'units': 'V'}}, {'twt': {'units': 'ms', 'dt': 0.2}})
    path = str(tmp_path / f'cube_0+2ms_twt_amp{ext}')
    save_cube(cube, path)
    params = str(tmp_path / 'params.yml')
    with open(params, 'w') as f:
        yaml.safe_dump({'attrs_time': ATTRS_TIME}, f)
    return path, params, x, twt


def run(path, params, *flags):
    return cp.main(['11', path, '--params_netcdf', params, *flags], return_dataset=True)


def traces_last(x):
    return np.moveaxis(x, 0, -1)


def test_each_flag_alone(tmp_path):
    path, params, x, twt = make_cube(tmp_path)
    today = datetime.date.today().strftime('%Y-%m-%d')
    xl = traces_last(x)
    # balance
    out, _ = run(path, params, '--balance', 'max', '--store_ref_amp')
    ref = S.calc_reference_amplitude(xl, axis=-1, scale='max')
    np.testing.assert_allclose(out.data_vars['amp'], np.moveaxis(xl / ref[..., None], -1, 0), rtol=1e-6)
    np.testing.assert_array_equal(out.data_vars['amp_ref'], ref)
    assert out.var_attrs['amp_ref'] == {'description': 'Reference amplitudes used to scale traces', 'method': 'max scaling', 'units': 'V'}
    assert out.attrs['history'] == 'binning;cube_preprocessing_3D: amplitude balancing (max);'
    assert out.attrs['text'] == f'made\n{today}: BALANCE'
    assert out.var_attrs['amp'] == dict(ATTRS_TIME['amp'], balanced='max amplitude')
    assert os.path.exists(str(tmp_path / 'cube_0+2ms_twt_amp_preproc.npz'))
    # gain
    out, _ = run(path, params, '--gain', 'tpow=2', 'agc=1', 'agc_win=0.01')
    want = S.gain(xl, twt / 1000.0, tpow=2.0, agc=1.0, agc_win=0.01)
    np.testing.assert_allclose(out.data_vars['amp'], np.moveaxis(want, -1, 0), rtol=1e-6, atol=1e-6)
    assert out.var_attrs['amp']['gain'] == 'tpow=2.0 agc=1.0 agc_win=0.01 (TWT-based)'
    assert os.path.exists(str(tmp_path / 'cube_0+2ms_twt_amp_AGC.npz'))
    out, _ = run(path, params, '--gain', 'tpow=2', '--use_samples')
    np.testing.assert_allclose(out.data_vars['amp'], np.moveaxis(S.gain(xl, np.arange(NT), tpow=2.0), -1, 0), rtol=1e-6)
    # filter
    out, _ = run(path, params, '--filter', 'bandpass', '--filter_freqs', '50', '100', '800', '1000')
    want = F.bandpass_filter(xl, [50, 100, 800, 1000], fs=5000.0)
    np.testing.assert_array_equal(out.data_vars['amp'], np.moveaxis(want, -1, 0))
    assert out.var_attrs['amp']['filter_freq_Hz'] == '50/100/800/1000'
    # resampling
    out, _ = run(path, params, '-f', '2')
    np.testing.assert_array_equal(out.data_vars['amp'], np.moveaxis(S.resample_poly(xl, 1, 2, axis=-1), -1, 0))
    np.testing.assert_array_equal(out.coords['twt'], np.around(S.get_resampled_twt(twt, NT // 2, NT), 3))
    assert out.coord_attrs['twt'] == {'units': 'ms', 'dt': 0.4, 'resampled': 'True', 'dt_original': 0.2}
    assert os.path.exists(str(tmp_path / 'cube_0+4ms_twt_amp_preproc.npz'))
    out, _ = run(path, params, '-dt', '0.1', '--resampling_function', 'resample')
    np.testing.assert_array_equal(out.data_vars['amp'], np.moveaxis(S.resample(xl, 2 * NT, axis=-1, window='hann'), -1, 0))
    # envelope
    out, _ = run(path, params, '--envelope')
    assert 'amp' not in out.data_vars and out.var_attrs['env'] == ATTRS_TIME['env']
    np.testing.assert_array_equal(out.data_vars['env'], np.moveaxis(S.envelope(xl), -1, 0))
    assert os.path.exists(str(tmp_path / 'cube_0+2ms_twt_env_preproc.npz'))


def test_all_together_then_step_12(tmp_path):
    path, params, x, twt = make_cube(tmp_path)
    x0 = x.copy()
    out, _ = run(path, params, '--balance', 'rms', '--store_ref_amp', '--gain', 'tpow=2', 'agc=1', '--filter', 'bandpass',
                 '--filter_freqs', '50', '100', '800', '1000', '-f', '2', '--envelope')
    xl = traces_last(x)
    ref = S.calc_reference_amplitude(xl, axis=-1, scale='rms')
    y = (xl / ref[..., None]).astype(np.float32)
    y = S.gain(y, twt / 1000.0, tpow=2.0, agc=1.0)
    y = F.bandpass_filter(y, [50, 100, 800, 1000], fs=5000.0)
    y = S.resample_poly(y, 1, 2, axis=-1)
    y = S.envelope(y)
    np.testing.assert_allclose(out.data_vars['env'], np.moveaxis(y, -1, 0), rtol=1e-5, atol=1e-6 * np.abs(y).max())
    np.testing.assert_array_equal(out.data_vars['amp_ref'], ref)
    # the same chain composed from the REFERENCE's functions in its order (make_golden_preproc.py)
    got, want = out.data_vars['env'].reshape(out.data_vars['env'].shape[0], -1).T, GOLD['chain/env'].reshape(GOLD['chain/env'].shape[0], -1).T
    err = np.linalg.norm(got.astype(np.float64) - want, axis=1) / np.maximum(np.linalg.norm(want.astype(np.float64), axis=1), 1e-30)
    assert err.max() < 1e-5, err.max()
    np.testing.assert_allclose(out.data_vars['amp_ref'], GOLD['chain/ref'], rtol=1e-6)
    np.testing.assert_array_equal(out.coords['twt'], GOLD['chain/twt_out'])
    assert out.dims['env'] == ('twt', 'iline', 'xline') and out.data_vars['env'].dtype == np.float32
    assert out.attrs['history'].endswith('cube_preprocessing_3D: amplitude balancing (rms), amplitude gain (tpow=2.0 agc=1.0 (TWT-based)), '
                                         'bandpass (50/100/800/1000 Hz), resampling (factor: 2.0), trace envelope;')
    assert out.attrs['text'].endswith(': BALANCE.GAIN.BANDPASS (50/100/800/1000 Hz).RESAMPLE.ENV')
    outpath = str(tmp_path / 'cube_0+4ms_twt_env_AGC.npz')
    assert os.path.exists(outpath)
    np.testing.assert_array_equal(open_cube(path).data_vars['amp'], x0)
    # step 12 on the envelope
    cube_apply_FFT.main(['12', outpath, '--params_netcdf', params])
    freq = open_cube(str(tmp_path / 'cube_0+4ms_freq_env_AGC.npz'))
    assert 'freq_env' in freq.data_vars and np.all(np.isfinite(freq.data_vars['freq_env']))


def test_netcdf_copy(tmp_path):
    if not h5py_enabled:
        pytest.skip('netCDF needs h5py or xarray')
    path, params, x, twt = make_cube(tmp_path, '.nc')
    out, _ = run(path, params, '--envelope')
    np.testing.assert_array_equal(out.data_vars['env'], np.moveaxis(S.envelope(traces_last(x)), -1, 0))
    assert os.path.exists(str(tmp_path / 'cube_0+2ms_twt_env_preproc.nc'))
