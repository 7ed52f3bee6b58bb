"""
Step 11 -- pre-processing of a (pseudo-)3D cube on the GPU, mirror of ``pseudo_3D_interpolation/cube_preprocessing_3D.py``.

Command line (``11_cube_preprocessing``, :58-101) and order of the operations (:170-360), all along twt, trace by trace:

  - amplitude **balancing** (time-invariant): ``calc_reference_amplitude`` (rms or max) per trace, ``cube / ref``;
  - time-variant **gain** (``functions.signal.gain``, the reference's port of Seismic Unix ``sugain``);
  - zero-phase Butterworth **filtering** (``functions.filter``: scipy's ``buttord`` / ``butter`` / ``sosfiltfilt`` design);
  - **resampling** (``resample_poly`` with integer up / down, or the FFT ``resample``);
  - trace **envelope** (``abs(hilbert(x))``).

The cube is uploaded once (in chunks of traces when it is larger than the free device memory), every selected operation runs on
device buffers (HIP unit ``p3d_preproc``, include/p3d.h), and the result is downloaded once.  Only small tables (gain curves,
filter sections, FIR taps, windows, spectral factors) are built on the host in NumPy.  Cubes are read and written through
``cube_io`` (``.nc`` or ``.npz``); the output keeps the input's file type.

Departures from the reference:

* ``qclip`` and ``norm_rms`` work per trace.  In the reference, ``gain`` broadcasts the per-trace statistic of an
  ``(iline, xline, twt)`` chunk without ``keepdims`` and raises ``ValueError``; they only work there on a single trace.
* ``agc_kind=rms|mean|median`` is accepted as a string (the reference's parser calls ``float()`` on it and fails).
* Output is float32 throughout (scipy's filters return float64; the reference declares float32 output).
* A missing ``history`` / ``text`` attribute counts as empty.
* ``--window_resample`` supports the windows without parameters (hann, hamming, blackman, bartlett, boxcar); any other raises
  ``NotImplementedError``.
"""
import argparse
import ast
import datetime
import os
import re
import sys

import numpy as np
import yaml

from . import _ffi
from .cube_io import open_cube, save_cube
from .functions.filter import design_filter, sos_padlen, sosfilt_zi
from .functions.signal import envelope_op, gain_tables, get_resampled_twt, resample_op, resample_poly_op
from .functions.utils import convert_twt, ffloat, xprint

def _gain_value(key, text):
    """One ``key=value`` gain argument: ``linear`` is a Python literal (a (start, stop) tuple), ``pgc`` a sequence of
    ``(twt,gain)`` pairs turned into a dict, ``agc_kind`` stays a string, every other value is a float."""
    name = key.lower()
    if name == 'linear':
        return ast.literal_eval(text)
    if name == 'pgc':
        return {float(t): float(g) for t, g in re.findall(r'\(\s*([^(),\s]+)\s*,\s*([^(),\s]+)\s*\)', text)}
    if name == 'agc_kind':
        return text
    return float(text)


class ParseGainArguments(argparse.Action):
    """Collect ``--gain key=value ...`` into an ordered dict of gain keyword arguments (see ``_gain_value``)."""

    def __call__(self, parser, namespace, values, option_string=None):  # noqa
        params = {}
        for item in values:
            key, text = item.split('=')
            params[key] = _gain_value(key, text)
        setattr(namespace, self.dest, params)


def define_input_args():  # noqa
    """Command line of step 11: the reference's flags, short options, choices and defaults."""
    p = argparse.ArgumentParser(description='Pre-process a binned (pseudo-)3D cube along twt on the GPU: trace balancing, '
                                            'time-variant gain, Butterworth filtering, resampling and the trace envelope.')
    p.add_argument('path_cube', type=str, help='cube to process (.nc or .npz)')
    p.add_argument('--path_out', type=str, help='output file (default: derived from the input name)')
    p.add_argument('--fsuffix', type=str, default='preproc', help='suffix of the derived output name')
    p.add_argument('--params_netcdf', type=str, required=True, help='YAML file with the netCDF attributes (attrs_time)')
    # time-variant gain / time-invariant balancing
    p.add_argument('--gain', nargs='*', default=None, action=ParseGainArguments,
                   help='gain keywords as key=value (tpow, epow, etpow, ebase, gpow, agc, agc_win, agc_kind, agc_sqrt, clip, pclip, '
                        'nclip, qclip, linear=(a,b), pgc=((t,g),...), bias, scale, norm, norm_rms)')
    p.add_argument('--use_samples', action='store_true', help='gain curves over sample numbers rather than twt in seconds')
    p.add_argument('--balance', type=str, nargs='?', const='rms', choices=['rms', 'max'],
                   help='divide every trace by its rms (default when given alone) or maximum amplitude')
    p.add_argument('--store_ref_amp', action='store_true', help='write the balancing amplitudes as the variable <var>_ref')
    # Butterworth filter
    p.add_argument('--filter', type=str, default=None, choices=['lowpass', 'highpass', 'bandpass'], help='zero-phase filter type')
    p.add_argument('--filter_freqs', type=int, nargs='+', help='corner frequencies in Hz (4 for bandpass, 2 otherwise)')
    # resampling
    p.add_argument('--resampling_function', type=str, default='resample_poly', choices=['resample', 'resample_poly'],
                   help='polyphase FIR (resample_poly) or FFT (resample) resampling')
    p.add_argument('--resampling_interval', '-dt', type=float, help='new sampling interval in ms')
    p.add_argument('--resampling_frequency', '-fs', type=float, help='new sampling rate in Hz')
    p.add_argument('--resampling_factor', '-f', type=float, help='new interval / old interval (< 1 upsamples, > 1 downsamples)')
    p.add_argument('--window_resample', type=str, default='hann', help='resampling window (hann, hamming, blackman, bartlett, boxcar)')
    # envelope
    p.add_argument('--envelope', action='store_true', help='replace the traces by their envelope (variable env)')
    p.add_argument('--verbose', '-V', type=int, nargs='?', default=0, const=1, choices=[0, 1, 2], help='verbosity (0, 1 or 2)')
    return p


def output_path(path_cube, gain_args, fsuffix):
    """Output path before resampling / envelope renames: ``<basename>_<fsuffix>`` (``AGC`` when a gain key contains 'agc');
    ``.nc`` for netCDF input, the input's own extension otherwise."""
    dir_work, filename = os.path.split(path_cube)
    basename, suffix = os.path.splitext(filename)
    fsuffix = 'AGC' if gain_args and 'agc' in '\t'.join(gain_args) else fsuffix
    ext = '.nc' if suffix.lower() == '.nc' else suffix
    return os.path.join(dir_work, f'{basename}_{fsuffix}{ext}')


def rename_resampled(path, resampling_interval):
    """The reference's file-name rewrite of the sampling interval: ``<d>+<ddd>ms`` -> the new interval."""
    return re.sub(r'\d{1,2}\+\d{0,3}(ms)', ffloat(resampling_interval).replace('.', '+') + 'ms', path)  # noqa


def gain_string(kwargs_gain, use_samples):
    s = ' '.join([f'{key}={val}' for key, val in kwargs_gain.items() if key != 'twt'])
    return s + (' (sample-based)' if use_samples else ' (TWT-based)')


def main(argv=sys.argv, return_dataset=False):  # noqa
    """Pre-process a 3D cube (step 11)."""
    TODAY = datetime.date.today().strftime('%Y-%m-%d')
    SCRIPT = os.path.splitext(os.path.basename(__file__))[0]

    parser = define_input_args()
    args = parser.parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)

    path_cube = args.path_cube
    path_cube_proc = output_path(path_cube, args.gain, args.fsuffix)

    resampling_interval = resampling_factor = None
    if args.resampling_interval is not None:
        resampling_interval = args.resampling_interval
    elif args.resampling_frequency is not None:
        resampling_interval = (1 / args.resampling_frequency) * 1000
    elif args.resampling_factor is not None:
        resampling_factor = args.resampling_factor

    # (0) open cube
    cube = open_cube(path_cube)
    dim = cube.slice_dim()
    var = [v for v in cube.data_vars if v != 'fold'][0]
    var_ref = f'{var}_ref'
    dims = cube.dims[var]
    data = np.transpose(np.asarray(cube.data_vars[var]), [dims.index(dim), dims.index('iline'), dims.index('xline')])
    twt = np.asarray(cube.coords[dim])
    twt_attrs = dict(cube.coord_attrs.get(dim, {}))
    twt_s = convert_twt(twt, twt_attrs.get('units', 'ms'), 's')
    dt = twt_attrs.get('dt', np.median(np.diff(twt)))  # sampling interval (ms)
    n_samples = twt.size

    with open(args.params_netcdf, 'r') as f_attrs:
        kwargs_nc = yaml.safe_load(f_attrs)
    var_new = 'env' if args.envelope else var
    attrs_var = dict(kwargs_nc['attrs_time'][var_new])
    _history = f'{SCRIPT}:'
    _text = f'{TODAY}: '

    ops = []
    # (1) balance traces (time-invariant)
    if args.balance is not None:
        xprint(f'Balance traces using < {args.balance} > amplitude for scaling (time-invariant)', kind='info', verbosity=args.verbose)
        ops.append(('balance', 0 if args.balance == 'rms' else 1))
        attrs_var.update({'balanced': f'{args.balance} amplitude'})
        _history += f' amplitude balancing ({args.balance}),'
        _text += 'BALANCE.'

    # (2) time-variant gain
    if args.gain is not None:
        kwargs_gain = dict(args.gain)
        gain_twt = np.arange(twt_s.size) if args.use_samples else twt_s
        prm, curves = gain_tables(n_samples, gain_twt, **kwargs_gain)
        ops.append(('gain', prm, curves))
        kwargs_gain_str = gain_string(kwargs_gain, args.use_samples)
        attrs_var.update({'gain': kwargs_gain_str})
        _history += f' amplitude gain ({kwargs_gain_str}),'
        _text += 'GAIN.'

    # (3) frequency filter
    if args.filter is not None:
        if args.filter_freqs is None:
            raise ValueError('Filter frequencies must be specified!')
        fs = 1 / (dt / 1000)
        _, _, sos = design_filter(args.filter_freqs, fs, args.filter)
        padlen = sos_padlen(sos)
        if n_samples <= padlen:
            raise ValueError(f'The length of the input vector x must be greater than padlen, which is {padlen}.')
        ops.append(('filter', sos, sosfilt_zi(sos), padlen))
        _filter_freq_str = '/'.join(str(f) for f in args.filter_freqs)
        attrs_var.update({'filter': args.filter, 'filter_freq_Hz': _filter_freq_str})
        _history += f' {args.filter} ({_filter_freq_str} Hz),'
        _text += f'{args.filter.upper()} ({_filter_freq_str} Hz).'

    # (4) resampling
    resampled = any(a is not None for a in (args.resampling_interval, args.resampling_frequency, args.resampling_factor))
    if resampled:
        if resampling_interval is not None:
            resampling_factor = resampling_interval / dt
        elif resampling_factor is not None:
            resampling_interval = resampling_factor * dt
        n_resamples = int(np.ceil(n_samples / resampling_factor))
        if args.resampling_function == 'resample':
            ops.append(resample_op(n_samples, n_resamples, window=args.window_resample))
        else:
            up = 1 / resampling_factor if resampling_factor < 1 else 1
            down = resampling_factor if resampling_factor > 1 else 1
            op = resample_poly_op(n_samples, up, down, window=args.window_resample)
            if op[5] != n_resamples:
                raise ValueError(f'resample_poly gives {op[5]} samples, the resampled twt has {n_resamples}')
            ops.append(op)
        xprint(f'Resample > {dim} < from > {dt} < to > {resampling_interval} < ms', kind='info', verbosity=args.verbose)
        _history += f' resampling (factor: {resampling_factor}),'
        _text += 'RESAMPLE.'
        path_cube_proc = rename_resampled(path_cube_proc, resampling_interval)

    # (5) envelope
    if args.envelope:
        n_env = n_samples
        for op in ops:
            n_env = _ffi._op_len(op, n_env)
        ops.append(envelope_op(n_env))
        _history += ' trace envelope,'
        _text += 'ENV.'
        path_cube_proc = path_cube_proc.replace(var, var_new)

    # run the chain on the GPU: one upload, one download per chunk of traces
    out, refs = _ffi.trace_ops(data, ops) if ops else (data.astype(np.float32), [])

    cube_out = cube.copy_meta()
    for k, v in cube.data_vars.items():
        if k != var:
            cube_out.data_vars[k] = v
            cube_out.dims[k] = cube.dims[k]
            cube_out.var_attrs[k] = dict(cube.var_attrs.get(k, {}))
    if args.balance is not None and args.store_ref_amp:
        cube_out.data_vars[var_ref] = refs[0]
        cube_out.dims[var_ref] = ('iline', 'xline')
        cube_out.var_attrs[var_ref] = {
            'description': 'Reference amplitudes used to scale traces',
            'method': f'{args.balance} scaling',
            'units': cube.var_attrs.get(var, {}).get('units', '-'),
        }
    if resampled:
        attrs = dict(twt_attrs)
        attrs.update(dt=resampling_interval)
        attrs.update({'resampled': 'True', 'dt_original': dt})
        cube_out.coords[dim] = np.around(get_resampled_twt(twt, n_resamples, n_samples).astype('float64'), 3)
        cube_out.coord_attrs[dim] = attrs
    cube_out.data_vars[var_new] = out
    cube_out.dims[var_new] = (dim, 'iline', 'xline')
    cube_out.var_attrs[var_new] = attrs_var
    cube_out.attrs.update({
        'history': (cube_out.attrs.get('history') or '') + f'{_history[:-1]};',  # remove trailing comma
        'text': (cube_out.attrs.get('text') or '') + f'\n{_text[:-1]}',          # remove trailing period
    })

    path_cube_proc = args.path_out if args.path_out is not None else path_cube_proc
    xprint(f'Write output data to file > {os.path.basename(path_cube_proc)} <', kind='info', verbosity=args.verbose)
    save_cube(cube_out, path_cube_proc)

    if return_dataset:
        return cube_out, cube
    return None


if __name__ == '__main__':
    main()
