"""
Step 5 -- compensate the static of SEG-Y profile(s) on the GPU, mirror of ``pseudo_3D_interpolation/static_correction_segy.py``.

The static of a trace is the deviation of its seafloor from the smooth seafloor along the profile, taken either from the first positive
amplitude peak of the seafloor reflection (mode ``amp``: STA/LTA detection and peak pick on the device, HIP unit ``p3d_static``,
``functions/static.py``) or from the ``SourceWaterDepth`` header word (mode ``swdep``).  The traces are shifted by it on the device, and
the static is logged in the trace headers: byte 103 ``TotalStaticApplied`` (ms x 1000), byte 233 its scalar (-1000), byte 237 the
TWT of the seafloor (ms x 1000, with ``--write_seafloor2trace``).

Flags, defaults, output naming (``<name>_<txt_suffix>.<ext>``, ``--inplace``, ``--output_dir``), the three kinds of input (a file, a
directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file, the auxiliary ``*.sta`` file and the ``STATIC CORRECTION``
line(s) of the textual header are the reference's.  Departures: a file counts as zero-padded when its path holds 'pad' or
the binary header names an original sample count other than 0 and other than the sample count (the reference also takes the padded
route when that word is 0); the seafloor TWT is computed whenever it is written (the reference needs ``--write_seafloor2trace`` for
``--write_aux`` in mode ``amp`` on unpadded files); mode ``swdep`` on a file with empty water depths is an error with a message.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

from .functions import segy_cli
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import TRACE_FIELDS, SegyFile, header_words, update_headers, update_samples
from .functions.static import compensate_static, get_static, samples2twt, seafloor_stages, twt2samples
from .functions.utils import xprint

STATIC_SCALAR = 1000
BYTE_STATIC, BYTE_SCALAR, BYTE_SEAFLOOR = (TRACE_FIELDS[k][0] for k in ('TotalStaticApplied', 'UnassignedInt1', 'UnassignedInt2'))
MSG_TARGET = '[ERROR]    Either `output_dir` OR `args.inplace` must be specified.'


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Compensate static on seismic profile(s) using either "SourceWaterDepth" (swdep) '
        + 'or first positive amplitude peak of seafloor reflection (amp).')
    parser.add_argument('input_path', type=str, help='Input file or directory.')
    parser.add_argument('--output_dir', '-o', type=str, help='Output directory for edited SEG-Y file(s)')
    parser.add_argument('--suffix', '-s', type=str, help='File suffix. Only used when "input_path" is a directory.')
    parser.add_argument('--inplace', '-i', action='store_true', help='Edit SEG-Y file(s) inplace')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "input_path" is a directory.')
    parser.add_argument('--txt_suffix', type=str, default='static', help='Additional text to append to output filename')
    parser.add_argument('--use_delay', action='store_true',
                        help='Use delay recording time to split input data before despiking (e.g. for TOPAS, Parasound)')
    parser.add_argument('--byte_delay', type=int, default=109, help='Byte position of input delay times in SEG-Y file(s). Default: 109')
    parser.add_argument('--mode', '-m', type=str, default='amp', choices=['amp', 'swdep'],
                        help='Use either peak seafloor amplitude [amp] or stored SourceWaterDepth [swdep] (if available).')
    parser.add_argument('--win_samples', type=int, default=30, help='Length of vertical padding (in samples) for seafloor detection.')
    parser.add_argument('--nsta', type=int, help='Length of short time average window (in samples).')
    parser.add_argument('--nlta', type=int, help='Length of long time average window (in samples).')
    parser.add_argument('--win_median', type=int, default=11, help='Length of median filter window (in traces).')
    parser.add_argument('--n_amp_samples', type=int, default=5, help='Selecting `n_amp_samples` amplitude samples within seafloor detection window.')
    parser.add_argument('--win_mad', type=int, help='Moving window length for MAD filter (traces [#])')
    parser.add_argument('--win_sg', type=int, default=7, help='Moving window length for Savitzky-Golay filter (traces [#])')
    parser.add_argument('--limit_shift', nargs='?', type=int, default=12, const=12,
                        help='Limit maximum vertical shift of individual traes (in samples)')
    parser.add_argument('--limit_depressions', nargs='+', type=int, default=[10, 10, 5],
                        help='Limit maximum vertical shift in area of seafloor depressions '
                        + 'using a transition zone [pad, max_edges, max_center] (as integer)')
    parser.add_argument('--write_seafloor2trace', action='store_true',
                        help='If mode is "amp": write TWT of peak seafloor amplitude to SEG-Y trace header')
    parser.add_argument('--write_aux', action='store_true', help='Write trace information and computed static to auxiliary file (*.sta)')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, choices=[0, 1, 2], help='Level of output verbosity (default: 0)')
    return parser
# fmt: on


def is_padded(path, hns, nso):
    """A zero-padded file: 'pad' in its path, or an original sample count in the binary header that differs from the sample count."""
    return 'pad' in path or (nso != 0 and nso != hns)


def scaled_depth(swdep, scalel):
    """SourceWaterDepth with ElevationScalar applied when all scalars have one sign (positive: multiply, negative: divide)."""
    if np.all(scalel > 0):
        return swdep * np.abs(scalel)
    if np.all(scalel < 0):
        return swdep / np.abs(scalel)
    return swdep


def seafloor_static(section, twt, dt, delrt, padded, nso, args, say):
    """Mode ``amp``: (static in samples as `get_static` returns it, TWT of the picked seafloor per trace)."""
    kw = dict(nsta=args.nsta, nlta=args.nlta, win=args.win_samples, win_median=args.win_median, n=args.n_amp_samples, trace_major=True)
    if padded:
        stages = seafloor_stages(section, nso=nso, **kw)
        idx_amp = stages['idx'] + stages['start']
        twt_seafloor = twt[idx_amp]
    else:
        idx_amp = seafloor_stages(section, **kw)['idx']
        picked = idx_amp.copy()
        changes = np.flatnonzero(np.diff(delrt))
        if args.use_delay and changes.size >= 1:
            say('Account for variable DelayRecordingTimes (`delrt`)', kind='info')
            idx_amp = idx_amp + twt2samples((delrt - delrt.min()).astype('int'), dt=dt).astype('int')
        twt_seafloor = twt[picked + twt2samples((delrt - delrt[0]).astype('int'), dt=dt).astype('int')]
    static = get_static(idx_amp, kind='diff', interp_kind='cubic', win_mad=args.win_mad, win_sg=args.win_sg, limit_perc=False,
                        limit_samples=args.limit_shift, limit_by_MAD=3, limit_depressions=args.limit_depressions)
    return static, twt_seafloor


def wrapper_static_correction_segy(in_path, args):
    """Apply the static correction to one SEG-Y file.  Returns (path, data, data_corrected), both [ns][ntr]."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    path, aux_dir, out_name = segy_cli.copied_target(in_path, args, 'static', say)

    segy = SegyFile(path)
    dt, ns = segy.dt, segy.ns
    tracl, tracr, fldr = (segy.header(k) for k in ('TRACE_SEQUENCE_LINE', 'TRACE_SEQUENCE_FILE', 'FieldRecord'))
    delrt = header_words(segy, args.byte_delay)
    twt = float(segy.header('DelayRecordingTime')[0]) + np.arange(ns) * dt          # TWT of the samples [ms], from the first trace's delay
    swdep = scaled_depth(segy.header('SourceWaterDepth'), segy.header('ElevationScalar'))
    section = segy.traces()                                                          # [ntr][ns]: the kernels' layout
    hns, nso = segy.binary['Samples'], segy.binary['SamplesOriginal']
    ntr = segy.ntraces
    del segy                                                                         # the read-only map goes before the file is rewritten

    twt_seafloor = None
    if args.mode == 'swdep':
        if np.count_nonzero(swdep) != ntr:
            raise ValueError(f'mode "swdep" needs a SourceWaterDepth in every trace ({ntr - np.count_nonzero(swdep)} of {ntr} are zero)')
        static_depth = get_static(swdep, kind='diff', interp_kind='cubic', win_mad=args.win_mad, win_sg=args.win_sg, limit_perc=False,
                                  limit_samples=args.limit_shift, limit_by_MAD=3, limit_depressions=args.limit_depressions)
        corrected, static_samples = compensate_static(section, static_depth, dt=dt, units='ms', cnv_d2s=True, trace_major=True)
    else:
        static, twt_seafloor = seafloor_static(section, twt, dt, delrt, is_padded(path, hns, nso), nso if nso != 0 else hns, args, say)
        corrected, static_samples = compensate_static(section, static, dt=dt, units='ms', trace_major=True)

    static_ms = samples2twt(static_samples, dt=dt)
    if args.write_aux:
        last = swdep if args.mode == 'swdep' else twt_seafloor
        with open(os.path.join(aux_dir, f'{out_name}.sta'), mode='w', newline='\n') as sta:
            sta.write(','.join(['tracl', 'tracr', 'fldr', 'static_samples', 'static_ms', 'swdep_m' if args.mode == 'swdep' else 'seafloor_ms']) + '\n')
            for i in range(ntr):
                sta.write(f'{tracl[i]},{tracr[i]},{fldr[i]},{static_samples[i]:d},{static_ms[i]:.3f},{last[i]:.2f}\n')

    seafloor2trace = args.mode == 'amp' and args.write_seafloor2trace
    text = add_processing_info_header(get_textual_header(path), f'STATIC CORRECTION:{args.mode} (byte:{BYTE_STATIC}) with SCALAR (byte:{BYTE_SCALAR})',
                                      prefix='_TODAY_')
    if seafloor2trace:
        text = add_processing_info_header(text, f'-> SEAFLOOR (byte:{BYTE_SEAFLOOR}) with SCALAR (byte:{BYTE_SCALAR})', prefix='_TODAY_')
    write_textual_header(path, text)

    words = {'TotalStaticApplied': (static_ms * STATIC_SCALAR).astype('int32'), 'UnassignedInt1': -STATIC_SCALAR}
    if seafloor2trace:
        words['UnassignedInt2'] = (twt_seafloor * STATIC_SCALAR).astype('int32')
    update_headers(path, words)
    update_samples(path, corrected)
    return path, section.T, corrected.T


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)
    if args.inplace == (args.output_dir is not None):
        sys.exit(MSG_TARGET)
    segy_cli.run(__file__, args, lambda path: wrapper_static_correction_segy(path, args), catch=True)


if __name__ == '__main__':
    main()
