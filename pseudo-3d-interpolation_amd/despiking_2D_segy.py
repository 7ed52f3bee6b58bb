"""
Step 8 -- despike SEG-Y file(s) on the GPU, mirror of ``pseudo_3D_interpolation/despiking_2D_segy.py``.

Single-trace noise bursts are found by comparing every sample with the background amplitude (mean, median or rms) of a number of
adjacent traces; where the amplitude exceeds ``threshold x background`` over enough samples of a time window, the burst is scaled
down (with a taper), replaced by the background amplitude, by ``threshold x background``, by the neighbours' median, or zeroed.
Detection and replacement run on the device (HIP unit ``p3d_despike``, ``functions/despike.py``) on the file's own trace-major layout.

Flags, defaults, output naming (``<name>_<txt_suffix>.<ext>``, ``--inplace``, ``--output_dir``), the three kinds of input (a file, a
directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file, ``argparse_parameter.yml`` at ``--verbose >= 1`` and the
``DESPIKE`` line of the textual header are the reference's.  Departures: a spike on one of the first ``window_traces // 2``
traces replaces its own trace; with ``--use_delay`` a split narrower than the trace window passes through unchanged with a warning;
the QC figures of the reference are not produced.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np
import yaml

from .functions import segy_cli
from .functions.despike import despike_2D
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import SegyFile, header_words, update_samples
from .functions.utils import xprint


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(description='Despike SEG-Y file(s) using 2D moving window function.')
    parser.add_argument('input_path', type=str, help='Input file or directory.')
    parser.add_argument('--output_dir', '-o', type=str, help='Output directory for edited SEG-Y file(s)')
    parser.add_argument('--inplace', '-i', action='store_true', help='Edit SEG-Y file(s) inplace')
    parser.add_argument('--suffix', '-s', type=str, default='sgy', help='File suffix. Only used when "input_path" is a directory.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "input_path" is a directory.')
    parser.add_argument('--use_delay', action='store_true',
                        help='Use delay recording time to split input data before despiking (e.g. for TOPAS, Parasound)')
    parser.add_argument('--byte_delay', type=int, default=109, help='Byte position of input delay times in SEG-Y file(s). Default: 109')
    parser.add_argument('--txt_suffix', type=str, default='despk', help='Additional text to append to output filename.')
    parser.add_argument('--mode', '-m', type=str, default='mean', choices=['mean', 'median', 'rms'],
                        help='Mode used to compute background amplitude and detect spikes in data')
    parser.add_argument('--window_time', '-wti', type=int, required=True, help='Moving window shape in time domain (TWT [ms])')
    parser.add_argument('--window_traces', '-wtr', type=int, required=True, help='Moving window shape in offset domain (traces [#])')
    parser.add_argument('--window_overlap', '-wo', type=int, default=10, metavar='PERC', help='Time overlap of moving windows (in percent)')
    parser.add_argument('--threshold_factor', '-t', type=float, help='Threshold x background amplitude will be used for spike detection')
    parser.add_argument('--out_amplitude', '-oa', type=str, default='threshold', choices=['scaled', 'mode', 'threshold', 'zeros', 'median'],
                        help='Spike amplitudes are replaced using selected method')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, choices=[0, 1, 2], help='Level of output verbosity (default: 0).')
    return parser
# fmt: on


MSG_OVERLAP = '[ERROR]    Please set window overlap to a reasonable value [0-99].'
MSG_THRESHOLD = '[ERROR]    Threshold factor must be larger than zero.'
MSG_TOO_FEW = 'Input SEG-Y contains too less traces for despiking ---> skipped file!'
MSG_NOTHING = '*** No spikes removed! Consider adjusting the input parameters. ***'


def wrapper_despiking_2D_segy(in_path, args):
    """Despike one SEG-Y file.  Returns (path, data, data_despiked), both [ns][ntr]; (path, None, None) when the file has fewer traces
    than the trace window."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    target, _, _ = segy_cli.output_target(in_path, args, 'despk')
    if target == in_path:
        say('Updating SEG-Y inplace', kind='warning')
    else:
        say('Creating copy of file in directory:\n', os.path.dirname(target), kind='info')
    segy_cli.copy_to_target(in_path, target, say)

    segy = SegyFile(target)
    if segy.ntraces < args.window_traces:
        return target, None, None
    section, sample_ms = segy.traces(), segy.dt                 # [ntr][ns]: the kernels' layout
    starts = None
    if args.use_delay:
        delay = header_words(segy, args.byte_delay)
        starts = np.flatnonzero(np.diff(delay)) + 1             # a new split wherever the delay time changes
        if starts.size:
            say('Splitting seismic section using `delrt`', kind='info')
    del segy                                                    # the read-only map goes before the file is rewritten
    cleaned = despike_2D(section, args.window_time, sample_ms, args.window_overlap, args.window_traces, args.mode, args.threshold_factor,
                         args.out_amplitude, verbosity=args.verbose, splits=starts, trace_major=True)
    if cleaned is not section:
        update_samples(target, cleaned)
    write_textual_header(target, add_processing_info_header(get_textual_header(target), 'DESPIKE', prefix='_TODAY_', newline=True))
    return target, section.T, cleaned.T


def despike_file(in_path, args):
    """One file through the wrapper; the copy is deleted again when the file is too short or nothing was removed (a file edited in place
    is never deleted)."""
    target, before, after = wrapper_despiking_2D_segy(in_path, args)
    if before is None:
        reason = MSG_TOO_FEW
    elif np.allclose(before, after):
        reason = MSG_NOTHING
    else:
        return True
    xprint(reason, kind='warning', verbosity=args.verbose)
    if target != in_path:
        os.unlink(target)
    return False


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)
    if not 0 <= args.window_overlap <= 99:
        sys.exit(MSG_OVERLAP)
    if args.threshold_factor is None or args.threshold_factor <= 0:
        sys.exit(MSG_THRESHOLD)

    stamp, script = segy_cli.time_stamp(), segy_cli.script_name(__file__)
    in_path = args.input_path
    folder = in_path if os.path.splitext(in_path)[1] == '' else os.path.dirname(in_path)
    if args.verbose >= 1:
        xprint('Saving argparse parameter to file', kind='info', verbosity=args.verbose)
        yml = os.path.join(args.output_dir or folder, f'{stamp}_{script}_argparse_parameter.yml')
        with open(yml, 'w', newline='\n') as fh:
            yaml.safe_dump(vars(args), fh)

    segy_cli.run(__file__, args, lambda path: despike_file(path, args), stamp=stamp)     # the log shares the stamp of the .yml


if __name__ == '__main__':
    main()
