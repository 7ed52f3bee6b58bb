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
import datetime
import glob
import os
import re
import sys
from contextlib import redirect_stdout
from functools import partial
from shutil import copy2

import numpy as np
import yaml

from .functions.despike import despike_2D
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import TRACE_FIELDS, SegyFile, update_samples
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


ANSI_COLOUR = re.compile(r'\x1b\[[0-9;]*m')
MSG_OVERLAP = '[ERROR]    Please set window overlap to a reasonable value [0-99].'
MSG_THRESHOLD = '[ERROR]    Threshold factor must be larger than zero.'
MSG_TOO_FEW = 'Input SEG-Y contains too less traces for despiking ---> skipped file!'
MSG_NOTHING = '*** No spikes removed! Consider adjusting the input parameters. ***'


def clean_log_file(path_log, newline='\n'):
    """Strip the terminal colour codes from a log file."""
    with open(path_log) as fh:
        text = fh.read()
    with open(path_log, 'w', newline=newline) as fh:
        fh.write(ANSI_COLOUR.sub('', text))


def output_path(in_path, args):
    """Where the despiked copy of ``in_path`` goes (the file itself with ``--inplace``, which supersedes ``--output_dir``)."""
    if args.inplace:
        return in_path
    folder, name = os.path.split(in_path)
    if args.output_dir is not None:
        if not os.path.isdir(args.output_dir):
            raise FileNotFoundError(f'The output directory > {args.output_dir} < does not exist')
        folder = args.output_dir
    stem, ext = os.path.splitext(name)
    tag = 'despk' if args.txt_suffix is None else args.txt_suffix
    return os.path.join(folder, f'{stem}_{tag}{ext}')


def header_words(segy, byte):
    """The trace-header word at 1-based ``byte`` of every trace.  A byte that starts one of the reader's named fields (``TRACE_FIELDS``) is
    read with that field's width; any other byte is read as a big-endian int16, the width of the delay time and its neighbours."""
    for name, (b, _) in TRACE_FIELDS.items():
        if b == byte:
            return segy.header(name)
    if not 1 <= byte <= 239:
        raise ValueError(f'--byte_delay {byte} is outside the 240-byte trace header')
    raw = np.memmap(segy.path, np.uint8, 'r')
    start = raw.size - segy.ntraces * segy._dtype.itemsize
    rows = raw[start:].reshape(segy.ntraces, segy._dtype.itemsize)[:, byte - 1:byte + 1]
    return np.ascontiguousarray(rows).view('>i2').ravel().astype(np.int64)


def wrapper_despiking_2D_segy(in_path, args):
    """Despike one SEG-Y file.  Returns (path, data, data_despiked), both [ns][ntr]; (path, None, None) when the file has fewer traces
    than the trace window."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    target = output_path(in_path, args)
    if target == in_path:
        say('Updating SEG-Y inplace', kind='warning')
    else:
        say('Creating copy of file in directory:\n', os.path.dirname(target), kind='info')
        if os.path.exists(target):
            say('Output file already exists and will be removed!', kind='warning')
            os.unlink(target)
        copy2(in_path, target)

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


def input_files(in_path, args):
    """(files, folder, single): the files named by a SEG-Y file, a directory (``*{filename_suffix}.{suffix}``) or a ``.txt`` list (names
    relative to the list), the folder that takes the log, and whether the input was one SEG-Y file."""
    ext = os.path.splitext(in_path)[1]
    if os.path.isdir(in_path):
        glob_pattern = '*' + (args.filename_suffix or '') + '.' + (args.suffix if args.suffix is not None else 'sgy')
        return sorted(glob.glob(os.path.join(in_path, glob_pattern))), in_path, False
    if not os.path.isfile(in_path):
        raise FileNotFoundError('Invalid input file')
    folder = os.path.dirname(in_path)
    if ext != '.txt':
        return [in_path], folder, True
    with open(in_path) as fh:
        entries = [ln.strip() for ln in fh if ln.strip()]
    return [e if os.path.isabs(e) else os.path.join(folder, e) for e in entries], folder, False


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)
    if not 0 <= args.window_overlap <= 99:
        sys.exit(MSG_OVERLAP)
    if args.threshold_factor is None or args.threshold_factor <= 0:
        sys.exit(MSG_THRESHOLD)

    stamp = datetime.datetime.now().strftime('%Y-%m-%dT%H%M%S')
    script = os.path.splitext(os.path.basename(__file__))[0]
    in_path = args.input_path
    folder = in_path if os.path.splitext(in_path)[1] == '' else os.path.dirname(in_path)
    if args.verbose >= 1:
        xprint('Saving argparse parameter to file', kind='info', verbosity=args.verbose)
        yml = os.path.join(args.output_dir or folder, f'{stamp}_{script}_argparse_parameter.yml')
        with open(yml, 'w', newline='\n') as fh:
            yaml.safe_dump(vars(args), fh)

    files, folder, single = input_files(in_path, args)
    if single:
        despike_file(files[0], args)
        sys.exit()
    if not files:
        sys.exit('No input files to process. Exit process.')
    log_path = os.path.join(folder, f'{stamp}_{script}.log')
    with open(log_path, 'w', newline='\n') as log, redirect_stdout(log):
        xprint(f'Processing total of < {len(files)} > files', kind='info', verbosity=args.verbose)
        for one in files:
            despike_file(one, args)
    clean_log_file(log_path)


if __name__ == '__main__':
    main()
