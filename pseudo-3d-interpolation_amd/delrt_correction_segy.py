"""
Step 3 -- fix an incorrect DelayRecordingTime in SEG-Y profile(s) on the GPU, mirror of ``pseudo_3D_interpolation/delrt_correction_segy.py``.

Where the delay of consecutive traces changes, the maximum amplitude of the first trace behind the change is compared with the maxima
of ``--win_ntraces`` neighbours to each side within ``--win_nsamples`` samples around it: traces recorded in the same window show the
seafloor there, the others do not.  When that pattern and the pattern of the delays disagree by one trace, the trace gets the other
delay.  The peaks and the window maxima of all changes of a file come from one launch (HIP unit ``p3d_delrt``, ``functions/delrt.py``).

Flags, defaults, output naming (``<name>_delrt.<ext>`` or ``--txt_suffix``, ``--inplace``, ``--output_dir``), the three kinds of input (a
file, a directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file, the "skipped" messages and the ``DELRT FIX``
line of the textual header are the reference's.  Departures: the corrected delay is written to the file that is produced,
copy or in place (the reference writes it only with ``--inplace``); and it is written to the trace the decision names (the reference's
message names that trace, yet it writes the header of the first trace behind the change -- the two differ for an offset trace).
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

from .functions import segy_cli
from .functions.delrt import correct_delay_changes, correct_single_trace_DelayRecordingTime, delay_changes  # noqa: F401
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import SegyFile, header_words, write_header_words
from .functions.utils import xprint

MSG_SKIPPED = 'Skipped: Identical "DelayRecordingTime" for whole SEG-Y file'


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Fix incorrect "DelayRecordingTime" in SEG-Y file(s).')
    parser.add_argument('input_path', type=str, help='Input file or directory.')
    parser.add_argument('--output_dir', '-o', type=str,
                        help='Output directory for edited SEG-Y file(s).')
    parser.add_argument('--inplace', '-i', action='store_true',
                        help='Edit SEG-Y file(s) inplace')
    parser.add_argument('--suffix', '-s', type=str,
                        help='File suffix. Only used when "input_path" is a directory.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "input_path" is a directory.')
    parser.add_argument('--txt_suffix', type=str,
                        help='Additional text to append to output filename.')
    parser.add_argument('--byte_delay', type=int, default=109,
                        help='Byte position of input delay times in SEG-Y file(s) (default: 109, "DelayRecordingTime")')
    parser.add_argument('--win_ntraces', type=int, default=5,
                        help='Number of traces in comparison window.')
    parser.add_argument('--win_nsamples', type=int, default=120,
                        help='Number of samples in comparison window.')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0).')
    return parser
# fmt: on


def check_varying_DelayRecordingTimes(path, byte_delay=109):
    """True when the SEG-Y file at ``path`` holds more than one DelayRecordingTime (header word at ``byte_delay``)."""
    return len(np.unique(header_words(SegyFile(path), byte_delay))) > 1


def wrapper_delrt_correction_segy(in_path, args):
    """Correct the DelayRecordingTime of one SEG-Y file.  Returns False for a file with one delay (nothing is written), else the list of
    corrections ``[(idx, trace, old, new)]`` (possibly empty) that were written to the output file."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    if not check_varying_DelayRecordingTimes(in_path, args.byte_delay):
        return False
    path, _, _ = segy_cli.copied_target(in_path, args, 'delrt', say)

    segy = SegyFile(path)
    delrt = header_words(segy, args.byte_delay)
    fldr, tracr = segy.header('FieldRecord'), segy.header('TRACE_SEQUENCE_FILE')
    changes = delay_changes(delrt)
    say(f'Found < {len(changes) - 1} > different DelayRecordingTimes: {dict(zip(changes.tolist(), delrt[changes].tolist()))}', kind='info')
    fixes = correct_delay_changes(segy, delrt, args.win_ntraces, args.win_nsamples, say=say)
    del segy                                                                         # the read-only map goes before the file is rewritten
    for idx, trace, old, new in fixes:
        say(f'Changing DelayRecordingTime for FRN #{fldr[trace]} (idx:{tracr[trace] - 1}) [i:{trace - idx + args.win_ntraces}] from > {old} < to > {new} <',
            kind='info')
    if fixes:
        write_header_words(path, args.byte_delay, [f[1] for f in fixes], [f[3] for f in fixes])

    text = add_processing_info_header(get_textual_header(path), f'DELRT FIX (BYTE:{args.byte_delay})', prefix='_TODAY_')
    write_textual_header(path, text)
    return fixes


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    segy_cli.run(__file__, args, lambda path: wrapper_delrt_correction_segy(path, args), skipped=MSG_SKIPPED,
                 summary='Fixed a total of < {done} > out of < {total} > files', empty='[INFO]    ' + segy_cli.MSG_NO_FILES)


if __name__ == '__main__':
    main()
