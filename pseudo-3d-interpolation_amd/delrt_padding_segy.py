"""
Step 4 -- zero-pad the traces of SEG-Y profile(s) recorded in window mode on the GPU, mirror of ``pseudo_3D_interpolation/delrt_padding_segy.py``.

Traces of a fixed length whose DelayRecordingTime varies along the profile are padded with zeros at top and bottom, so that all share the
time axis from the smallest delay to the largest delay plus the window length (placement on the device: HIP unit ``p3d_delrt``,
``functions/delrt.py``).  The output ``<name>_pad.<ext>`` (or ``--txt_suffix``) is a new file with the new sample count: textual, binary,
extended and trace headers are the source's, but for the sample count (binary header and every trace), ``SamplesOriginal`` = the old
count and DelayRecordingTime (byte 109) = the smallest delay, and the line ``PAD DELRT (byte:109)`` in the textual header -- what step 5
recognises a padded file by.  Flags, defaults, the three kinds of input (a file, a directory with ``--suffix`` / ``--filename_suffix``, a
``.txt`` list), the log file and the "skipped" message for a file with one delay are the reference's.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

from .functions import segy_cli
from .functions.delrt import pad_trace_data
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import TRACE_FIELDS, SegyFile, header_words, write_resized
from .functions.utils import xprint

MSG_SKIPPED = 'Continuous "DelayRecordingTime" for whole SEG-Y file --> skipped!'
BYTE_DELRT = TRACE_FIELDS['DelayRecordingTime'][0]


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Pad time delays in SEG-Y file(s) using "DelayRecordingTime".')
    parser.add_argument('input_path', type=str, help='Input file or directory.')
    parser.add_argument('--output_dir', '-o', type=str,
                        help='Output directory for padded SEG-Y file(s).')
    parser.add_argument('--suffix', '-s', type=str,
                        help='File suffix. Only used when "input_path" is a directory.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "input_path" is a directory.')
    parser.add_argument('--txt_suffix', type=str,
                        help='Additional text to append to output filename.')
    parser.add_argument('--byte_delay', type=int, default=109,
                        help='Byte position of input delay times in SEG-Y file(s) (default: 109, "DelayRecordingTime")')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0).')
    return parser
# fmt: on


def wrapper_delrt_padding_segy(in_path, args):
    """Pad one SEG-Y file.  Returns False for a file with one delay (nothing is written), else the path of the padded file."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    target, _, _ = segy_cli.output_target(in_path, args, 'pad')
    segy_cli.say_target(in_path, target, args, say)
    segy_cli.remove_existing(target, say)                                            # the padded file is written anew, not copied

    segy = SegyFile(in_path)
    recording_delays = header_words(segy, args.byte_delay)
    ndelays = len(np.unique(recording_delays))
    if ndelays <= 1:
        return False
    say(f'Found < {ndelays} > different "DelayRecordingTimes" for file < {os.path.basename(in_path)} >', kind='info')
    dt, ns = segy.dt, segy.ns
    twt = (np.arange(ns) * dt) + int(segy.header('DelayRecordingTime')[0])           # TWT of the samples [ms], from the first trace's delay
    section = segy.traces()                                                          # [ntr][ns]: the kernels' layout
    del segy

    padded, _, n_samples_padded, (_, min_delay, _) = pad_trace_data(section, recording_delays, section.shape[0], dt, twt, trace_major=True)
    if n_samples_padded > 65535:
        raise ValueError(f'{n_samples_padded} padded samples per trace do not fit the 16-bit sample count of the SEG-Y headers (at most 65535)')
    say(f'Writing padded output file < {os.path.basename(target)} >', kind='info')
    write_resized(in_path, target, padded, fields={'DelayRecordingTime': int(min_delay)})
    text = add_processing_info_header(get_textual_header(target), f'PAD DELRT (byte:{BYTE_DELRT})', prefix='_TODAY_')
    write_textual_header(target, text)
    return target


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    segy_cli.run(__file__, args, lambda path: wrapper_delrt_padding_segy(path, args), skipped=MSG_SKIPPED,
                 summary='Padded a total of < {done} > out of < {total} > files')


if __name__ == '__main__':
    main()
