"""
Step 1 -- merge short SEG-Y file(s) with the neighbouring ones on the GPU, mirror of ``pseudo_3D_interpolation/merge_segys.py``.

Files smaller than ``--filesize_kB`` are merged with the files recorded next to them: every run of consecutive small files together with
the file that follows it (`functions.merge.files_to_merge`).  Within a group duplicate traces are dropped, the traces are put in the order of
TRACE_SEQUENCE_LINE, missing traces are filled with zero traces whose header words are interpolated linearly, and TRACE_SEQUENCE_FILE is
renumbered (`functions.merge.merge_segys`; fingerprints, gather and gap headers on the device, HIP unit ``p3d_merge``).  The output
``<first file>_<txt_suffix>.<ext>`` lies beside the first file of the group, with ``<first file>_<txt_suffix>.parts`` listing what went into it.

Flags and defaults are the reference's.  Its ``main()`` does not run as shipped (it reads ``args.input_dir``, which the parser does not
define); here the input is a directory (its files sorted by name) or a ``.txt`` list (in the listed order), ``--filesize_kB`` and
``--txt_suffix`` are passed on (the reference drops both), a single SEG-Y file is refused with a message, and no small file among the input
is an info message and a normal exit.  One log ``<stamp>_merge_segys.log`` goes into the input folder.
"""
import argparse
import os
import sys
from contextlib import redirect_stdout
from functools import partial

from .functions import segy_cli
from .functions.merge import files_to_merge, merge_segys
from .functions.utils import xprint

MSG_SINGLE = 'A single SEG-Y file cannot be merged: "input_path" must be a directory or a datalist (.txt).'
MSG_NOTHING = 'No file is smaller than the given file size: nothing to merge.'


def define_input_args():
    """The reference's flags, defaults and choices; the texts are this package's."""
    parser = argparse.ArgumentParser(description='Merge SEG-Y files below a size threshold with the file recorded after them (step 1, GPU).')
    parser.add_argument('input_path', type=str, help='A directory of SEG-Y files (taken sorted by name) or a .txt list of files (taken in its order).')
    parser.add_argument('--filename_suffix', '-fns', type=str, default='',
                        help='With a directory: take only files whose name ends in this text before the extension.')
    parser.add_argument('--suffix', '-s', type=str, default='sgy', help='With a directory: the extension of the files to take (default: sgy).')
    parser.add_argument('--txt_suffix', type=str, default='merge', help='Appended to the name of the first file of a group to name the merged file (default: merge).')
    parser.add_argument('--filesize_kB', type=float, default=2000,
                        help='A file smaller than this many kB (1024 bytes) counts as short and is merged (default: 2000).')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, choices=[0, 1, 2], help='0: warnings only, 1: progress, 2: every step (default: 0).')
    return parser


def main(argv=sys.argv):  # noqa
    """Merge small SEG-Y files with others."""
    args = define_input_args().parse_args(argv[1:])
    say = partial(xprint, verbosity=args.verbose)
    files, folder, single = segy_cli.input_files(args.input_path, args)
    if single:
        sys.exit(MSG_SINGLE)
    if not files:
        sys.exit(segy_cli.MSG_NO_FILES)

    log_path = os.path.join(folder, f'{segy_cli.time_stamp()}_{segy_cli.script_name(__file__)}.log')
    try:
        with open(log_path, 'w', newline='\n') as log, redirect_stdout(log):
            groups = files_to_merge(files, fsize_kB=args.filesize_kB, verbosity=args.verbose)
            if not groups:
                xprint(MSG_NOTHING, kind='info', verbosity=max(args.verbose, 1))
                return
            say(f'Processing total of < {len(groups)} > files', kind='info')
            for k, group in enumerate(groups):
                say(f'Merging {k + 1}th set of files', kind='info')
                merge_segys(group, txt_suffix=args.txt_suffix, verbosity=args.verbose)
    finally:
        segy_cli.clean_log_file(log_path)


if __name__ == '__main__':
    main()
