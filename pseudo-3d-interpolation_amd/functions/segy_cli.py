"""What the command lines of the 2-D SEG-Y steps (02 ... 09) share: the three kinds of input, where the output of a file goes, the copy that
is edited, and the run over a list of files with its log.  Nothing here knows a step; the parsers stay with their steps."""
import datetime
import glob
import os
import re
import sys
from contextlib import redirect_stdout
from functools import partial
from shutil import copy2

from .utils import xprint

ANSI_COLOUR = re.compile(r'\x1b\[[0-9;]*m')
MSG_NO_FILES = 'No input files to process. Exit process.'


def time_stamp():
    """Now as ``YYYY-MM-DDTHHMMSS``, the prefix of a run's log file."""
    return datetime.datetime.now().strftime('%Y-%m-%dT%H%M%S')


def script_name(script_file):
    return os.path.splitext(os.path.basename(script_file))[0]


def clean_log_file(path_log, newline='\n'):
    """Strip the terminal colour codes from a log file."""
    with open(path_log) as fh:
        text = fh.read()
    with open(path_log, 'w', newline=newline) as fh:
        fh.write(ANSI_COLOUR.sub('', text))


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


def output_target(in_path, args, tag):
    """(path, folder, name): the file a step writes for ``in_path``, the folder it lies in and ``<stem>_<tag or --txt_suffix>``, the name of
    the output (and of its auxiliary file) without extension.  ``--inplace`` supersedes ``--output_dir`` and makes the path the input itself;
    an ``--output_dir`` that does not exist is an error.  Nothing is written and nothing is said."""
    folder, name = os.path.split(in_path)
    stem, ext = os.path.splitext(name)
    out_name = f'{stem}_{tag if args.txt_suffix is None else args.txt_suffix}'
    if getattr(args, 'inplace', False):
        return in_path, folder, out_name
    if args.output_dir is not None:
        if not os.path.isdir(args.output_dir):
            raise FileNotFoundError(f'The output directory > {args.output_dir} < does not exist')
        folder = args.output_dir
    return os.path.join(folder, out_name + ext), folder, out_name


def say_target(in_path, target, args, say):
    """The reference's message on where the output goes."""
    if target == in_path:
        say('Updating SEG-Y inplace', kind='warning')
    elif args.output_dir is None:
        say('Creating copy of file in INPUT directory:\n', os.path.dirname(target), kind='info')
    else:
        say('Creating copy of file in OUTPUT directory:\n', args.output_dir, kind='info')


def remove_existing(target, say):
    if os.path.isfile(target):
        say('Output file already exists and will be removed!', kind='warning')
        os.remove(target)


def copy_to_target(in_path, target, say):
    """Make ``target`` a fresh copy of ``in_path`` (an existing one is removed with a warning); a file edited in place stays as it is."""
    if target != in_path:
        remove_existing(target, say)
        copy2(in_path, target)


def copied_target(in_path, args, tag, say):
    """`output_target`, said and copied at once, for the steps that edit the copy right away."""
    target, folder, out_name = output_target(in_path, args, tag)
    say_target(in_path, target, args, say)
    copy_to_target(in_path, target, say)
    return target, folder, out_name


def process_list(script_file, folder, files, args, per_file, *, skipped=None, summary=None, catch=False, stamp=None):
    """``per_file(path)`` for every file, with the output in ``<folder>/<stamp>_<script>.log`` (colour codes stripped at the end).

    ``skipped``: the line for a file whose ``per_file`` returned ``False``; ``summary``: a closing line of the log, formatted with ``done`` (the
    files not skipped) and ``total``; ``catch``: a file that raises is logged as 'Failed: ...' and the others are still processed, and the
    number of failures is printed once the log is closed."""
    say = partial(xprint, verbosity=args.verbose)
    log_path = os.path.join(folder, f'{stamp or time_stamp()}_{script_name(script_file)}.log')
    done = failed = 0
    with open(log_path, 'w', newline='\n') as log, redirect_stdout(log):
        say(f'Processing total of < {len(files)} > files', kind='info')
        for one in files:
            try:
                result = per_file(one)
            except Exception as err:  # noqa: BLE001 -- as the reference: a file that fails is logged, the others are still processed
                if not catch:
                    raise
                say(f'Failed: {err}', kind='error')
                failed += 1
                continue
            if result is False and skipped is not None:
                say(skipped, kind='info')
                continue
            done += 1
        if summary is not None:
            say(summary.format(done=done, total=len(files)), kind='info')
    clean_log_file(log_path)
    if catch:
        say(f'>{failed}< out of >{len(files)}< files failed!', kind='info')


def run(script_file, args, per_file, *, skipped=None, summary=None, catch=False, empty=MSG_NO_FILES, stamp=None):
    """The tail of a step's ``main()``: one SEG-Y file is processed on the terminal (``skipped`` as in `process_list`, nothing is caught)
    and the process exits; a directory or a ``.txt`` list goes through `process_list`, or exits with ``empty`` when it names no file."""
    files, folder, single = input_files(args.input_path, args)
    if single:
        if per_file(files[0]) is False and skipped is not None:
            xprint(skipped, kind='info', verbosity=args.verbose)
        sys.exit()
    if not files:
        sys.exit(empty)
    process_list(script_file, folder, files, args, per_file, skipped=skipped, summary=summary, catch=catch, stamp=stamp)
