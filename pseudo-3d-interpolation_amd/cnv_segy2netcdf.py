"""
Step 9 -- convert SEG-Y file(s) to netCDF on the GPU, mirror of ``pseudo_3D_interpolation/cnv_segy2netcdf.py`` (which calls segysak's
``segy_converter(cdp=5, cdpx=73, cdpy=77)`` in a process pool).

Every file is read through its memory map and decoded on the device (HIP unit ``p3d_segy``, ``functions/segy_gpu.py``: samples of formats 1, 2,
3, 5 and 8, and the header words below in the same pass), then written as ``<name>.seisnc`` -- netCDF-4 through ``cube_io``'s h5py writer -- or,
with ``--file_type npz``, as ``<name>.npz``.  The ``Cube`` holds ``data`` over ('cdp', 'twt'); the coordinates ``cdp`` (header word 5, the
reference's ``cdp=5``) and ``twt`` (ms, from the DelayRecordingTime of the first trace and the sample interval); ``cdp_x`` / ``cdp_y`` over
('cdp',) from words 73 / 77 scaled by word 71 (``segy.scaled_coordinates``); and the attributes ``sample_rate`` (ms), ``text``, ``source_file``
and ``coord_scalar``.  Files whose traces differ in their delay are converted as they are, with a warning: step 4 (``04_pad_delrt``) puts
them on one time axis.  ``--nprocesses`` is accepted for the reference's command lines and ignored: there is one GPU and the files are
converted in turn.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

from . import cube_io
from .cube_io import Cube
from .functions.backends import h5py_enabled
from .functions.segy import scaled_coordinates
from .functions.segy_cli import input_files
from .functions.segy_gpu import read_segy_gpu
from .functions.utils import xprint

WORDS = ['TRACE_SEQUENCE_FILE', 'SourceGroupScalar', 'SourceX', 'SourceY', 'DelayRecordingTime']
MSG_DELAYS = ('Found < {n} > different "DelayRecordingTime" values in < {name} >: the traces are converted as they are, on the time axis of the '
              'first trace. Pad the file first (step 4, `04_pad_delrt`).')
MSG_NO_H5PY = 'writing `.seisnc` (netCDF-4) needs h5py, which is not installed: use `--file_type npz`'


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Convert SEG-Y files to netCDF format on the GPU.')
    parser.add_argument('path_input', type=str, help='Input datalist or directory.')
    parser.add_argument('--output_dir', '-o', type=str,
                        help='Output directory for created netCDF file(s)')
    parser.add_argument('--suffix', '-s', type=str, default='sgy',
                        help='File suffix. Only used when "path_input" is a directory.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "path_input" is a directory.')
    parser.add_argument('--nprocesses', type=int, default=4,
                        help='Accepted and ignored: the files are converted in turn on one GPU.')
    parser.add_argument('--file_type', type=str, default='nc', choices=['nc', 'npz'],
                        help='Output file type: "nc" (<name>.seisnc, netCDF-4; needs h5py) or "npz" (<name>.npz).')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, const=1, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0)')
    return parser
# fmt: on


def segy_to_cube(path, say=lambda *a, **k: None):
    """One SEG-Y file as a ``Cube`` (see the module text)."""
    samples, words, src = read_segy_gpu(path, WORDS)
    delays = words['DelayRecordingTime']
    ndelays = len(np.unique(delays))
    if ndelays > 1:
        say(MSG_DELAYS.format(n=ndelays, name=os.path.basename(path)), kind='warning')
    twt = (float(delays[0]) if delays.size else 0.0) + np.arange(src.ns) * src.dt
    cdp_x, cdp_y = scaled_coordinates(words['SourceGroupScalar'], words['SourceX'], words['SourceY'])
    attrs = {'sample_rate': src.dt, 'text': src.text, 'source_file': os.path.basename(path),
             'coord_scalar': int(words['SourceGroupScalar'][0]) if src.ntraces else 0}
    return Cube({'data': samples, 'cdp_x': cdp_x, 'cdp_y': cdp_y}, {'data': ('cdp', 'twt'), 'cdp_x': ('cdp',), 'cdp_y': ('cdp',)},
                {'cdp': words['TRACE_SEQUENCE_FILE'], 'twt': twt}, attrs)


def convert(path, dir_out, file_type, say=lambda *a, **k: None):
    """Convert one file; returns the path written."""
    stem = os.path.splitext(os.path.basename(path))[0]
    if file_type == 'nc' and not h5py_enabled:
        raise ImportError(MSG_NO_H5PY)
    cube = segy_to_cube(path, say)
    if file_type == 'npz':
        return cube_io.save_cube(cube, os.path.join(dir_out, stem + '.npz'))
    return cube_io._save_nc_h5py(cube, os.path.join(dir_out, stem + '.seisnc'))


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    say = partial(xprint, verbosity=args.verbose)
    files, folder, single = input_files(args.path_input, args)
    if args.output_dir is None:
        dir_out = folder
    elif os.path.isdir(args.output_dir):
        dir_out = args.output_dir
    else:
        raise ValueError('``--output_dir`` must be an existing directory!')

    if single:
        say('Converting SEG-Y file to netCDF format', kind='info')
        convert(files[0], dir_out, args.file_type, say)
        sys.exit()
    say(f'Converting > {len(files)} < SEG-Y files to netCDF format', kind='info')
    for one in files:
        convert(one, dir_out, args.file_type, say)
    say(f'Finished conversion of > {len(files)} < SEG-Y files!', kind='success')


if __name__ == '__main__':
    main()
