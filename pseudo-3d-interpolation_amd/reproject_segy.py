"""
Step 2 -- reproject the trace-header coordinates of SEG-Y profile(s) on the GPU, mirror of ``pseudo_3D_interpolation/reproject_segy.py``.

The coordinates at ``--src_coords`` are scaled as the first trace's ``CoordinateUnits`` and ``SourceGroupScalar`` say (length: the scalar; seconds
of arc: divided by 3 600 000), transformed from ``--crs_src`` to ``--crs_dst`` (``functions/crs.py``: transverse Mercator in double precision, HIP
unit ``p3d_proj``), optionally smoothed along the profile (``--smooth``, ``functions/filter.smooth``) and written as integers with ``--scalar_coords``
to ``--dst_coords``, together with ``CoordinateUnits`` = 1 and ``SourceGroupScalar`` = the scalar in every trace.  The textual header gets
``CRS (PROJECTED): EPSG:<code>`` and a dated ``REPROJECT (BYTES:x y)[ SMOOTHED]`` line.

Flags, defaults, output naming (``<name>_reproj.<ext>`` or ``--txt_suffix``, ``--inplace``, ``--output_dir``), the three kinds of input (a file, a
directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file and the messages are the reference's.  The reference takes the
transformation from pyproj; here the set of coordinate reference systems is the one ``functions/crs.py`` lists (UTM on WGS84 / ETRS89 and
``+proj=tmerc`` strings; no EPSG database, no datum shifts).  Departure: both CRS are parsed, and a geographic ``--crs_dst`` is
refused, before the output copy is made (the reference leaves an unchanged copy behind when it raises).
"""
import argparse
import datetime
import os
import sys
from contextlib import redirect_stdout
from functools import partial
from shutil import copy2

import numpy as np

from .despiking_2D_segy import clean_log_file, input_files
from .functions import crs as C
from .functions.filter import smooth
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.segy import TRACE_FIELDS, SegyFile, update_headers
from .functions.utils import xprint

TRACE_HEADER_COORDS = {'source': (73, 77), 'CDP': (181, 185), 'group': (81, 85)}
ARC_SECONDS = 3600000
MSG_FORCED = 'Forced source CRS to be geographic (WGS84 - EPSG:4326)!'
MSG_GEOGRAPHIC_DST = 'Functionality to convert to geographic output CRS is not yet implemented.'


COORDS = ['source', 'CDP', 'group']
# (names, keywords) per argument, in the reference's order; the help texts are the reference's, so that `--help` reads the same
ARGUMENTS = [
    (('input_path',), dict(type=str, help='Input file or directory.')),
    (('--crs_src',), dict(type=str, required=True, help='Source CRS of SEG-Y file(s). Indicate using EPSG code or PROJ.4 string.')),
    (('--crs_dst',), dict(type=str, required=True, help='Destination CRS of SEG-Y file(s). Indicate using EPSG code or PROJ.4 string.')),
    (('--output_dir', '-o'), dict(type=str, help='Output directory for reprojected SEG-Y file(s).')),
    (('--inplace', '-i'), dict(action='store_true', help='Edit SEG-Y file(s) inplace.')),
    (('--filename_suffix', '-fns'), dict(type=str, help='Filename suffix for guided selection (e.g. "env" or "despk"). '
                                                        'Only used when "input_path" is a directory.')),
    (('--suffix', '-s'), dict(type=str, help='File suffix. Only used when "input_path" is a directory.')),
    (('--txt_suffix',), dict(type=str, help='Additional text to append to output filename.')),
    (('--scalar_coords', '-sc'), dict(type=int, default=-100, choices=[-1000, -100, -10, 0, 10, 100, 1000],
                                      help='Output coordinate scalar.\n' + ' ' * 28 + 'Negative: division by absolute value,\n'
                                           + ' ' * 28 + 'positive: multiplication by absolute value.')),
    (('--src_coords',), dict(type=str, choices=COORDS, default='source', help='Byte position of input coordinates in SEG-Y file(s).')),
    (('--dst_coords',), dict(type=str, choices=COORDS, default='source', help='Byte position of output coordinates in SEG-Y file(s).')),
    (('--smooth',), dict(type=int, nargs='?', default=None, const=11, help='Smooth coordinates using window of size `k` traces (default: 11).')),
    (('--verbose', '-V'), dict(type=int, nargs='?', default=0, const=1, choices=[0, 1, 2], help='Level of output verbosity (default: 0).')),
]


def define_input_args():
    parser = argparse.ArgumentParser(description='Coordinate transformation for SEG-Y file(s).')
    for names, keywords in ARGUMENTS:
        parser.add_argument(*names, **keywords)
    return parser


def field_at(byte):
    """Name of the reader's trace-header field that starts at 1-based ``byte``."""
    for name, (b, _) in TRACE_FIELDS.items():
        if b == byte:
            return name
    raise KeyError(f'no trace-header field at byte {byte}')


def scale_coordinates(segy, src_coords_bytes=(73, 77)):
    """(x, y, CoordinateUnits): the header coordinates at ``src_coords_bytes`` in their real unit.  The FIRST trace decides for all: units 1
    (length) apply its ``SourceGroupScalar`` (negative: divide by its magnitude, positive: multiply, 0: as stored), units 2 (seconds of arc)
    divide by 3 600 000; units 3 and 4 are not implemented (reference: functions/header.py ``scale_coordinates``)."""
    units = int(segy.header('CoordinateUnits')[0])
    x, y = segy.header(field_at(src_coords_bytes[0])), segy.header(field_at(src_coords_bytes[1]))
    if units == 1:
        scalar = int(segy.header('SourceGroupScalar')[0])
        if scalar < 0:
            x, y = x / np.abs(scalar), y / np.abs(scalar)
        elif scalar > 0:
            x, y = x * np.abs(scalar), y * np.abs(scalar)
    elif units == 2:
        x, y = x / ARC_SECONDS, y / ARC_SECONDS
    elif units == 3:
        raise NotImplementedError('Functionality to convert DD data is not implemented.')
    elif units == 4:
        raise NotImplementedError('Functionality to convert DMS data is not implemented.')
    return x, y, units


def unscale_coordinates(x, y, scale_factor=-100):
    """Coordinates in metres as the integers of a header with scalar ``scale_factor``: rounded ``v * |scalar|`` for a negative scalar,
    rounded ``v / |scalar|`` for a positive one, rounded ``v`` for 0 (reference: functions/header.py ``unscale_coordinates``, units 1)."""
    x, y = np.asarray(x), np.asarray(y)
    if scale_factor < 0:
        x, y = x * np.abs(scale_factor), y * np.abs(scale_factor)
    elif scale_factor > 0:
        x, y = x / np.abs(scale_factor), y / np.abs(scale_factor)
    return np.around(x, 0).astype(np.int64), np.around(y, 0).astype(np.int64)


def output_target(in_path, args, say):
    """Path of the file that is edited; the copy is made here."""
    folder, name = os.path.split(in_path)
    stem, ext = os.path.splitext(name)
    if args.inplace:                                            # supersedes any --output_dir
        say('Updating SEG-Y inplace', kind='warning')
        return in_path
    if args.output_dir is None:
        say('Creating copy of file in INPUT directory:\n', folder, kind='info')
    elif os.path.isdir(args.output_dir):
        say('Creating copy of file in OUTPUT directory:\n', args.output_dir, kind='info')
        folder = args.output_dir
    else:
        raise FileNotFoundError(f'The output directory > {args.output_dir} < does not exist')
    target = os.path.join(folder, f"{stem}_{'reproj' if args.txt_suffix is None else args.txt_suffix}{ext}")
    if os.path.isfile(target):
        say('Output file already exists and will be removed!', kind='warning')
        os.remove(target)
    copy2(in_path, target)
    return target


def wrapper_reproject_segy(in_path, src_coords_bytes, dst_coords_bytes, args):
    """Reproject the header coordinates of one SEG-Y file; returns the path of the file that was written."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    crs_src, crs_dst = C.parse_crs(args.crs_src), C.parse_crs(args.crs_dst)
    if crs_dst.is_geographic:
        raise NotImplementedError(MSG_GEOGRAPHIC_DST)
    path = output_target(in_path, args, say)

    segy = SegyFile(path)
    xcoords, ycoords, coordinate_units = scale_coordinates(segy, src_coords_bytes)
    del segy                                                    # the read-only map goes before the file is rewritten
    if coordinate_units != 1 and crs_src.is_projected:
        say(MSG_FORCED, kind='warning')
        crs_src = C.parse_crs('epsg:4326')
    xcoords_t, ycoords_t = C.transform(crs_src, crs_dst, xcoords, ycoords)
    if args.smooth is not None:
        xcoords_t, ycoords_t = smooth(xcoords_t, args.smooth), smooth(ycoords_t, args.smooth)
    x_int, y_int = unscale_coordinates(xcoords_t, ycoords_t, args.scalar_coords)
    update_headers(path, {field_at(dst_coords_bytes[0]): x_int, field_at(dst_coords_bytes[1]): y_int, 'CoordinateUnits': 1,
                          'SourceGroupScalar': args.scalar_coords})

    text = add_processing_info_header(get_textual_header(path), f'EPSG:{crs_dst.to_epsg()}', prefix='CRS (PROJECTED)')
    info = f'REPROJECT (BYTES:{dst_coords_bytes[0]} {dst_coords_bytes[1]})' + (' SMOOTHED' if args.smooth is not None else '')
    write_textual_header(path, add_processing_info_header(text, info, prefix='_TODAY_'))
    return path


def main(argv=sys.argv):  # noqa
    """Reproject the trace-header coordinates of SEG-Y file(s)."""
    stamp = datetime.datetime.now().isoformat(timespec='seconds').replace(':', '')
    script = os.path.splitext(os.path.basename(__file__))[0]
    args = define_input_args().parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)
    src_coords_bytes, dst_coords_bytes = TRACE_HEADER_COORDS[args.src_coords], TRACE_HEADER_COORDS[args.dst_coords]

    files, folder, single = input_files(args.input_path, args)
    if single:
        wrapper_reproject_segy(files[0], src_coords_bytes, dst_coords_bytes, args)
        sys.exit()
    if not files:
        sys.exit('No input files to process. Exit process.')
    log_path = os.path.join(folder, f'{stamp}_{script}.log')
    with open(log_path, 'w', newline='\n') as log, redirect_stdout(log):
        xprint(f'Processing total of < {len(files)} > files', kind='info', verbosity=args.verbose)
        for one in files:
            wrapper_reproject_segy(one, src_coords_bytes, dst_coords_bytes, args)
    clean_log_file(log_path)


if __name__ == '__main__':
    main()
