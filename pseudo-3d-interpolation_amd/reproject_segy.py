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
import os
import sys
from functools import partial

from .functions import crs as C
from .functions import segy_cli
from .functions.filter import smooth
from .functions.header import (COORDS, MSG_FORCED, TRACE_HEADER_COORDS, add_processing_info_header, get_textual_header, scale_coordinates,
                               unscale_coordinates, write_textual_header)
from .functions.segy import SegyFile, field_at, update_headers
from .functions.utils import xprint

MSG_GEOGRAPHIC_DST = 'Functionality to convert to geographic output CRS is not yet implemented.'

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


def wrapper_reproject_segy(in_path, src_coords_bytes, dst_coords_bytes, args):
    """Reproject the header coordinates of one SEG-Y file; returns the path of the file that was written."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    crs_src, crs_dst = C.parse_crs(args.crs_src), C.parse_crs(args.crs_dst)
    if crs_dst.is_geographic:
        raise NotImplementedError(MSG_GEOGRAPHIC_DST)
    path, _, _ = segy_cli.copied_target(in_path, args, 'reproj', say)

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
    args = define_input_args().parse_args(argv[1:])
    xprint(args, kind='debug', verbosity=args.verbose)
    src_coords_bytes, dst_coords_bytes = TRACE_HEADER_COORDS[args.src_coords], TRACE_HEADER_COORDS[args.dst_coords]
    segy_cli.run(__file__, args, lambda path: wrapper_reproject_segy(path, src_coords_bytes, dst_coords_bytes, args))


if __name__ == '__main__':
    main()
