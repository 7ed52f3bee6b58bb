"""
Step 7 -- compensate the mistie of crossing SEG-Y profiles on the GPU, mirror of ``pseudo_3D_interpolation/mistie_correction_segy.py``.

The survey's 2-D lines are intersected (shot-point segments against shot-point segments), the trace of either line nearest to every
crossing is found, the two (envelope) traces are cross-correlated over their common time window, and one vertical offset per line is
solved from the crossings' misties by least squares (Bishop & Nunns, 1994).  Crossings, nearest shot points and correlations run on the
device (HIP unit ``p3d_mistie``, ``functions/mistie.py``); every file is then copied and its samples shifted by its line's offset on the
device, in the file's own sample format.

Flags, defaults, output naming (``<name>_mistie.<ext>`` or ``--txt_suffix``, ``--inplace``, ``--output_dir``, the input directory when
neither is given), the two kinds of input (a directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file, the auxiliary
``*.mst`` file and the ``MISTIE`` line of the textual header are the reference's.  Departures: an offset reaches its file
through the file's line name, not through the file's position in the list; the QC output is a CSV table of the intersections (GeoPackage
layers need geopandas); the navigation tables are read without pandas.
"""
import argparse
import csv
import datetime
import glob
import os
import sys
from functools import partial

import numpy as np

from .functions import segy_cli
from .functions.header import add_processing_info_header, get_textual_header, write_textual_header
from .functions.mistie import compensate_mistie, compute_misties, find_intersections, line_key, nearest_intersection_vertices
from .functions.segy import SegyFile, scaled_coordinates, update_samples
from .functions.utils import xprint

QC_COLUMNS = ['x', 'y', 'line_0', 'dist_0', 'x_0', 'y_0', 'line_1', 'dist_1', 'x_1', 'y_1']
MST_HEADER = 'tracl,tracr,fldr,mistie_samples,mistie_ms\n'


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Compensate mistie for SEG-Y file(s) via cross-correlation of nearest traces of intersecting lines.')
    parser.add_argument('input_path', type=str, help='Input datalist or directory.')
    parser.add_argument('--output_dir', '-o', type=str,
                        help='Output directory for corrected SEG-Y file(s).')
    parser.add_argument('--inplace', '-i', action='store_true',
                        help='Edit SEG-Y file(s) inplace.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Only used when "input_path" is a directory.')
    parser.add_argument('--suffix', '-s', type=str, default='sgy',
                        help='File suffix. Only used when "input_path" is a directory.')
    parser.add_argument('--txt_suffix', type=str, help='Additional text to append to output filename.')
    #
    parser.add_argument('--coords_origin', choices=['header', 'aux'], default='header',
                        help='Origin of (shotpoint) coordinates (i.e. navigation).')
    parser.add_argument('--coords_path', type=str, required=True,
                        help='Path to SEG-Y directory (coords_origin=header) or navigation file with coordinates (coords_origin=aux).')
    parser.add_argument('--coords_fsuffix', type=str,
                        help='File suffix of auxiliary or SEG-Y files (depending on chosen parameter for `coords_origin`.')
    parser.add_argument('--coords_text_suffix', type=str,
                        help='Filename text suffix to filter auxiliary or SEG-Y files.')
    #
    parser.add_argument('--win_cc', nargs='*',
                        help='Upper/lower trace window limits used for cross-correlation (in ms).')
    parser.add_argument('--quality_threshold', type=float, default=0.5,
                        help='Cut-off threshold for cross-correlation [0-1].')
    parser.add_argument('--write_aux', action='store_true',
                        help='Write mistie offsets to auxiliary file (*.mst).')
    parser.add_argument('--write_QC', action='store_true',
                        help='Write line intersections and nearest traces to GeoPackage (*.gpkg).')
    parser.add_argument('--verbose', '-V', type=int, nargs='?',
                        default=0, const=1, choices=[0, 1, 2],
                        help='Level of output verbosity.')
    return parser
# fmt: on


def navigation_files(path, fsuffix, text_suffix):
    """The files that carry the navigation: ``*.{fsuffix}`` of a directory (sorted; ``text_suffix``: the base name must end with it), or the
    entries of a ``.txt`` list with their extension replaced by ``fsuffix`` (names relative to the list)."""
    fsuffix = fsuffix if fsuffix.startswith('.') else '.' + fsuffix
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, f'*{fsuffix}')))
        if text_suffix is not None:
            files = [f for f in files if os.path.splitext(os.path.basename(f))[0].endswith(text_suffix)]
        return files
    if os.path.isfile(path) and path.endswith('.txt'):
        folder = os.path.dirname(path)
        with open(path) as fh:
            entries = [ln.strip() for ln in fh if ln.strip()]
        return [os.path.join(folder, os.path.splitext(e)[0] + fsuffix) for e in entries]
    raise IOError('Invalid input for `path` parameter. Should be either directory or datalist!')


def read_nav_table(path):
    """x / y columns of a ``*.nav`` table (comma-separated with a header line, the reference's ``export_coords``) as float64 [n, 2]."""
    with open(path, newline='') as fh:
        rows = list(csv.reader(fh))
    if not rows or 'x' not in rows[0] or 'y' not in rows[0]:
        raise ValueError(f'{path}: a navigation table needs the columns x and y')
    ix, iy = rows[0].index('x'), rows[0].index('y')
    return np.array([[float(r[ix]), float(r[iy])] for r in rows[1:] if r], dtype=np.float64).reshape(-1, 2)


def load_navigation(args, say):
    """{line name: shot points [n, 2]} in the order of the (sorted) navigation files, from the trace headers (source X / Y at bytes 73 / 77
    with the scalar at byte 71) or from ``*.nav`` tables."""
    nav = {}
    if args.coords_origin == 'aux':
        fsuffix = args.coords_fsuffix if args.coords_fsuffix is not None else 'nav'
        say(f'Load navigation from auxiliary files (*.{fsuffix})', kind='info')
        for path in navigation_files(args.coords_path, fsuffix, args.coords_text_suffix):
            nav.setdefault(line_key(path), []).append(read_nav_table(path))
    else:
        fsuffix = args.suffix if args.suffix is not None else 'sgy'
        say('Extract and load navigation from headers of SEG-Y files', kind='info')
        for path in navigation_files(args.coords_path, fsuffix, args.coords_text_suffix):
            segy = SegyFile(path)
            x, y = scaled_coordinates(segy.header('SourceGroupScalar'), segy.header('SourceX'), segy.header('SourceY'))
            nav.setdefault(line_key(path), []).append(np.stack([x, y], axis=1))
    if not nav:
        raise FileNotFoundError(f'No navigation found in > {args.coords_path} <')
    return {key: np.concatenate(parts) for key, parts in nav.items()}


def correlation_window_argument(win_cc):
    if win_cc is None:
        return (False, False)
    if len(win_cc) < 2:
        raise ValueError('`win_cc` takes the upper and the lower window limit (in ms)')
    upper, lower = sorted((float(win_cc[0]), float(win_cc[1])))
    return (upper, lower)


def main_misties(args, files, say):
    """Offsets of the files' lines.  Returns ``{line name: (offset in samples, offset in ms)}`` and the residuals of the least squares."""
    if args.quality_threshold < 0 or args.quality_threshold > 1:
        raise ValueError('`quality_threshold` must be float in range [0-1]')
    nav = load_navigation(args, say)
    lookup = {}
    for path in files:
        lookup.setdefault(line_key(path), os.path.basename(path))
    unused = [key for key in nav if key not in lookup]
    if unused:
        say(f'Navigation without corresponding SEG-Y is left out: {unused}', kind='warning')
    lines = [key for key in nav if key in lookup]
    missing = [key for key in lookup if key not in nav]
    if missing:
        say(f'SEG-Y without navigation stays as it is: {missing}', kind='warning')
    if len(lines) < 2:
        raise ValueError('at least two lines with navigation and SEG-Y file are needed')
    lookup_lines = {key: lookup[key] for key in lines}
    pts_split = [nav[key] for key in lines]

    xy, line_idx, _ = find_intersections(pts_split, return_segments=True)
    say(f'Found < {xy.shape[0]} > intersections of < {len(lines)} > lines', kind='info')
    names = np.array(lines, dtype=object)[line_idx]
    index, dist = nearest_intersection_vertices(pts_split, xy, line_idx)
    (offsets, residuals), offsets_ms, _ = compute_misties(os.path.dirname(files[0]), names, line_idx, index[:, 0], index[:, 1],
                                                          win=correlation_window_argument(args.win_cc), quality=args.quality_threshold,
                                                          lookup_df=lookup_lines, lookup_col='line', check_bad_traces=True, ntraces2mix=3,
                                                          return_ms=True, return_coeff=True, verbosity=args.verbose)
    if args.write_QC:
        write_intersections_QC(args, pts_split, line_idx, names, index, dist, xy, say)
    return {key: (int(offsets[k]), float(offsets_ms[k])) for k, key in enumerate(lines)}, residuals


def write_intersections_QC(args, pts_split, line_idx, names, index, dist, xy, say):
    """The reference's 'intersections' layer as ``<date>_QC_<dir>_intersections.csv``: the point, and per line its name, the distance to the
    nearest shot point and that shot point."""
    say('GeoPackage output needs geopandas: the intersections are written as a CSV table', kind='warning')
    work_dir = args.output_dir if args.output_dir is not None else os.path.dirname(args.input_path)
    path = os.path.join(work_dir, f'{datetime.date.today().isoformat()}_QC_{os.path.basename(work_dir)}_intersections.csv')
    with open(path, 'w', newline='\n') as fh:
        fh.write(','.join(QC_COLUMNS) + '\n')
        for c in range(xy.shape[0]):
            row = [repr(float(xy[c, 0])), repr(float(xy[c, 1]))]
            for side in range(2):
                shot = pts_split[int(line_idx[c, side])][int(index[c, side])]
                row += [str(names[c, side]), repr(float(dist[c, side])), repr(float(shot[0])), repr(float(shot[1]))]
            fh.write(','.join(row) + '\n')
    return path


def wrapper_mistie_correction_segy(in_path, offset, offset_ms, args):
    """Shift one SEG-Y file (or its copy) by its line's offset."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    path, out_dir, out_name = segy_cli.copied_target(in_path, args, 'mistie', say)

    segy = SegyFile(path)
    say(f'n_traces:  {segy.ntraces}', kind='debug')
    say(f'n_samples: {segy.ns}', kind='debug')
    say(f'dt:        {segy.dt}', kind='debug')
    tracl, tracr, fldr = (segy.header(k) for k in ('TRACE_SEQUENCE_LINE', 'TRACE_SEQUENCE_FILE', 'FieldRecord'))
    section = segy.traces()                                     # [ntr][ns]: the kernel's layout
    del segy                                                    # the read-only map goes before the file is rewritten
    say('Apply mistie compensation', kind='info')
    corrected = compensate_mistie(section, offset, verbosity=args.verbose, trace_major=True)
    say('Writing compensated data to disk', kind='info')
    update_samples(path, corrected)
    write_textual_header(path, add_processing_info_header(get_textual_header(path), 'MISTIE', prefix='_TODAY_', newline=True))

    if args.write_aux:
        say(f'Creating auxiliary file < {out_name}.mst >', kind='info')
        with open(os.path.join(out_dir, f'{out_name}.mst'), 'w', newline='\n') as fout:
            fout.write(MST_HEADER)
            for i in range(len(tracr)):
                fout.write(f'{tracl[i]},{tracr[i]},{fldr[i]},' + f'{offset},{offset_ms:.2f}\n')
    return path


def main(argv=sys.argv):  # noqa
    args = define_input_args().parse_args(argv[1:])
    say = partial(xprint, verbosity=args.verbose)
    say(args, kind='debug')

    # not `segy_cli.run`: one file is refused, and the offsets of all lines are solved between listing the files and the logged loop
    files, folder, single = segy_cli.input_files(args.input_path, args)
    if single:
        raise FileNotFoundError('Invalid input file')          # a directory or a .txt datalist: one line has nothing to tie to
    if not files:
        sys.exit(segy_cli.MSG_NO_FILES)
    offsets, _ = main_misties(args, files, say)
    segy_cli.process_list(__file__, folder, files, args,
                          lambda path: wrapper_mistie_correction_segy(path, *offsets.get(line_key(path), (0, 0.0)), args))


if __name__ == '__main__':
    main()
