"""
Step 6 -- compensate the tidal elevation in SEG-Y profile(s) on the GPU, mirror of ``pseudo_3D_interpolation/tide_compensation_segy.py``.

Per file: the header coordinates at ``--src_coords`` are scaled (``functions/header.scale_coordinates``) and brought to geographic degrees
(``functions/crs.transform``), the recording time of every trace is read from the header words 157 ... 165, the tide is predicted at every
position and time from the TPXO9-atlas style model in ``model_dir`` (``functions/tide.tide_predict``: HIP unit ``p3d_tide``), converted to
samples with 1500 m/s and the file's sample interval, and every trace is shifted by its rounded offset (``functions/tide.compensate_tide``).
The samples are written back in the file's own format and the textual header gets a dated ``TIDE COMPENSATION`` line.  ``--write_aux`` writes
``tracl,tracr,fldr,time,tide_m,tide_ms,tide_samples`` per trace to a ``.tid`` file.

Flags, defaults, output naming (``<name>_tide.<ext>`` or ``--txt_suffix``, ``--inplace``, ``--output_dir``), the three kinds of input (a file, a
directory with ``--suffix`` / ``--filename_suffix``, a ``.txt`` list), the log file and the messages are the reference's.  The reference takes
the prediction from tpxo-tide-prediction and the transformation from pyproj; neither is needed here.

Duplicate positions, as in the reference: the positions are made unique with ``np.unique(latlon, axis=0)``, and all traces that share one
position get the tide at the recording time of the FIRST such trace.

Departures: the CRS is parsed, ``--correct_minor`` refused, the recording times checked and the tide predicted BEFORE the output
copy is made, so an invalid time (``ValueError`` naming the first such trace) or a trace on land (NaN tide: ``ValueError`` with the count) leaves
no file behind; ``--write_aux`` with ``--inplace`` writes ``<name>.tid`` beside the file (the reference stops at an undefined name there).
"""
import argparse
import os
import sys
from functools import partial

import numpy as np

from .functions import crs as C
from .functions import segy_cli
from .functions.header import (COORDS, MSG_FORCED, TRACE_HEADER_COORDS, add_processing_info_header, get_textual_header, scale_coordinates,
                               write_textual_header)
from .functions.segy import SegyFile, update_samples
from .functions.tide import CONSTITUENTS, DEFAULT_CONSTITUENTS, MSG_MINOR, compensate_tide, header_times, tide_predict
from .functions.utils import depth2samples, depth2twt, xprint

# (names, keywords) per argument, in the reference's order; the help texts are the reference's, so that `--help` reads the same
ARGUMENTS = [
    (('input_path',), dict(type=str, help='Input file or directory.')),
    (('model_dir',), dict(type=str, help='Input directory of tidal model files.')),
    (('--output_dir', '-o'), dict(type=str, help='Output directory for compensated SEG-Y file(s).')),
    (('--inplace', '-i'), dict(action='store_true', help='Edit SEG-Y file(s) inplace.')),
    (('--suffix', '-s'), dict(type=str, help='File suffix. Only used when "input_path" is a directory.')),
    (('--filename_suffix', '-fns'), dict(type=str, help='Filename suffix for guided selection (e.g. "env" or "despk"). '
                                                        'Only used when "input_path" is a directory.')),
    (('--txt_suffix',), dict(type=str, help='Additional text to append to output filename.')),
    (('--constituents', '-c'), dict(nargs='+', choices=list(CONSTITUENTS), default=list(DEFAULT_CONSTITUENTS),
                                    help='Available tidal constituents supported by TPXO9 atlas model.')),
    (('--correct_minor',), dict(action='store_true', help='Correct for minor tidal constituents.')),
    (('--src_coords',), dict(type=str, choices=COORDS, default='source', help='Byte position of input coordinates in SEG-Y file(s).')),
    (('--crs_src',), dict(type=str, default='epsg:32760', help='Source CRS of SEG-Y file(s). Indicate using EPSG code or PROJ.4 string.')),
    (('--write_aux',), dict(action='store_true', help='Write times and tide predictions to auxiliary file (*.tid).')),
    (('--verbose', '-V'), dict(type=int, nargs='?', default=0, choices=[0, 1, 2], help='Level of output verbosity (default: 0).')),
]
AUX_HEADER = 'tracl,tracr,fldr,time,tide_m,tide_ms,tide_samples\n'


def define_input_args():
    parser = argparse.ArgumentParser(description='Compensate tidal effect for SEG-Y file(s) using TPXO9-atlas-v4 tide model.')
    for names, keywords in ARGUMENTS:
        parser.add_argument(*names, **keywords)
    return parser


def aux_lines(tracl, tracr, fldr, times, tides, dt):
    """The lines of the ``.tid`` file (reference columns and formats); ``dt`` in ms."""
    tides_twt = depth2twt(tides)
    tides_samples = np.around(depth2samples(tides, dt=dt, units='ms'), 0)
    return [f'{tracl[i]},{tracr[i]},{fldr[i]},{np.datetime_as_string(times[i], "s")},{tides[i]:.6f},{tides_twt[i] * 1000:.3f},{tides_samples[i]:.0f}\n'
            for i in range(tides.size)]


def wrapper_tide_compensation(in_path, args):
    """Compensate the tide in one SEG-Y file; returns the path of the file that was written."""
    say = partial(xprint, verbosity=args.verbose)
    say(f'Processing file < {os.path.basename(in_path)} >', kind='info')
    if args.correct_minor:
        raise NotImplementedError(MSG_MINOR)
    crs_src = C.parse_crs(args.crs_src)
    path, folder, _ = segy_cli.output_target(in_path, args, 'tide')               # nothing is copied yet
    segy_cli.say_target(in_path, path, args, say)
    stem = os.path.splitext(os.path.basename(path))[0]                              # of the file that is edited and of its ``.tid`` companion

    segy = SegyFile(in_path)
    dt = segy.dt                                                # sample interval (ms)
    say(f'n_traces:  {segy.ntraces}', kind='debug')
    say(f'n_samples: {segy.ns}', kind='debug')
    say(f'dt:        {dt}', kind='debug')
    tracl, tracr, fldr = segy.header('TRACE_SEQUENCE_LINE'), segy.header('TRACE_SEQUENCE_FILE'), segy.header('FieldRecord')
    say('Reading coordinates from SEG-Y file', kind='debug')
    xcoords, ycoords, coordinate_units = scale_coordinates(segy, TRACE_HEADER_COORDS[args.src_coords])
    if coordinate_units != 1 and crs_src.is_projected:
        say(MSG_FORCED, kind='warning')
        crs_src = C.parse_crs('epsg:4326')
    # geographic degrees on the ellipsoid of the source (no datum shift: ETRS89 and WGS84 agree to well under a cell of any tide model)
    lon, lat = C.transform(crs_src, C.CRS('geographic', crs_src.a, crs_src.f), xcoords, ycoords)
    say('Reading timestamps from SEG-Y file', kind='debug')
    times = header_times(*(segy.header(k) for k in ('YearDataRecorded', 'DayOfYear', 'HourOfDay', 'MinuteOfHour', 'SecondOfMinute')))
    data_src = segy.traces().T                                  # samples x traces
    del segy                                                    # the read-only map goes before the file is rewritten

    # unique positions; traces that share one get the tide at the time of the FIRST of them (the reference's rule)
    latlon_uniq, uniq_idx, uniq_inv = np.unique(np.vstack((lat, lon)).T, axis=0, return_index=True, return_inverse=True)
    uniq_inv = np.ravel(uniq_inv)
    say('Predicting tidal elevation along profile', kind='debug')
    tides_track = tide_predict(args.model_dir, latlon_uniq[:, 0], latlon_uniq[:, 1], times[uniq_idx], args.constituents,
                               correct_minor=args.correct_minor, mode='track')[uniq_inv]
    times = times[uniq_idx][uniq_inv]
    on_land = int(np.isnan(tides_track).sum())
    if on_land:
        raise ValueError(f'{in_path}: {on_land} of {tides_track.size} traces lie where all surrounding nodes of the tide model are dry '
                         '(no tide can be predicted there); nothing was written')
    say('Compensating tide', kind='debug')
    data_comp = compensate_tide(data_src, tides_track, dt, tide_units='meter', units='ms', verbosity=args.verbose)

    say('Writing compensated data to disk', kind='debug')
    segy_cli.copy_to_target(in_path, path, say)
    update_samples(path, data_comp.T)
    write_textual_header(path, add_processing_info_header(get_textual_header(path), 'TIDE COMPENSATION', prefix='_TODAY_', newline=True))

    if args.write_aux:
        say(f'Creating auxiliary file < {stem}.tid >', kind='debug')
        with open(os.path.join(folder, f'{stem}.tid'), 'w', newline='\n') as fout:
            fout.write(AUX_HEADER)
            fout.writelines(aux_lines(tracl, tracr, fldr, times, tides_track, dt))
    return path


def main(argv=sys.argv):  # noqa
    """Compensate the tidal effect in SEG-Y file(s)."""
    args = define_input_args().parse_args(argv[1:])
    if args.verbose is None:                                    # a bare -V (the reference's parser stores None for it)
        args.verbose = 1
    xprint(args, kind='debug', verbosity=args.verbose)
    segy_cli.run(__file__, args, lambda path: wrapper_tide_compensation(path, args))


if __name__ == '__main__':
    main()
