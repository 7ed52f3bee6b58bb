"""
Step 16 -- write a 3-D cube (``.nc`` / ``.npz``) as a 3-D SEG-Y file on the GPU, mirror of ``pseudo_3D_interpolation/cube_cnv_netcdf2segy_3D.py``.

The reference hands the cube to segysak's writer; here the records are coded on the device (HIP unit ``p3d_segy``, ``functions/segy_gpu.py``): the
cube goes in as it is stored, ('iline', 'xline', 'twt') or ('twt', 'iline', 'xline'), whole inlines at a time, and comes out as records of a
240-byte header and IBM (``--format 1``, the default) or IEEE (``--format 5``) samples, one trace per (iline, xline) in C order.

Per-trace header words (1-based bytes): TRACE_SEQUENCE_LINE (1), TRACE_SEQUENCE_FILE (5) and CDP (21) = 1 ... n; NStackedTraces (33) = ``fold``;
SourceGroupScalar (71) = the coordinate scalar; CDP_X (181) / CDP_Y (185) = rint(x * factor), rint(y * factor) from the cube's 2-D ``x`` / ``y``
(``functions.header.check_coordinate_scalar``); INLINE_3D (189) / CROSSLINE_3D (193) from the coordinates; DelayRecordingTime (109) = the first
``twt`` in ms where it fits 16 bits; TRACE_SAMPLE_COUNT (115) and TRACE_SAMPLE_INTERVAL (117, microseconds).  Binary header: interval, sample
count, format and revision as ``segy.write_segy`` sets them, the original interval (3219) = int(dt_original * 1000) or 0, the sorting code
(3229) = 2 (the reference's INLINE_SORTING) and the measurement system (3255) = 1 for 'm'.  The textual header holds the reference's 40 cards.
"""
import argparse
import datetime
import getpass
import os
import sys
from functools import partial

import numpy as np
import yaml

from .cube_io import open_cube
from .functions.header import check_coordinate_scalar
from .functions.segy_gpu import CHUNK_BYTES, FIELDS, write_cube_segy
from .functions.utils import xprint

SCALARS = [-1000, -100, -10, 0, 10, 100, 1000, 'auto']
AUX_DEFAULT = ['fold', 'ref_amp']
CARD_TEXT = 75                                                     # characters of a card the reference fills behind 'Cnn '
MEASUREMENT_SYSTEM = {'m': 1, 'ft': 2}
SORTING_INLINE = 2


def _scalar(text):
    return text if text == 'auto' else int(text)


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(
        description='Convert 3D cube from netCDF to SEG-Y file format.')
    parser.add_argument('path_cube', type=str, help='Input path of 3D cube')
    parser.add_argument('--params_netcdf', type=str, required=True,
                        help='Path of netCDF parameter file (YAML format).')
    parser.add_argument('--path_segy', type=str, help='Output SEG-Y file path.')
    parser.add_argument('--scalar_coords', type=_scalar, default='auto', choices=SCALARS,
                        help='Coordinate scalar for SEG-Y trace header.')
    parser.add_argument('--format', type=int, default=1, choices=[1, 5],
                        help='Sample format of the SEG-Y file: 1 (IBM float, default) or 5 (IEEE float).')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, const=1, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0)')
    return parser
# fmt: on


def user_name():
    """The login name for the EVOKER card; without a controlling terminal ``os.getlogin`` fails and ``getpass.getuser`` answers."""
    try:
        return os.getlogin()
    except OSError:
        return getpass.getuser()


def textual_header(timestamp, user, factor, processing_text=None):
    """The 40 cards of the reference as one string of 3200 characters: title, creation time, user, the cube's processing lines from card 11 on
    (they overwrite later cards where there are many, as there), the byte locations of the key header words and the end card."""
    cards = {
        1: '3D SEG-Y CONVERTED FROM NETCDF USING PSEUDO_3D_INTERPOLATION_AMD',
        3: f'CREATION: {timestamp}',
        4: f'EVOKER: {user}',
        10: '*** PROCESSING STEPS ***',
        35: '*** BYTE LOCATION OF KEY HEADERS ***',
        36: f"CDP: {FIELDS['CDP'][0]}  FOLD: {FIELDS['NStackedTraces'][0]}",
        37: f"CDP UTM-X: {FIELDS['CDP_X'][0]} CDP UTM-Y: {FIELDS['CDP_Y'][0]} ALL COORDS SCALED BY: {factor}",
        38: f"INLINE: {FIELDS['INLINE_3D'][0]}, XLINE: {FIELDS['CROSSLINE_3D'][0]}",
        40: 'END TEXTUAL HEADER',
    }
    if processing_text:
        cards.update(zip(range(11, 41), processing_text.split('\n')))
    return ''.join(f'C{k:02d} {cards.get(k, "")[:CARD_TEXT]:<76}' for k in range(1, 41))


def trace_headers(iline, xline, x, y, scalar, factor, fold, twt, dt_ms):
    """The header words of every trace of the cube (names of ``functions.segy_gpu.FIELDS``): arrays of nil * nxl values in C order over
    (iline, xline) and scalars for the words all traces share."""
    nil, nxl, ns = len(iline), len(xline), len(twt)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != (nil, nxl) or y.shape != (nil, nxl):
        raise ValueError(f'x / y of shape {x.shape} / {y.shape} for a cube of {nil} x {nxl} traces')
    for name, c in (('iline', iline), ('xline', xline)):
        if np.any(np.asarray(c) != np.rint(c)):
            raise ValueError(f'{name} numbers must be integers for the SEG-Y trace headers')
    seq = np.arange(1, nil * nxl + 1)
    words = {'TRACE_SEQUENCE_LINE': seq, 'TRACE_SEQUENCE_FILE': seq, 'CDP': seq, 'SourceGroupScalar': int(scalar),
             'CDP_X': np.rint(x * factor).ravel(), 'CDP_Y': np.rint(y * factor).ravel(),
             'INLINE_3D': np.repeat(np.rint(iline).astype(np.int64), nxl), 'CROSSLINE_3D': np.tile(np.rint(xline).astype(np.int64), nil),
             'TRACE_SAMPLE_COUNT': ns, 'TRACE_SAMPLE_INTERVAL': int(round(dt_ms * 1000))}
    if fold is not None:
        words['NStackedTraces'] = np.asarray(fold).reshape(-1).astype(np.int64)
    delay = int(round(float(twt[0]))) if ns else 0
    if -32768 <= delay <= 32767:
        words['DelayRecordingTime'] = delay
    return words


def sample_interval(cube, twt):
    """``dt`` of the twt axis in ms: its attribute, else the mean step cut to microseconds as the reference does."""
    dt = cube.coord_attrs.get('twt', {}).get('dt')
    return float(dt) if dt is not None else int(float(np.mean(np.diff(twt))) * 1000) / 1000


def main(argv=sys.argv):  # noqa
    """Convert `netCDF` cube to `SEG-Y` format."""
    timestamp = datetime.datetime.now().isoformat(timespec='seconds')
    args = define_input_args().parse_args(argv[1:])
    say = partial(xprint, verbosity=args.verbose)
    path_cube = args.path_cube
    path_segy = args.path_segy if args.path_segy is not None else os.path.splitext(path_cube)[0] + '.sgy'
    with open(args.params_netcdf, 'r') as fh:
        kwargs_nc = yaml.safe_load(fh) or {}
    aux = list(kwargs_nc.get('var_aux', AUX_DEFAULT)) + ['x', 'y']

    say('Open 3D cube', kind='info')
    cube = open_cube(path_cube)
    var = next((v for v in cube.data_vars if v not in aux), None)
    if var is None:
        raise ValueError(f'{path_cube}: no data variable beside {aux}')
    dims = tuple(cube.dims[var])
    data = np.asarray(cube.data_vars[var])
    if data.dtype != np.float32:
        data = data.astype(np.float32)
    x, y = (cube.data_vars[k] if k in cube.data_vars else cube.coords.get(k) for k in ('x', 'y'))
    if x is None or y is None:
        raise ValueError(f'{path_cube}: the cube needs the 2-D bin centre coordinates `x` and `y`')
    iline, xline, twt = cube.coords['iline'], cube.coords['xline'], np.asarray(cube.coords['twt'], np.float64)

    scalar, factor = check_coordinate_scalar(args.scalar_coords, xcoords=np.asarray(x), ycoords=np.asarray(y))
    dt_ms = sample_interval(cube, twt)
    dto = cube.coord_attrs.get('twt', {}).get('dt_original')
    binary = {'IntervalOriginal': int(dto * 1000) if dto is not None else 0, 'SortingCode': SORTING_INLINE,
              'MeasurementSystem': MEASUREMENT_SYSTEM.get(cube.attrs.get('measurement_system', 'm'), 0)}
    words = trace_headers(iline, xline, x, y, scalar, factor, cube.data_vars.get('fold'), twt, dt_ms)
    text = textual_header(timestamp, user_name(), factor, cube.attrs.get('text'))

    say(f'Write < {var} > {dims} of shape {data.shape} to < {os.path.basename(path_segy)} > (format {args.format}, coordinate scalar {scalar})', kind='info')
    write_cube_segy(path_segy, data, dims, words, dt_ms, fmt=args.format, text=text, binary=binary, chunk_bytes=CHUNK_BYTES)
    say('Finished conversion to SEG-Y', kind='success')
    return path_segy


if __name__ == '__main__':
    main()
