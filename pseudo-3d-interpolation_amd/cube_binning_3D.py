"""
Step 10 -- bin 2D profiles into a sparse (pseudo-)3D cube on the GPU, mirror of ``pseudo_3D_interpolation/cube_binning_3D.py``.

The cube geometry (rotated inline / xline grid, square or rectangular bins, optional region with a coarser step) and the trace
assignment are computed in NumPy (``functions/binning.py``, ``functions/transform.py``).  The stacking of every bin's traces -- after
aligning them on the global twt axis -- runs on the device (HIP unit ``p3d_binning``, include/p3d.h) with one of four rules:
``average``, ``median``, ``nearest`` or ``IDW`` (inverse distance weighting).  Outputs are the reference's two cubes, written through
``cube_io`` (``.nc`` or ``.npz``): ``{name}_{method}{_attr}_{il}x{xl}m_{dt}ms`` in (iline, xline, twt) order and ``..._twt-il-xl`` in
(twt, iline, xline) order, each with the amplitude variable (``amp``, or ``env`` with ``--attribute env``), ``fold`` (uint8) and the
bin-centre coordinates ``x`` / ``y`` as (iline, xline) variables after the amplitude.

Departures from the reference (fixes, or limits of an environment without pandas / xarray / pyproj / segyio):

* Input: trace samples are read straight from the SEG-Y files (``functions/segy.py``), not from step-09 ``.seisnc`` files.  Only
  ``--coords_origin header`` is supported; ``aux`` raises ``NotImplementedError``.
* CRS: a ``spatial_ref`` of the cube setup that differs from ``params_spatial_ref`` raises ``NotImplementedError`` (reprojection needs
  pyproj).  ``epsg`` is taken from the WKT when it names one.
* Padding: a trace that needs zero padding at both the top and the bottom of the window is padded; the reference's ``pad_trace``
  fails its assertion on such a trace.
* Fold saturates at 255 instead of wrapping around (a wrapped 0 would mask a full bin in step 13).
* IDW: a bin with traces at distance 0 shares its weight equally among them (the reference computes inf / inf = NaN there).
* Files: one sorted file list serves both the navigation and the trace headers (the reference globs one of them unsorted and joins
  the two by position).
* ``--parallel`` and ``--encode`` are accepted and have no effect; ``--path_coords`` and ``--filename_suffix`` are accepted and not
  used (the navigation comes from the input files' headers).  The per-inline intermediate files (``inlines_*/``) are not written.
"""
import argparse
import datetime
import glob
import os
import re
import sys

import numpy as np
import yaml

from . import _ffi
from .cube_io import Cube, save_cube
from .functions.binning import (STACK_METHODS, check_sampling_interval, distance, get_cube_parameter, idw_weights, nearest_per_bin,
                                polygon_centroid, trace_shifts, twt_axis)
from .functions.segy import SegyFile, scaled_coordinates
from .functions.transform import Affine
from .functions.utils import ffloat, xprint

_PACK_ROWS = 65536


def _pair(v):
    return (v, v) if isinstance(v, (int, float)) else tuple(v)


def _rows(src, rows):
    if isinstance(src, SegyFile):
        return src.traces(rows)
    return np.asarray(src)[rows].astype(np.float32, copy=False)


def bin_traces(traces, delays, x, y, *, dt, extent_cube, bin_size, rotation_angle, rotation_center=None, extent_region=None,
               bin_size_region=None, twt_limits=None, method='average', factor_dist=1.0, device=0, max_bytes=0):
    """Bin traces into a slice-major cube.

    traces: one 2-D array [ntraces][nsamples] per file (or a ``SegyFile``), or a single 2-D array; delays (ms), x, y: one value per trace
    in (file, trace) order.  extent_cube / extent_region: corner points (4, 2); bin_size / bin_size_region: one size or (iline, xline);
    twt_limits: (start, end) in ms (default: the latest start to the earliest end of the binned traces).

    Returns a dict: ``cube`` float32 (twt, iline, xline), ``fold`` uint8 (iline, xline), ``twt``, ``iline``, ``xline``, ``x`` / ``y``
    (bin centres, (iline, xline)), ``geometry`` (get_cube_parameter's extents) and ``selected`` (per kept trace: index, il, xl)."""
    if method not in STACK_METHODS:
        raise ValueError(f'unknown stacking method {method!r} (use one of {STACK_METHODS})')
    sources = [traces] if isinstance(traces, np.ndarray) and traces.ndim == 2 else list(traces)
    counts = np.array([s.ntraces if isinstance(s, SegyFile) else np.asarray(s).shape[0] for s in sources], np.int64)
    lengths = np.array([s.ns if isinstance(s, SegyFile) else np.asarray(s).shape[1] for s in sources], np.int64)
    file_of = np.repeat(np.arange(len(sources)), counts)
    row_of = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    delays = np.asarray(delays, dtype=np.float64)
    xy = np.column_stack((np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)))
    if delays.size != file_of.size or xy.shape[0] != file_of.size:
        raise ValueError('one delay and one (x, y) per trace')

    bin_size = _pair(bin_size)
    bin_size_region = _pair(bin_size_region) if bin_size_region is not None else bin_size
    extent_cube = np.asarray(extent_cube, dtype=np.float64)
    centre = tuple(rotation_center) if rotation_center is not None else tuple(polygon_centroid(extent_cube))
    fwd = Affine().rotate_around(angle=-float(rotation_angle), origin=centre)
    rev = fwd.inverse()
    bins, ilxl, geom_cube, geom_region, region_centres = get_cube_parameter(
        fwd, rev, xy, bin_size, extent_cube, bin_size_region=bin_size_region,
        region_corner_pts=None if extent_region is None else np.asarray(extent_region, dtype=np.float64), return_geometry=True)
    il_idx, xl_idx = np.unique(bins['il']), np.unique(bins['xl'])
    nil, nxl = il_idx.size, xl_idx.size

    # inner merge with the bins: positions on the grid, traces outside dropped
    pil = np.clip(np.searchsorted(il_idx, ilxl[:, 0]), 0, nil - 1)
    pxl = np.clip(np.searchsorted(xl_idx, ilxl[:, 1]), 0, nxl - 1)
    keep = np.flatnonzero((il_idx[pil] == ilxl[:, 0]) & (xl_idx[pxl] == ilxl[:, 1]))
    bid_all = pil[keep].astype(np.int64) * nxl + pxl[keep]
    order = keep[np.argsort(bid_all, kind='stable')]          # bin order, (file, trace) order inside a bin
    bid = pil[order].astype(np.int64) * nxl + pxl[order]

    if twt_limits is not None:
        t0, t1 = twt_limits
    elif order.size:
        t0, t1 = delays[order].max(), (delays[order] + lengths[file_of[order]] * dt).min()
    else:
        raise ValueError('no trace inside the cube: give twt_limits')
    twt = twt_axis(t0, t1, dt)
    nt = twt.size
    if nt < 1:
        raise ValueError(f'empty twt window {(t0, t1)}')

    fold_n = np.bincount(bid, minlength=nil * nxl)
    fold = np.minimum(fold_n, 255).astype(np.uint8).reshape(nil, nxl)
    centres = np.column_stack((bins['x'], bins['y']))
    dist = distance(xy[order], centres[bid])
    weight = None
    sel = np.arange(order.size)
    if method == 'nearest':
        sel = nearest_per_bin(dist, bid)
    elif method == 'IDW':
        weight = idw_weights(dist, bid, factor_dist)
    tr, tb = order[sel], bid[sel]
    bin_start = np.zeros(nil * nxl + 1, np.int64)
    np.cumsum(np.bincount(tb, minlength=nil * nxl), out=bin_start[1:])

    # samples packed in bin order: a chunk of inlines is one contiguous span
    tlen = lengths[file_of[tr]]
    toff = np.zeros(tr.size, np.int64)
    if tr.size:
        toff[1:] = np.cumsum(tlen)[:-1]
    samples = np.empty(int(tlen.sum()), np.float32)
    for f, src in enumerate(sources):
        pos = np.flatnonzero(file_of[tr] == f)
        ar = np.arange(lengths[f])
        for p0 in range(0, pos.size, _PACK_ROWS):
            p = pos[p0:p0 + _PACK_ROWS]
            samples[(toff[p][:, None] + ar[None, :]).ravel()] = _rows(src, row_of[tr[p]]).ravel()
    shift = trace_shifts(delays[tr], twt[0], dt)
    cube = _ffi.bin_stack(samples, toff, tlen, shift, bin_start, nil, nxl, nt, method=method, weight=weight, max_bytes=max_bytes,
                          device=device)
    return {'cube': cube, 'fold': fold, 'twt': twt, 'iline': il_idx, 'xline': xl_idx, 'x': bins['x'].reshape(nil, nxl),
            'y': bins['y'].reshape(nil, nxl), 'bins': bins, 'geometry': (geom_cube, geom_region, region_centres),
            'selected': {'trace': order, 'il': ilxl[order, 0], 'xl': ilxl[order, 1], 'dist': dist}}


# ---- files ----------------------------------------------------------------------------------------------------------------------
def list_segy_files(path_input, suffix='sgy'):
    """SEG-Y files of a directory (``*.{suffix}``) or of a datalist (one name per line, relative to the list's directory), sorted."""
    if os.path.isdir(path_input):
        pattern = suffix if suffix.startswith('*') else ('*' + suffix if suffix.startswith('.') else f'*.{suffix}')
        return sorted(glob.glob(os.path.join(path_input, pattern)))
    if os.path.isfile(path_input):
        base = os.path.dirname(path_input)
        with open(path_input) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        return sorted(n if os.path.isabs(n) else os.path.join(base, n) for n in names)
    raise IOError(f'{path_input!r} is neither a directory nor a datalist')


def read_segy_headers(files):
    """Open the files (memory-mapped) and scrape the headers step 10 needs, in (file, trace) order."""
    segys = [SegyFile(p) for p in files]
    if not segys:
        raise IOError('no SEG-Y files found')
    cat = {k: np.concatenate([s.header(k) for s in segys]) for k in ('SourceGroupScalar', 'SourceX', 'SourceY', 'DelayRecordingTime',
                                                                     'TRACE_SAMPLE_INTERVAL', 'TRACE_SAMPLE_COUNT', 'TRACE_SEQUENCE_FILE')}
    x, y = scaled_coordinates(cat['SourceGroupScalar'], cat['SourceX'], cat['SourceY'])
    dt_file = [s.header('TRACE_SAMPLE_INTERVAL').min() / 1000.0 for s in segys]
    return segys, cat, x, y, dt_file


def epsg_from_wkt(wkt):
    """The EPSG code a WKT string names for its CRS (the last ID / AUTHORITY), else None."""
    hits = re.findall(r'(?:ID|AUTHORITY)\[\s*"EPSG"\s*,\s*"?(\d+)"?\s*\]', str(wkt))
    return int(hits[-1]) if hits else None


def _size_str(v):
    return f'{v:.0f}' if v % 1 == 0 else f'{v}'


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(description='Create sparse 3D cube from several 2D profiles (SEG-Y), stacked on the GPU.')
    parser.add_argument('path_input', type=str, help='Input directory or path to datalist.')
    parser.add_argument('--params_netcdf', type=str, required=True, help='Path of netCDF parameter file (YAML format).')
    parser.add_argument('--params_spatial_ref', type=str, required=True,
                        help='Path of spatial reference parameter file with CRS as WKT string (YAML format).')
    parser.add_argument('--params_cube_setup', type=str, required=True, help='Path of config file for cube geometry setup (YAML format).')
    parser.add_argument('--output_dir', '-o', type=str, help='Output directory for the cube files.')
    parser.add_argument('--suffix', '-s', type=str, help='File suffix. Only used when "path_input" is a directory.')
    parser.add_argument('--filename_suffix', '-fns', type=str,
                        help='Filename suffix for guided selection (e.g. "env" or "despk"). Accepted, not used.')
    parser.add_argument('--attribute', '-a', type=str, choices=['amp', 'env'], help='Seismic attribute to compute.')
    parser.add_argument('--coords_origin', choices=['header', 'aux'], default='header',
                        help='Origin of (shotpoint) coordinates (i.e. navigation); only "header" is supported.')
    parser.add_argument('--path_coords', type=str, required=True,
                        help='Path to SEG-Y directory (coords_origin == header) or auxiliary navigation file (coords_origin == aux). '
                             'Accepted, not used: the navigation comes from the input files.')
    parser.add_argument('--coords_fsuffix', type=str, help='File suffix of auxiliary or SEG-Y files (depending on `coords_origin`).')
    parser.add_argument('--bin_size', type=float, nargs='+',
                        help='Bin size(s) in inline and crossline direction(s) given in CRS units (e.g., meter). '
                             'Single value or space-separated `inline` and `crossline` values.')
    parser.add_argument('--twt_limits', type=float, nargs='+', help='Vertical two-way travel time range of output 3D cube (in ms).')
    parser.add_argument('--parallel', action='store_true', help='Accepted for compatibility; no effect (stacking runs on the GPU).')
    parser.add_argument('--encode', action='store_true', help='Accepted for compatibility; no effect (no netCDF encoding is applied).')
    parser.add_argument('--stacking_method', type=str, choices=STACK_METHODS, help='Stacking method for multiple traces within one bin.')
    parser.add_argument('--factor_dist', type=float, default=1.0,
                        help='Distance factor controlling the impact of weighting function: 1/(distance**factor). '
                             'Only used if stacking_method="IDW".')
    parser.add_argument('--dtype_data', type=str, default='float32', help='Output dtype of created 3D cube.')
    parser.add_argument('--name', type=str, default='', help='Optional identifier string to add to exported files.')
    parser.add_argument('--write_aux', action='store_true', help='Write auxiliary files featuring key cube parameters.')
    parser.add_argument('--file_type', type=str, choices=['nc', 'npz'], default='nc', help='Output file type (default: nc).')
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, const=1, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0)')
    return parser
# fmt: on


def resolve_settings(args, cfg):
    """Command line over cube-setup config (reference :1486-1560): bin sizes and their file-name string, twt limits, stacking method
    and distance factor, name and attribute."""
    if args.bin_size is not None:
        bin_size = (args.bin_size[0], args.bin_size[0]) if len(args.bin_size) == 1 else tuple(args.bin_size)
    elif cfg.get('bin_size') is not None:
        bin_size = _pair(cfg['bin_size'])
    else:
        raise ValueError('`bin_size` is required! Either (1) as command line parameter or (2) from cube geometry config file.')
    size_il, size_xl = _size_str(bin_size[0]), _size_str(bin_size[1])
    bin_size_str = f'{size_il.replace(".", "+")}x{size_xl.replace(".", "+")}m'
    bin_size_region, bin_size_region_str = bin_size, None
    if 'bin_size_region' in cfg:
        bin_size_region = _pair(cfg['bin_size_region'])
        size_il, size_xl = _size_str(bin_size_region[0]), _size_str(bin_size_region[1])   # (the reference's text then names these)
        bin_size_region_str = f'{size_il.replace(".", "+")}x{size_xl.replace(".", "+")}m'

    if args.twt_limits is not None:
        twt_limits = tuple(args.twt_limits)
    elif cfg.get('twt_limits') is not None and len(cfg['twt_limits']) == 2:
        twt_limits = tuple(cfg['twt_limits'])
    else:
        raise ValueError('`twt_limits` are required! Either (1) as command line parameter or (2) from cube geometry config file.')

    if args.stacking_method is not None:
        method, factor_dist = args.stacking_method, args.factor_dist
    elif cfg.get('stacking_method') in STACK_METHODS:
        method, factor_dist = cfg['stacking_method'], cfg.get('factor_dist', 1.0)
    else:
        method, factor_dist = 'average', None
        xprint(f'No `stacking_method` provided, using default method: < {method} >', kind='warning', verbosity=args.verbose)

    name = args.name if args.name != '' else cfg.get('name', os.path.split(os.path.split(args.params_cube_setup)[0])[-1])
    name += f'_{method}'
    attr = args.attribute if args.attribute is not None else cfg.get('attribute', '')
    attr = f'_{attr}' if attr != '' else attr
    return dict(bin_size=bin_size, bin_size_str=bin_size_str, bin_size_region=bin_size_region, bin_size_region_str=bin_size_region_str,
                size_il=size_il, size_xl=size_xl, twt_limits=twt_limits, method=method, factor_dist=factor_dist, name=name, attr=attr)


def output_names(dir_out, name, attr, bin_size_str, dt, file_type='nc'):
    """The reference's two cube paths: (iline, xline, twt) and (twt, iline, xline)."""
    fname = f'{name}{attr}_{bin_size_str}_{ffloat(dt).replace(".", "+")}ms'
    return os.path.join(dir_out, f'{fname}.{file_type}'), os.path.join(dir_out, f'{fname}_twt-il-xl.{file_type}')


def _write_aux(dir_out, s, res, use_region, segys, cat):
    name, bs = s['name'], s['bin_size_str']
    b = res['bins']
    np.savetxt(os.path.join(dir_out, f'aux_{name}_{bs}_bins.txt'), np.column_stack((b['il'], b['xl'], b['x'], b['y'])),
               fmt=['%d', '%d', '%.10f', '%.10f'], delimiter=',', header='il,xl,x,y', comments='')
    geom_cube, geom_region, centres = res['geometry']
    kw = dict(fmt='%.10f', delimiter=';', newline='\n', header='x;y', comments='')
    np.savetxt(os.path.join(dir_out, f'aux_{name}_{bs}_extent_corner_points.txt'), geom_cube[0], **kw)
    if use_region:
        np.savetxt(os.path.join(dir_out, f'aux_region_{bs}_extent_corner_points.txt'), geom_region[0], **kw)
        np.savetxt(os.path.join(dir_out, f'aux_region_{s["bin_size_region_str"]}_outer_bin_center_points.txt'), centres, **kw)
    sel = res['selected']
    counts = np.array([sg.ntraces for sg in segys])
    line_id = np.repeat(np.arange(counts.size), counts)[sel['trace']]
    np.savetxt(os.path.join(dir_out, f'aux_{name}_{bs}_selected_traces.txt'),
               np.column_stack((line_id, cat['TRACE_SEQUENCE_FILE'][sel['trace']], sel['il'], sel['xl'], sel['dist'])),
               fmt=['%d', '%d', '%d', '%d', '%.6f'], delimiter=',', header='line_id,TRACE_SEQUENCE_FILE,il,xl,dist_bin_center', comments='')


def main(argv=sys.argv, return_dataset=False):  # noqa
    """Bin SEG-Y profiles into a sparse 3D cube (step 10)."""
    TODAY = datetime.date.today().strftime('%Y-%m-%d')
    SCRIPT = os.path.splitext(os.path.basename(__file__))[0]
    args = define_input_args().parse_args(argv[1:])
    verbose = args.verbose

    if args.coords_origin == 'aux':
        raise NotImplementedError('--coords_origin aux: navigation from auxiliary files is not supported; use the SEG-Y headers')
    path_input = args.path_input
    dir_work = path_input if os.path.isdir(path_input) else os.path.dirname(path_input)
    dir_out = args.output_dir if args.output_dir is not None else dir_work
    suffix = args.suffix or args.coords_fsuffix or 'sgy'

    with open(args.params_netcdf) as f_attrs, open(args.params_spatial_ref) as f_crs:
        kwargs_nc = yaml.safe_load(f_attrs)
        kwargs_nc['spatial_ref'] = yaml.safe_load(f_crs)
    with open(args.params_cube_setup) as f:
        cfg = yaml.safe_load(f)
    s = resolve_settings(args, cfg)
    method = s['method']

    attrs_time = kwargs_nc.setdefault('attrs_time', {})
    cube_attrs = dict(attrs_time.get('cube', {}) or {})
    cube_attrs['long_name'] = cfg['long_name']
    cube_attrs['history'] = (cube_attrs.get('history') or '') + f'{SCRIPT}: create sparse 3D volume;'
    cube_attrs['text'] = ((cube_attrs.get('text') or '') + '\n=== 3D PROCESSING ===' +
                          f'\n{TODAY}: 3D BINNING {method} ILINE:{s["size_il"]} XLINE:{s["size_xl"]} UNIT:METER')

    extent_cube = np.asarray(list(cfg['extent_cube'].values()), dtype=np.float64)
    use_region = 'extent_region' in cfg
    extent_region = np.asarray(list(cfg['extent_region'].values()), dtype=np.float64) if use_region else None
    if cfg.get('spatial_ref') is not None and str(cfg['spatial_ref']).strip() != str(kwargs_nc['spatial_ref']).strip():
        raise NotImplementedError('the cube setup and params_spatial_ref name different coordinate reference systems; '
                                  'reprojecting the extent needs pyproj, which is not available')
    rotation_center = cfg.get('rotation_center')

    files = list_segy_files(path_input, suffix)
    xprint(f'Scrape trace headers of > {len(files)} < SEG-Y files', kind='info', verbosity=verbose)
    segys, cat, x, y, dt_file = read_segy_headers(files)
    dt = check_sampling_interval(dt_file)

    res = bin_traces(segys, cat['DelayRecordingTime'], x, y, dt=dt, extent_cube=extent_cube, bin_size=s['bin_size'],
                     rotation_angle=float(cfg['rotation_angle']), rotation_center=rotation_center, extent_region=extent_region,
                     bin_size_region=s['bin_size_region'] if use_region else None, twt_limits=s['twt_limits'], method=method,
                     factor_dist=s['factor_dist'] if s['factor_dist'] is not None else 1.0)
    xprint(f'Traces: >{res["selected"]["trace"].size}< valid out of >{x.size}< traces within extent', kind='info', verbosity=verbose)

    os.makedirs(dir_out, exist_ok=True)
    if args.write_aux:
        _write_aux(dir_out, s, res, use_region, segys, cat)

    var = 'env' if args.attribute == 'env' or s['attr'] == '_env' else 'amp'
    wkt = kwargs_nc['spatial_ref']
    projected = str(wkt).lstrip().upper().startswith(('PROJCS', 'PROJCRS', 'PROJECTEDCRS'))
    stack_str = f'{method} (distance factor={s["factor_dist"]})' if method == 'IDW' else method
    attrs = {'bin_units': 'm', 'measurement_system': 'm' if projected else 'deg', 'epsg': epsg_from_wkt(wkt) or 'None',
             'stacking_method': stack_str, 'spatial_ref': wkt if wkt is not None else 'None',
             'bin_size_iline': s['bin_size'][0], 'bin_size_xline': s['bin_size'][1]}
    attrs.update(cube_attrs)
    fold = res['fold']
    fold_attrs = dict(attrs_time.get('fold', {}) or {})
    fold_attrs['coverage_perc'] = round(np.count_nonzero(fold) / fold.size * 100, 2)
    coord_attrs = {k: dict(attrs_time.get(k, {}) or {}) for k in ('twt', 'iline', 'xline')}
    coord_attrs['twt']['dt'] = dt
    coord_attrs['iline'].update(bin_il=s['bin_size'][0], comment='`bin_il` is the bin distance ALONG dim `iline` and NOT the inline spacing')
    coord_attrs['xline'].update(bin_xl=s['bin_size'][1], comment='`bin_xl` is the distance ALONG dim `xline` and NOT the crossline spacing')
    coords = {'iline': res['iline'], 'xline': res['xline'], 'twt': res['twt']}
    data = res['cube'].astype(np.dtype(args.dtype_data), copy=False)

    def make(amp, amp_dims):
        return Cube({var: amp, 'fold': fold, 'x': res['x'], 'y': res['y']},
                    {var: amp_dims, 'fold': ('iline', 'xline'), 'x': ('iline', 'xline'), 'y': ('iline', 'xline')},
                    coords, attrs, {var: dict(attrs_time.get(var, {}) or {}), 'fold': fold_attrs,
                                    'x': dict(attrs_time.get('x', {}) or {}), 'y': dict(attrs_time.get('y', {}) or {})}, coord_attrs)

    cube_path, cube_twt_path = output_names(dir_out, s['name'], s['attr'], s['bin_size_str'], dt, args.file_type)
    cube = make(np.ascontiguousarray(np.transpose(data, (1, 2, 0))), ('iline', 'xline', 'twt'))
    save_cube(cube, cube_path)
    cube_twt = make(data, ('twt', 'iline', 'xline'))
    save_cube(cube_twt, cube_twt_path)
    xprint(f'Bin fold:  {fold_attrs["coverage_perc"]:.2f}%  ({np.count_nonzero(fold)} out of {fold.size} bins)', kind='info',
           verbosity=verbose)
    if return_dataset:
        return cube, cube_twt
    return None


if __name__ == '__main__':
    main()
