"""
Step 15 -- post-processing of a (pseudo-)3D cube on the GPU, mirror of ``pseudo_3D_interpolation/cube_postprocessing_3D.py``.

Command line (``15_cube_postprocessing``, :32-85) and order of the operations (:491-717): iline / xline upsampling
(``upsample_ilxl``, :350-488; HIP kernel ``p3d_upsample``), acquisition footprint removal over the slices or over the
(line, twt) profiles (``remove_acquisition_footprint``, :179-260), smoothing of the slices with an optional percentile rescale
(``smoothing_filter``, :88-124) and automatic gain control along twt (``functions.signal.AGC``; HIP kernel ``p3d_agc``).

The kx-ky filters -- ``remove_acquisition_footprint`` and ``spatial_antialiasing`` (:263-347), both
``ifft2(ifftshift(filter) * fft2(slice)).real`` with a filter that depends on the slice shape only, and their helper
``gaussian_kernel_2d`` (:127-176) -- build the filter once on the host (NumPy; the reference uses scipy.signal.fftconvolve for
the same convolution) and send the slices through the 2-D FFT kernels of this package in batches.  ``smoothing_filter`` runs
scipy.ndimage's gaussian / median filter semantics in HIP gather kernels.

Cubes are read and written through ``cube_io`` (``.nc`` or ``.npz``) instead of xarray / dask.  Departures from the reference:

* AGC runs along twt, trace by trace, as the reference's documentation describes, and the output keeps ``(twt, iline, xline)``.
  The reference (:685) applies ``AGC`` along the LAST axis of the slice-major array (xline) and assigns the result to the dims
  ``('iline', 'xline', 'twt')``, which cannot be constructed unless nt == nil == nxl.  AGC also runs on the cube as processed so
  far (a profile footprint removal before it is kept), where the reference re-reads the input.
* ``--path_out`` (parsed but ignored by the reference) names the output file, or the directory it goes to.
* The profile footprint removal derives its profile direction also when ``--direction`` is given (the reference only does so
  without it and fails otherwise).
* Variables that are not 3-D (``fold``) are upsampled on the host along with the cube and written as they come out of the
  operations above.

Not covered: ``cubic`` / ``polynomial`` upsampling, AGC pad modes other than zero padding.
"""
import argparse
import datetime
import os
import re
import sys

import numpy as np

from . import _ffi
from .cube_io import open_cube, save_cube
from .functions.signal import AGC, get_AGC_samples
from .functions.utils import convert_twt, rescale, xprint


# fmt: off
def define_input_args():  # noqa
    parser = argparse.ArgumentParser(description='Apply post-processing algorithm to (pseudo-)3D cube.')
    parser.add_argument('path_cube', type=str, help='Input path of 3D cube')
    parser.add_argument('--path_out', type=str, help='Output path of pre-processed 3D cube')
    # UPSAMPLING
    parser.add_argument(
        '--upsample', nargs='?', type=str, const='linear', choices=['linear', 'nearest', 'slinear', 'cubic', 'polynomial'],
        help='Upsample cube to equal bin size along ilines and xlines.'
    )
    parser.add_argument(
        '--spatial-dealiasing', action='store_true', help='Whether to apply filter in kx-ky domain to remove spatial aliasing.'
    )
    # FOOTPRINT
    parser.add_argument(
        '--remove-footprint', nargs='?', const='slice', choices=['slice', 'profile', 'profile-iline', 'profile-xline'],
        help='Remove acquisition footprint.'
    )
    parser.add_argument(
        '--direction', choices=['both', 'iline', 'xline', 'twt'],
        help="Direction of acquisition footprint removal filter (default: `'both'`)."
    )
    parser.add_argument(
        '--footprint-sigma', type=int, default=7, help='Standard deviation for smoothing Gaussian filter (default: `7`) to remove footprint.'
    )
    parser.add_argument(
        '--buffer-center', type=float, default=0.20, help='Percentual buffer (0-1) around center in kx-ky domain (default: `0.20`).'
    )
    parser.add_argument(
        '--buffer-filter', type=int, default=3, help='Footprint filter buffer size (in grid cells).'
    )
    # FILTER
    parser.add_argument(
        '--smooth', nargs='?', choices=['gaussian', 'median'], help='Smooth slices (frequency or time domain).'
    )
    parser.add_argument(
        '--smooth-sigma', type=int, default=1, help='Standard deviation for Gaussian kernel.'
    )
    parser.add_argument(
        '--smooth-size', type=int, default=3, help='Shape of Median kernel (identical for iline and xline).'
    )
    parser.add_argument(
        '--rescale', nargs='*', default=None, type=float,
        help='Rescale smoothed slices to given percentile range (without arguments: [0.01, 99.99]).'
    )
    # AGC
    parser.add_argument('--agc', action='store_true', help='Apply Automatic Gain Control (AGC).')
    parser.add_argument('--agc-win', type=float, help='AGC window length (in seconds).')
    parser.add_argument('--agc-kind', type=str, default='rms', choices=['rms', 'mean', 'median'], help='AGC kind.')
    parser.add_argument('--agc-sqrt', action='store_true', help='Whether to compute squared AGC (enhances strong amplitudes).')
    #
    parser.add_argument('--verbose', '-V', type=int, nargs='?', default=0, const=1, choices=[0, 1, 2],
                        help='Level of output verbosity (default: 0)')
    return parser
# fmt: on


def smoothing_filter(x, filter_name=None, kwargs_filter=None, rescale_slice=False, kwargs_rescale=None, device=0):
    """Same arguments as the reference's wrapper of ``scipy.ndimage`` (cube_postprocessing_3D.py:88-124); ``x`` is one slice
    ``(ny, nx)`` or a stack ``(n, ny, nx)`` (each slice filtered -- and rescaled -- on its own).  Supported: ``gaussian`` with a
    scalar ``sigma`` (``truncate`` optional) and ``median`` with an odd ``size`` of 3, 5 or 7, both with SciPy's default
    'reflect' boundary; the arithmetic is float32."""
    kwargs_filter = dict(kwargs_filter or {})
    if filter_name not in ('gaussian', 'median'):
        raise TypeError(f'unknown filter {filter_name!r}')       # the reference calls None(...) here
    if kwargs_filter.pop('mode', 'reflect') != 'reflect':
        raise NotImplementedError("only the default boundary mode 'reflect' is implemented")
    if filter_name == 'gaussian':
        extra = set(kwargs_filter) - {'sigma', 'truncate'}
        if extra or np.ndim(kwargs_filter.get('sigma')) != 0 or kwargs_filter.get('sigma') is None:
            raise NotImplementedError(f'gaussian: scalar sigma (and truncate) only, got {sorted(kwargs_filter)}')
    else:
        extra = set(kwargs_filter) - {'size'}
        if extra or kwargs_filter.get('size') not in (3, 5, 7):
            raise NotImplementedError(f'median: size 3, 5 or 7 only, got {kwargs_filter}')
    x = np.asarray(x)
    squeeze = x.ndim == 2
    stack = x[None] if squeeze else x
    filt = _ffi.smooth_slices(stack, filter_name, device=device, **kwargs_filter)
    if rescale_slice:
        lo_hi = sorted(kwargs_rescale['vminmax'])
        for i in range(stack.shape[0]):
            vmin, vmax = np.percentile(stack[i], lo_hi)
            filt[i] = rescale(filt[i], vmin=vmin, vmax=vmax)
    return filt[0] if squeeze else filt


def _gaussian_window(m, sigma):
    k = np.arange(m) - (m - 1) / 2.0
    return np.exp(-0.5 * (k / sigma) ** 2)


def gaussian_kernel_2d(sigma=7, n=None, normalized=True, orientation='equal'):
    """2-D Gaussian kernel (same arguments and sizes as the reference's, cube_postprocessing_3D.py:127-176)."""
    ny, nx = n if isinstance(n, tuple) else (n, n)
    factor = {'equal': (8, 8), 'iline': (2, 8), 'xline': (8, 2)}
    ny = sigma * factor[orientation][0] + 1 if ny is None else ny
    ny = ny + 1 if ny % 2 == 0 else ny
    nx = sigma * factor[orientation][1] + 1 if nx is None else nx
    nx = nx + 1 if nx % 2 == 0 else nx
    kernel = np.outer(_gaussian_window(ny, sigma), _gaussian_window(nx, sigma))
    if normalized:
        kernel /= 2 * np.pi * (sigma ** 2)
    return kernel


def _convolve_same(a, k):
    """Linear convolution cropped to the shape of ``a`` around its centre (scipy.signal.fftconvolve(a, k, mode='same'))."""
    full = (a.shape[0] + k.shape[0] - 1, a.shape[1] + k.shape[1] - 1)
    out = np.fft.irfft2(np.fft.rfft2(a, full) * np.fft.rfft2(k, full), full)
    r0, c0 = (k.shape[0] - 1) // 2, (k.shape[1] - 1) // 2
    return out[r0:r0 + a.shape[0], c0:c0 + a.shape[1]]


def _orient(direction, dims, ny, nx):
    if direction == 'iline':
        return 'horizontal' if dims[0] == 'iline' else 'vertical'
    if direction == 'xline':
        return 'vertical' if dims[1] == 'xline' else 'horizontal'
    if direction == 'twt':
        return 'vertical' if ny > nx else 'horizontal'
    return direction


def footprint_filter(shape, sigma=7, direction='both', buffer_center=0.25, buffer_filter=3, dims=('iline', 'xline')):
    """Centred kx-ky weight (1 = keep) that notches the acquisition footprint (cube_postprocessing_3D.py:212-253)."""
    ny, nx = shape
    npad = sigma * 5
    ny_pad, nx_pad = ny + npad, nx + npad
    grid = np.zeros((ny_pad, nx_pad))
    direction = _orient(direction, dims, ny, nx)
    if direction in ('both', 'horizontal'):
        cidx = nx_pad // 2 + 1
        fwidth = round(ny_pad * (1 - buffer_center) + .5) // 2
        grid[:fwidth, cidx - buffer_filter: cidx + buffer_filter + 1] = 1
        grid[-fwidth:, cidx - buffer_filter: cidx + buffer_filter + 1] = 1
    if direction in ('both', 'vertical'):
        cidx = ny_pad // 2 + 1
        fwidth = round(nx_pad * (1 - buffer_center) + .5) // 2
        grid[cidx - buffer_filter: cidx + buffer_filter + 1, :fwidth] = 1
        grid[cidx - buffer_filter: cidx + buffer_filter + 1, -fwidth:] = 1
    ffilter = _convolve_same(grid, gaussian_kernel_2d(sigma=sigma))
    return 1 - rescale(ffilter[npad // 2: -npad // 2, npad // 2: -npad // 2])


def antialias_filter(shape, direction, factors_upsampling, sigma=7, dims=('iline', 'xline')):
    """Centred kx-ky weight of the de-aliasing filter after iline / xline upsampling (cube_postprocessing_3D.py:300-340)."""
    il, xl = dims
    if not sorted(dims) == sorted(factors_upsampling.keys()):
        raise ValueError(f'Coordinates {dims} not found in `factors_upsampling` {factors_upsampling.keys()}')
    ny, nx = shape
    npad = sigma * 5
    p = 0.98
    grid = np.zeros((ny + npad, nx + npad))
    direction = _orient(direction, dims, ny, nx)
    if direction == 'horizontal':
        perc = 1 - factors_upsampling.get(xl, 1) / factors_upsampling.get(il, 1)
        half = round(ny * perc * p) // 2 + npad
        grid[half:-half, :] = 1
    elif direction == 'vertical':
        perc = 1 - factors_upsampling.get(il, 1) / factors_upsampling.get(xl, 1)
        half = round(nx * perc * p) // 2 + npad
        grid[:, half:-half] = 1
    ffilter = _convolve_same(grid, gaussian_kernel_2d(sigma=sigma))
    return rescale(ffilter[npad // 2: -npad // 2, npad // 2: -npad // 2], vmin=1e-3, vmax=1)


def apply_kxky_filter(data, ffilter, device=0, batch_slices=None):
    """``ifft2(ifftshift(ffilter) * fft2(slice)).real`` for one slice ``(ny, nx)`` or a stack ``(n, ny, nx)`` on the GPU
    (one real spectrum weight = a one-element frame of ``_ffi.ShearletPlan``)."""
    data = np.asarray(data)
    squeeze = data.ndim == 2
    stack = data[None] if squeeze else data
    if stack.ndim != 3 or stack.shape[1:] != ffilter.shape:
        raise ValueError(f'data {data.shape} does not match the filter {ffilter.shape}')
    n = stack.shape[0]
    step = int(batch_slices) if batch_slices else max(1, min(n, (256 << 20) // (stack.shape[1] * stack.shape[2] * 8)))
    out = np.empty(stack.shape, np.float64 if stack.dtype == np.float64 else np.float32)
    weight = np.fft.ifftshift(np.asarray(ffilter, dtype=np.float64))[..., None]
    with _ffi.ShearletPlan(weight, max_slices=min(step, n), device=device) as plan:
        for lo in range(0, n, step):
            out[lo:lo + step] = plan.transform(stack[lo:lo + step].astype(np.complex64))[..., 0].real
    return out[0] if squeeze else out


def remove_acquisition_footprint(data, sigma=7, direction='both', buffer_center=0.25, buffer_filter=3, return_filter=False,
                                 dims=('iline', 'xline'), verbose=1, device=0):
    """Same arguments as the reference's function; ``data`` may also be a stack of slices ``(n, ny, nx)``."""
    data = np.asarray(data)
    ffilter = footprint_filter(data.shape[-2:], sigma, direction, buffer_center, buffer_filter, dims)
    filt = apply_kxky_filter(data, ffilter, device=device)
    return (filt, ffilter) if return_filter else filt


def spatial_antialiasing(data, direction, factors_upsampling, sigma=7, dims=('iline', 'xline'), return_filter=False, verbose=1,
                         device=0):
    """Same arguments as the reference's function; ``data`` may also be a stack of slices ``(n, ny, nx)``."""
    data = np.asarray(data)
    ffilter = antialias_filter(data.shape[-2:], direction, factors_upsampling, sigma, dims)
    filt = apply_kxky_filter(data, ffilter, device=device)
    return (filt, ffilter) if return_filter else filt


# ---- iline / xline upsampling ------------------------------------------------------------------------------------------------
_METHODS = ('linear', 'slinear', 'nearest')


def interp_table(src, dst, method='linear'):
    """Per output coordinate ``dst``: the source line ``i0`` at or below it and the weight ``w`` towards line ``i0 + 1``.
    ``linear`` / ``slinear`` (the same in 1-D): ``w = (dst - src[i0]) / (src[i0 + 1] - src[i0])``; ``nearest``: the nearer source
    line, the lower one on an exact tie (SciPy's interp1d / interpn under ``interp_like``), ``w = 0``."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    i0 = np.clip(np.searchsorted(src, dst, side='right') - 1, 0, src.size - 1)
    i1 = np.minimum(i0 + 1, src.size - 1)
    span = src[i1] - src[i0]
    w = np.where(span > 0, (dst - src[i0]) / np.where(span > 0, span, 1.0), 0.0)
    if method == 'nearest':
        i0, w = np.where(w > 0.5, i1, i0), np.zeros_like(w)
    return i0.astype(np.int32), w


def _interp_host(a, tables):
    """Separable interpolation of a 2-D variable (iline, xline) on the host, in float64 (``interp_like`` on a 2-D variable)."""
    out = np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64)
    for axis, (i0, w) in enumerate(tables):
        i1 = np.minimum(i0 + 1, out.shape[axis] - 1)
        w = w.reshape((-1, 1) if axis == 0 else (1, -1))
        out = (1 - w) * np.take(out, i0, axis=axis) + w * np.take(out, i1, axis=axis)
    return out


def _to_slices(data, dims, dim):
    """``data`` with dims ``dims`` as a slice-major stack ``(dim, iline, xline)``."""
    order = [dims.index(d) for d in (dim, 'iline', 'xline')]
    return np.transpose(data, order) if order != [0, 1, 2] else data


def upsample_ilxl(cube, coords=('iline', 'xline'), method='linear', update_attrs=True, spatial_dealiasing=True, return_factor=False,
                  verbose=1, device=0):
    """Upsample a :class:`cube_io.Cube` to equal bin sizes along ilines and xlines (the reference's ``upsample_ilxl`` on an
    ``xr.Dataset``, cube_postprocessing_3D.py:350-488).  An axis whose first coordinate step ``d`` is not 1 is filled to every
    integer line from its first to its last; every 3-D variable (float32 or complex64) is interpolated on the GPU
    (``p3d_upsample``), 2-D variables (``fold``) on the host with the same method.  ``update_attrs`` updates ``bin_il`` / ``bin_xl``
    of the coordinates and ``bin_size_iline`` / ``bin_size_xline`` of the cube; ``spatial_dealiasing`` runs ``spatial_antialiasing``
    over the upsampled slices.  Returns the new cube (and the factors ``{'iline': d_il, 'xline': d_xl}`` when ``return_factor``);
    without a gap the input cube itself comes back, with the factors."""
    il, xl = coords
    if method in ('cubic', 'polynomial'):
        raise NotImplementedError(f'upsampling method {method!r} is not implemented (linear, slinear, nearest)')
    if method not in _METHODS:
        raise ValueError(f'unknown upsampling method {method!r}')
    diff_ilines = np.diff(cube.coords[il])[0]
    interp_ilines = diff_ilines != 1
    diff_xlines = np.diff(cube.coords[xl])[0]
    interp_xlines = diff_xlines != 1
    if not interp_ilines and not interp_xlines:
        xprint(f'No missing/omitted `{coords[0]}` or `{coords[1]}` indices. Returning input dataset.', kind='warning', verbosity=verbose)
        return cube, dict(iline=diff_ilines, xline=diff_xlines)

    src_il, src_xl = np.asarray(cube.coords[il]), np.asarray(cube.coords[xl])
    new_il = np.arange(src_il[0], src_il[-1] + 1, 1) if interp_ilines else src_il
    new_xl = np.arange(src_xl[0], src_xl[-1] + 1, 1) if interp_xlines else src_xl
    out = cube.copy_meta()
    out.coords[il], out.coords[xl] = new_il, new_xl
    out.var_attrs = {k: dict(v) for k, v in cube.var_attrs.items()}
    if update_attrs:
        bin_il = out.coord_attrs.get(il, {}).get('bin_il')
        bin_xl = out.coord_attrs.get(xl, {}).get('bin_xl')
        if all([bin_il, bin_xl]):
            if interp_xlines:
                out.coord_attrs.setdefault(il, {})['bin_il'] = type(bin_xl)(bin_il / diff_xlines)
            if interp_ilines:
                out.coord_attrs.setdefault(xl, {})['bin_xl'] = type(bin_il)(bin_xl / diff_ilines)
            attrs_update = {'bin_size_iline': type(bin_xl)(bin_il / diff_xlines), 'bin_size_xline': type(bin_il)(bin_xl / diff_ilines)}
        else:
            raise ValueError('Could not find metadata `bin_il` and/or `bin_xl`')

    t_il, t_xl = interp_table(src_il, new_il, method), interp_table(src_xl, new_xl, method)
    for name, data in cube.data_vars.items():
        dims = tuple(cube.dims[name])
        data = np.asarray(data)
        if data.ndim == 3 and il in dims and xl in dims:
            dim = [d for d in dims if d not in (il, xl)][0]
            stack = np.transpose(data, [dims.index(d) for d in (dim, il, xl)])
            kind = np.complex64 if np.iscomplexobj(stack) else np.float32
            up = _ffi.upsample_slices(stack.astype(kind, copy=False), t_il[0], t_il[1], t_xl[0], t_xl[1], device=device)
            out.data_vars[name], out.dims[name] = up, (dim, il, xl)
        elif data.ndim == 2 and set(dims) == {il, xl}:
            a = data if dims == (il, xl) else data.T
            out.data_vars[name], out.dims[name] = _interp_host(a, (t_il, t_xl)), (il, xl)
        elif il in dims or xl in dims:
            raise NotImplementedError(f'variable {name!r} with dims {dims}: only 3-D cubes and 2-D (iline, xline) maps are upsampled')
        else:
            out.data_vars[name], out.dims[name] = data, dims
    if update_attrs:
        out.attrs.update(attrs_update)

    if spatial_dealiasing:
        kwargs = dict(direction='iline' if interp_ilines else 'xline', factors_upsampling=dict(iline=diff_ilines, xline=diff_xlines), sigma=7,
                      verbose=verbose)
        for name, data in out.data_vars.items():
            if np.ndim(data) == 3:
                out.data_vars[name] = spatial_antialiasing(data, device=device, **kwargs)

    if return_factor:
        return out, dict(iline=diff_ilines, xline=diff_xlines)
    return out


# ---- the step-15 driver --------------------------------------------------------------------------------------------------------
def _profile_planes(stack, dim_direction):
    """Slice-major ``(twt, iline, xline)`` -> profile planes: ``(iline, xline, twt)`` (one ``(xline, twt)`` plane per inline) when
    ``dim_direction == 'xline'``, ``(xline, iline, twt)`` (one ``(iline, twt)`` plane per crossline) when it is ``'iline'``."""
    return np.ascontiguousarray(np.transpose(stack, (1, 2, 0) if dim_direction == 'xline' else (2, 1, 0)))


def _from_profile_planes(planes, dim_direction):
    return np.ascontiguousarray(np.transpose(planes, (2, 0, 1) if dim_direction == 'xline' else (2, 1, 0)))


def main(argv=sys.argv, return_dataset=False):  # noqa
    """Post-process 3D cube wrapper function (the reference's main, cube_postprocessing_3D.py:491-717)."""
    TODAY = datetime.date.today().strftime('%Y-%m-%d')
    SCRIPT = os.path.splitext(os.path.basename(__file__))[0]

    parser = define_input_args()
    args = parser.parse_args(argv[1:])
    args.rescale = [0.01, 99.99] if args.rescale == [] else args.rescale
    xprint(args, kind='debug', verbosity=args.verbose)

    if (args.agc or args.remove_footprint == 'profile') and (args.remove_footprint == 'slice' or args.upsample or args.smooth):
        xprint(
            (
                'The option `--agc`/`--remove_footprint profile` and `--remove_footprint slice`/`--upsampling`/`--filter`'
                ' are mutually exclusive as they require different chunk sizes. Please run this script twice instead.'
            ), kind='error', verbosity=args.verbose
        )
        return

    path_cube = args.path_cube
    dir_work, filename = os.path.split(path_cube)
    basename, suffix = os.path.splitext(filename)

    # (0) open cube
    cube = open_cube(path_cube)
    dim = cube.slice_dim()
    data_vars = [var for var in cube.data_vars if np.ndim(cube.data_vars[var]) == 3]
    nodata_vars = [var for var in cube.data_vars if var not in data_vars]
    xprint(f'dim:         {dim}', kind='debug', verbosity=args.verbose)
    xprint(f'data_vars:   {data_vars}', kind='debug', verbosity=args.verbose)
    xprint(f'nodata_vars: {nodata_vars}', kind='debug', verbosity=args.verbose)

    # profile planes of the footprint removal (the reference's chunk choice, :534-546)
    dim_direction = None
    if args.remove_footprint is not None and 'profile' in args.remove_footprint:
        if 'iline' in args.remove_footprint:
            dim_direction = 'xline'           # one inline per chunk: (xline, twt) planes
        elif 'xline' in args.remove_footprint:
            dim_direction = 'iline'           # one crossline per chunk: (iline, twt) planes
        else:
            dim_direction = 'xline' if cube.coords['iline'].size < cube.coords['xline'].size else 'iline'

    # every 3-D variable as a slice-major stack (dim, iline, xline)
    cube_proc = cube.copy_meta()
    cube_proc.var_attrs = {k: dict(v) for k, v in cube.var_attrs.items()}
    for var in cube.data_vars:
        if var in data_vars:
            cube_proc.data_vars[var] = _to_slices(np.asarray(cube.data_vars[var]), tuple(cube.dims[var]), dim)
            cube_proc.dims[var] = (dim, 'iline', 'xline')
        else:
            cube_proc.data_vars[var], cube_proc.dims[var] = cube.data_vars[var], cube.dims[var]
    _history = f'{SCRIPT}:'
    _text = f'{TODAY}: '
    text_suffix = ''

    # ========== inline/crossline upsampling (to equal bin sizes) ==========
    if args.upsample is not None:
        xprint('Upsample iline/xline bins to equal size', kind='info', verbosity=args.verbose)
        cube_proc, factor = upsample_ilxl(cube_proc, method=args.upsample, spatial_dealiasing=args.spatial_dealiasing, return_factor=True,
                                          verbose=args.verbose)
        if factor['iline'] != factor['xline']:
            _history += ' iline/xline bin size upsampling,'
            _text += 'UPSAMPLING.'
            text_suffix += '_upsampled'
            bin_size_iline = cube.attrs['bin_size_iline'] / factor['xline']
            bin_size_iline = f"{bin_size_iline:.0f}" if bin_size_iline % 1 == 0 else f"{bin_size_iline}"
            bin_size_xline = cube.attrs['bin_size_xline'] / factor['iline']
            bin_size_xline = f"{bin_size_xline:.0f}" if bin_size_xline % 1 == 0 else f"{bin_size_xline}"
            bin_size_str = f'{bin_size_iline.replace(".","+")}x{bin_size_xline.replace(".","+")}m'
            basename = re.sub(r'_\d{1}\+?\d{0,2}x\d{1}\+?\d{0,2}m_', f'_{bin_size_str}_', basename)

    # ========== acquisition footprint removal ==========
    core_dims = ('iline', 'xline')
    if args.remove_footprint:
        xprint('Remove acquisition footprint', kind='info', verbosity=args.verbose)
        if args.direction is None:
            if args.remove_footprint == 'slice':
                ratio = cube.coord_attrs['iline'].get('bin_il') / cube.coord_attrs['xline'].get('bin_xl')
                direction = 'both' if ratio == 1 else 'iline' if ratio < 1 else 'xline'
            else:
                direction = 'twt'
                xprint('dim_direction:', dim_direction, kind='debug', verbosity=args.verbose)
            xprint(f'Detected footprint direction: `{direction}`', kind='info', verbosity=args.verbose)
        else:
            direction = args.direction
        core_dims = ('iline', 'xline') if args.remove_footprint == 'slice' else (dim_direction, dim)
        kwargs = dict(direction=direction, sigma=args.footprint_sigma, buffer_center=args.buffer_center, buffer_filter=args.buffer_filter,
                      dims=core_dims, verbose=args.verbose)
        xprint(kwargs, kind='debug', verbosity=args.verbose)
        for var in data_vars:
            stack = cube_proc.data_vars[var]
            if args.remove_footprint == 'slice':
                cube_proc.data_vars[var] = remove_acquisition_footprint(stack, **kwargs)
            else:
                planes = remove_acquisition_footprint(_profile_planes(stack, dim_direction), **kwargs)
                cube_proc.data_vars[var] = _from_profile_planes(planes, dim_direction)
        _history += f' footprint removal ({args.remove_footprint}: {direction}),'
        _text += 'FOOTPRINT REMOVAL.'
        text_suffix += '_footprint-profile' if 'profile' in args.remove_footprint else '_footprint'
        text_suffix += '-il' if 'iline' in args.remove_footprint else '-xl' if 'xline' in args.remove_footprint else ''

    # ========== smoothing filter (frequency/time slice) ==========
    if args.smooth:
        xprint(f'args.rescale:  {args.rescale}', kind='debug', verbosity=args.verbose)
        if args.smooth == 'gaussian':
            kwargs_smooth_str = 'sigma={args.smooth_sigma}'       # (sic: the reference's text, kept verbatim for tools that match it)
            kwargs_smooth = dict(filter_name=args.smooth, kwargs_filter=dict(sigma=args.smooth_sigma))
        elif args.smooth == 'median':
            kwargs_smooth_str = 'size={args.smooth_size}'         # (sic)
            kwargs_smooth = dict(filter_name=args.smooth, kwargs_filter=dict(size=args.smooth_size))
        if args.rescale:
            kwargs_smooth.update(rescale_slice=True, kwargs_rescale=dict(vminmax=args.rescale))
        xprint(f'kwargs_smooth:  {kwargs_smooth}', kind='debug', verbosity=args.verbose)
        for var in data_vars:
            stack = cube_proc.data_vars[var]
            if core_dims == ('iline', 'xline'):
                cube_proc.data_vars[var] = smoothing_filter(stack, **kwargs_smooth)
            else:   # after a profile footprint removal the reference smooths the same (line, twt) planes
                planes = smoothing_filter(_profile_planes(stack, dim_direction), **kwargs_smooth)
                cube_proc.data_vars[var] = _from_profile_planes(planes, dim_direction)
        _history += f' {args.smooth} filter ({kwargs_smooth_str}),'
        _text += f'{args.smooth.upper()} FILTER.'
        text_suffix += f'_{args.smooth}'
        text_suffix += f'-{args.smooth_sigma}' if args.smooth == 'gaussian' else f'-{args.smooth_size}'
        text_suffix += f'_rescale-{"-".join([str(i) for i in args.rescale])}' if args.rescale is not None else ''

    # ========== AGC ==========
    if args.agc:
        if dim != 'twt':
            xprint(f"Input data must be in time domain (dim='twt') and not dim={dim}", kind='error', verbosity=args.verbose)
            return
        if args.agc_win is None:
            xprint('AGC window length (`--agc-win`) is required!', kind='error', verbosity=args.verbose)
            return
        twt_attrs = cube_proc.coord_attrs.get(dim, {})
        dt = twt_attrs.get('dt', np.median(np.diff(np.asarray(cube.coords[dim]))))  # sampling interval (ms)
        dt = convert_twt(dt, twt_attrs.get('units', 'ms'), 's')
        win_samples = get_AGC_samples(args.agc_win, dt=dt)
        xprint(f'Apply AGC with window length of >{args.agc_win}< sec', kind='info', verbosity=args.verbose)
        xprint(f'win_samples: {win_samples}', kind='debug', verbosity=args.verbose)
        kwargs_agc = dict(win=win_samples, kind=args.agc_kind, squared=args.agc_sqrt)
        xprint(kwargs_agc, kind='debug', verbosity=args.verbose)
        for var in data_vars:   # along twt (axis 0 of the slice-major stack), trace by trace
            cube_proc.data_vars[var] = AGC(cube_proc.data_vars[var], axis=0, **kwargs_agc)
        _history += f' AGC (win={args.agc_win:g} kind={args.agc_kind}, squared={args.agc_sqrt}),'
        _text += 'AGC ({args.agc_win:g} s).'                     # (sic)
        text_suffix += '_AGC'

    # add/update metadata
    xprint('Update netCDF metadata attributes', kind='info', verbosity=args.verbose)
    cube_proc.attrs.update({
        'history': cube_proc.attrs.get('history', '') + f'{_history[:-1]};',  # remove trailing comma
        'text': cube_proc.attrs.get('text', '') + f'\n{_text[:-1]}',          # remove trailing period
    })

    # write the processed cube
    path_cube_proc = os.path.join(dir_work, f'{basename}{text_suffix}{suffix}')
    if args.path_out:
        path_cube_proc = os.path.join(args.path_out, f'{basename}{text_suffix}{suffix}') if os.path.isdir(args.path_out) else args.path_out
    xprint(f'Write output data to file > {os.path.basename(path_cube_proc)} <', kind='info', verbosity=args.verbose)
    save_cube(cube_proc, path_cube_proc)

    if return_dataset:
        return cube_proc, cube


if __name__ == '__main__':
    main()
