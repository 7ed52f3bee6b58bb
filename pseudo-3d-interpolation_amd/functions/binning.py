"""Cube geometry and per-trace preparation of step 10 (NumPy only), restating the reference's cube_binning_3D.py:41-558 and :955-1030.

Geometry: the cube's corner points are rotated by ``-rotation_angle`` about the rotation centre into a north-aligned frame, their
bounding box is widened to whole bins, and an affine map takes coordinates to (iline, xline) numbers starting at 1 (or at the numbers
of a larger region, with a step, when ``extent_region`` / ``bin_size_region`` are given).  A trace belongs to the bin
``np.around`` of its mapped (il, xl); traces whose bin is not part of the cube are dropped (the reference's inner merge).

Per trace: the integer offset ``o`` that puts its sample ``i`` on cube sample ``i + o`` (the reference's ``pad_trace``), the distance to
its bin centre, and per bin the IDW weights or the nearest trace.  Everything ends in the CSR layout of ``p3d_bin_stack``."""
import math
import warnings

import numpy as np

from .transform import Affine

STACK_METHODS = ['average', 'median', 'nearest', 'IDW']


def distance(p1, p2):
    """Euclidean distance of two points, or row by row of two (N, 2) arrays."""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    if p1.shape != p2.shape:
        raise ValueError('points must have the same shape')
    if p1.ndim == 1:
        return np.sqrt((p2[0] - p1[0]) ** 2 + (p2[1] - p1[1]) ** 2)
    return np.sqrt((p2[:, 0] - p1[:, 0]) ** 2 + (p2[:, 1] - p1[:, 1]) ** 2)


def points_from_extent(extent):
    """(xmin, xmax, ymin, ymax) -> corner points (lower left, upper left, upper right, lower right)."""
    w, e, s, n = extent
    return np.array([[w, s], [w, n], [e, n], [e, s]], dtype=np.float64)


def extent_from_points(points):
    p = np.asarray(points)
    return (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max())


def polygon_area(pts):
    """Shoelace area of a closed polygon given by its vertices (N, 2)."""
    pts = np.asarray(pts, dtype=np.float64)
    x, y = pts[:, 0], pts[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, 1)) - np.dot(np.roll(x, 1), y))


def polygon_centroid(pts):
    """Area centroid of a polygon (N, 2)."""
    pts = np.asarray(pts, dtype=np.float64)
    x, y = pts[:, 0], pts[:, 1]
    cross = x * np.roll(y, 1) - np.roll(x, 1) * y
    return np.dot(pts.T + np.roll(pts.T, 1, axis=1), cross) / (6 * polygon_area(pts))


def _ceil_multiple(x, multiple):
    return type(x)(math.ceil(x / multiple) * multiple)


def adjust_extent(extent, spacing):
    """Widen (xmin, xmax, ymin, ymax) symmetrically so both sides are whole multiples of spacing (x: spacing[0], y: spacing[1])."""
    sx, sy = spacing
    dx, dy = extent[1] - extent[0], extent[3] - extent[2]
    px, py = _ceil_multiple(dx, sx) - dx, _ceil_multiple(dy, sy) - dy
    return (extent[0] - px / 2, extent[1] + px / 2, extent[2] - py / 2, extent[3] + py / 2)


def transform_and_adjust_extent(extent_pts, spacing, transform):
    """Corner points -> transformed bounding box adjusted to whole bins (integer spacings: corners rounded to integers first)."""
    pts = transform.transform(extent_pts)
    if all(isinstance(s, int) for s in spacing):
        pts = (pts + 0.5).astype('int').astype('float')
    return adjust_extent(extent_from_points(pts), spacing)


def affine_transform_coords_to_ilxl(extent, spacing, base_transform=None):
    """Affine map from coordinates to (iline, xline) numbers for a north-aligned ``extent`` with bins of ``spacing`` (il, xl) or a
    single size; the first bin centre maps to (1, 1).  ``base_transform`` (rotation into the aligned frame) is applied first."""
    corners = points_from_extent(extent)
    ysp, xsp = spacing if isinstance(spacing, (tuple, list)) else (spacing, spacing)
    centres = corners + np.array([[xsp / 2, ysp / 2], [xsp / 2, -ysp / 2], [-xsp / 2, -ysp / 2], [-xsp / 2, ysp / 2]])
    dist_x = distance(centres[0], centres[-1])
    dist_y = distance(centres[0], centres[1])
    n_il = int(np.around(dist_x / xsp, 0))
    n_xl = int(np.around(dist_y / ysp, 0))
    a = (Affine().translation(-centres[0]).scaling((1.0 / np.around(dist_x), 1.0 / np.around(dist_y))).scaling((n_il, n_xl))
         .translation((1, 1)))
    return a @ base_transform if base_transform is not None else a


def round_ilxl_extent(points):
    """Corner (il, xl) of the cube to integers: lower / left ends up, upper / right ends down."""
    eps = 1e-9
    nudge = np.array([[eps, eps], [eps, -eps], [-eps, -eps], [-eps, eps]])
    return np.around(points + nudge, 0).astype('int')


def find_nearest_ilxl(reference, values, return_index=False):
    """Nearest entry of the sorted ``reference`` for every value (midpoints in float32, ties to the lower entry)."""
    reference = np.asarray(reference)
    mids = reference[1:] - np.diff(reference.astype('f')) / 2
    idx = np.searchsorted(mids, values)
    return (reference[idx], idx) if return_index else reference[idx]


def get_cube_parameter(transform_forward, transform_reverse, xy, bin_size, cube_corner_pts, bin_size_region=None,
                       region_corner_pts=None, return_geometry=False):
    """Bins and trace assignment of the cube (reference cube_binning_3D.py:413-558).

    Returns ``bins`` (dict of il, xl (int32), x, y (float64) over the il-major grid), ``ilxl`` (int32 (N, 2), the bin of every point
    of ``xy``) and, with ``return_geometry``, ``(extent_cube, extent_cube_t)``, ``(extent_region, extent_region_t)`` and the region's
    outer bin centres."""
    use_region = region_corner_pts is not None
    if bin_size_region is None:
        bin_size_region = bin_size
    ext_cube_t = transform_and_adjust_extent(cube_corner_pts, bin_size_region if use_region else bin_size, transform_forward)
    ext_region_t = transform_and_adjust_extent(region_corner_pts, bin_size_region, transform_forward) if use_region else None
    cube_pts_t = points_from_extent(ext_cube_t)
    region_pts_t = points_from_extent(ext_region_t) if use_region else None

    to_ilxl = affine_transform_coords_to_ilxl(ext_region_t if use_region else ext_cube_t, bin_size_region if use_region else bin_size,
                                              base_transform=transform_forward)
    corners_ilxl = round_ilxl_extent(to_ilxl.transform(transform_reverse.transform(cube_pts_t)))
    il_range = (corners_ilxl[0, 0], corners_ilxl[-1, 0])
    xl_range = (corners_ilxl[0, 1], corners_ilxl[1, 1])
    il_step = 1 if bin_size[1] == bin_size_region[1] else bin_size[1] // bin_size_region[1]    # from the XLINE bin size
    xl_step = 1 if bin_size[0] == bin_size_region[0] else bin_size[0] // bin_size_region[0]    # from the ILINE bin size
    il_idx = np.arange(il_range[0], il_range[-1] + 1, il_step)
    xl_idx = np.arange(xl_range[0], xl_range[-1] + 1, xl_step)

    grid = np.asarray(np.meshgrid(il_idx, xl_idx)).T.reshape(-1, 2)     # il-major: (il0, xl0), (il0, xl1), ...
    grid_xy = to_ilxl.inverse().transform(grid)

    ilxl = to_ilxl.transform(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
    if use_region:
        cutoff = max(il_step, xl_step) / min(il_step, xl_step)
        for axis, step, idx in ((0, il_step, il_idx), (1, xl_step, xl_idx)):
            if step > 1:      # snap to the output lines of the coarser cube (the reference's rule, on the grid's own column)
                mapped = find_nearest_ilxl(grid[:, axis], ilxl[:, axis])
                keep = ((np.abs(ilxl[:, axis] - mapped) < cutoff + 1) & (ilxl[:, axis] >= idx[0] - cutoff / 2)
                        & (ilxl[:, axis] <= idx[-1] + cutoff / 2))
                ilxl[:, axis] = np.where(keep, mapped, ilxl[:, axis])
    ilxl = np.around(ilxl, 0).astype('int32')
    warnings.warn('\nCoordinates at the boundary between two ilines/xlines are assigned to the next SMALLER index (x.5 --> x)!')

    bins = {'il': grid[:, 0].astype('int32'), 'xl': grid[:, 1].astype('int32'), 'x': grid_xy[:, 0], 'y': grid_xy[:, 1]}
    if not return_geometry:
        return bins, ilxl
    ext_cube = transform_reverse.transform(cube_pts_t)
    if use_region:
        ext_region = transform_reverse.transform(region_pts_t)
        h = np.array([[bin_size_region[1] / 2, bin_size_region[0] / 2], [bin_size_region[1] / 2, -bin_size_region[0] / 2],
                      [-bin_size_region[1] / 2, -bin_size_region[0] / 2], [-bin_size_region[1] / 2, bin_size_region[0] / 2]])
        region_centres = transform_reverse.transform(region_pts_t + h)
    else:
        ext_region = region_centres = None
    return bins, ilxl, (ext_cube, ext_cube_t), (ext_region, ext_region_t), region_centres


def check_sampling_interval(dt_per_file):
    """One sampling interval (ms) for all files: the smallest of each file must agree (reference :41-49)."""
    d = np.asarray(dt_per_file, dtype=np.float64)
    lo, hi = float(d.min()), float(d.max())
    if np.mean((lo, hi)) != lo:
        raise ValueError(f'SEG-Y files with different sampling intervals (dt: {(lo, hi)})')
    return lo


def twt_axis(t0, t1, dt):
    """The cube's twt axis (ms): np.around(np.arange(t0, t1, dt), 5)."""
    return np.around(np.arange(t0, t1, dt, dtype=np.float64), 5)


def trace_shifts(delays, twt0, dt):
    """Output offset o of every trace (its sample i lands on cube sample i + o), pad_trace's rule: a trace that starts before the
    window loses round((twt0 - delay) / dt) samples at the top; one that starts inside it is padded by int((delay - twt0) / dt)."""
    d = np.asarray(delays, dtype=np.float64)
    early = d < twt0
    clip = np.round((twt0 - d) / dt)
    pad = np.trunc((d - twt0) / dt)
    return np.where(early, -clip, pad).astype(np.int64)


def idw_weights(dist, bin_id, factor):
    """Normalised inverse-distance weights d**-factor per bin (traces sorted by bin).  A bin with traces at distance 0 shares its
    weight equally among them (the reference divides inf by inf there)."""
    dist = np.asarray(dist, dtype=np.float64)
    with np.errstate(divide='ignore'):
        w = 1 / dist ** factor
    zero = dist == 0
    if zero.any():
        has_zero = np.zeros(int(bin_id.max()) + 1, bool)
        has_zero[bin_id[zero]] = True
        hz = has_zero[bin_id]
        w = np.where(hz, zero.astype(np.float64), w)
    starts = np.flatnonzero(np.r_[True, bin_id[1:] != bin_id[:-1]])
    sums = np.add.reduceat(w, starts)
    counts = np.diff(np.r_[starts, bin_id.size])
    return w / np.repeat(sums, counts)


def nearest_per_bin(dist, bin_id):
    """Index (into the bin-sorted arrays) of the nearest trace of every occupied bin; ties go to the first trace."""
    order = np.lexsort((np.arange(bin_id.size), dist, bin_id))
    first = np.r_[True, bin_id[order][1:] != bin_id[order][:-1]]
    return order[first]
