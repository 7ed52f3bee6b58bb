"""Windowed POCS as a composition of the oracle: ``oracle.pocs_oracle.pocs_slice`` per window in float64 and the tapered overlap-add blend in float64.
The geometry is restated here (not imported from the package under test): starts ``0, step, ...`` while ``start + w < n``, then ``n - w``; the taper
``0.5 - 0.5 cos(2 pi (i + 0.5) / w)`` ('hann') or ones ('boxcar'); ``out = sum_k W_k y_k / sum_k W_k`` over the active windows, 0 where there is none."""
import numpy as np

from oracle import pocs_oracle as orc


def starts(n, w, o):
    out, s = [], 0
    while s + w < n:
        out.append(s)
        s += w - o
    return out + [n - w]


def taper(w, kind):
    if kind == "boxcar":
        return np.ones(w)
    assert kind == "hann"
    return 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(w) + 0.5) / w)


def windows(shape2d, w, o):
    """[(start_il, start_xl)] in window order (iline-major)."""
    return [(a, b) for a in starts(shape2d[0], w[0], o[0]) for b in starts(shape2d[1], w[1], o[1])]


def pair(v):
    return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def patch_cube(cube, w, o):
    """The windows of every slice, job-major: [nslices * npatch][w_il][w_xl]."""
    w, o = pair(w), pair(o)
    wins = windows(cube.shape[1:], w, o)
    return np.stack([cube[s, a:a + w[0], b:b + w[1]] for s in range(cube.shape[0]) for a, b in wins])


def pocs_windowed(cube, mask, patch_shape, patch_overlap=None, patch_taper="hann", slice_fn=None, **kw):
    """(out, infos, jobs): the blended cube in the oracle's precision (complex128 / float64), per slice a list of the windows' info dicts, and the un-blended
    window results, job-major.  ``slice_fn(x, mask, info=..., **kw)``: the oracle of one job (default ``pocs_slice``: FFT)."""
    fn = orc.pocs_slice if slice_fn is None else slice_fn
    cube = np.asarray(cube)
    cube = cube.astype(np.complex128 if np.iscomplexobj(cube) else np.float64)
    mask = np.asarray(mask)
    w = pair(patch_shape)
    o = (w[0] // 2, w[1] // 2) if patch_overlap is None else pair(patch_overlap)
    wins = windows(cube.shape[1:], w, o)
    W = np.outer(taper(w[0], patch_taper), taper(w[1], patch_taper))
    out = np.zeros_like(cube)
    infos, jobs = [], []
    for s in range(cube.shape[0]):
        num = np.zeros(cube.shape[1:], cube.dtype)
        den = np.zeros(cube.shape[1:], np.float64)
        row = []
        for a, b in wins:
            x = cube[s, a:a + w[0], b:b + w[1]].copy()
            m = (mask[s] if mask.ndim == 3 else mask)[a:a + w[0], b:b + w[1]]
            info = {}
            y = np.array(fn(x, m, info=info, **kw))
            row.append(info)
            jobs.append(y)
            if info["niterations"] == 0:   # an all-zero window: inactive, no part in the blend
                continue
            num[a:a + w[0], b:b + w[1]] += W * y
            den[a:a + w[0], b:b + w[1]] += W
        covered = den > 0
        out[s][covered] = num[covered] / den[covered]
        infos.append(row)
    return out, infos, np.stack(jobs)


def slice_results(infos):
    """The per-slice ``results`` rows of a windowed job from the windows' infos: maxima over the active windows."""
    rows = []
    for row in infos:
        live = [i for i in row if i["niterations"]]
        k = max((i["niterations"] for i in live), default=0)
        rows.append({
            "niterations": k,
            "cost": max((i["costs"][-1] for i in live), default=0),
            "costs": [max(i["costs"][j] for i in live if i["niterations"] > j) for j in range(k)] if k else [0],
            "patches": [(i["niterations"], i["costs"][-1] if i["niterations"] else 0) for i in row],
        })
    return rows
