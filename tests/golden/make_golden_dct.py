#!/usr/bin/env python3
"""
Generate tests/golden/dct.npz by running THE REFERENCE ITSELF with SciPy's DCT pair (transform_kind='DCT').

Needs a checkout of the reference on PYTHONPATH, like make_golden.py (whose `field` and `trace_mask` recipes it reuses): the reference's
POCS_algorithm is imported, fed with seeded inputs and `partial(scipy.fft.dctn, norm=...)` / `partial(scipy.fft.idctn, norm=...)`, and its outputs are
stored.  Nothing of the reference is copied -- the fixture holds inputs and expected outputs (data).

    PYTHONPATH=<reference checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_dct.py

Per case: x, mask, params, norm, out (the reference fed float32 / complex64), out_f64 (fed float64 / complex128), niter (both runs),
costs_f64.  Further: dctn / idctn input / output pairs of SciPy for both norms (small shapes; the test computes the pairs of its larger
shapes with SciPy itself -- they would not fit the size limit of a committed file) and schedules of the reference's
get_threshold_decay(..., 'DCT', ...) on stored spectra.

Interpreter used for the committed fixture: python3 3.10, NumPy 2.2.6, SciPy 1.15.3.
"""
import os
import sys
from functools import partial

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import scipy.fft  # noqa: E402

from pseudo_3D_interpolation.functions import POCS as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import field, trace_mask  # noqa: E402

SEED, MISSING = 5, 0.5
BASE = dict(eps=0, p_max=0.99, p_min=1e-3)
CASES = {
    # name: (nil, nxl, real, norm, params)
    "soft_lin": (48, 80, False, "ortho", dict(BASE, niter=12, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=1e-2)),
    # hard threshold deep into the floor: a decision of the float32-fed run flips against the float64-fed one (spread 1e-4).  Kept on purpose: the
    # bound of its test is the reference's own spread
    "real_hard_exp": (64, 64, True, "ortho", dict(BASE, niter=12, thresh_op="hard", thresh_model="exponential")),
    "real_garrote_odd": (45, 63, True, "backward", dict(BASE, niter=10, thresh_op="garrote", thresh_model="exponential")),
    "fast": (64, 32, False, "ortho", dict(BASE, niter=10, thresh_op="soft", thresh_model="exponential", version="fast")),
    "adaptive": (32, 48, False, "ortho", dict(BASE, niter=10, thresh_op="soft", thresh_model="exponential", alpha=0.9, version="adaptive")),
    "pmin_adaptive_early": (32, 48, False, "ortho", dict(niter=10, thresh_op="soft", thresh_model="exponential", eps=1e-4, p_max=0.99, p_min="adaptive")),
    "sqrt_decay": (24, 32, False, "backward", dict(BASE, niter=8, thresh_op="soft", thresh_model="exponential", sqrt_decay=True)),
    "factors": (24, 32, False, "ortho", dict(niter=8, thresh_op="soft", thresh_model="linear", decay_kind="factors", eps=0, p_max=2.0, p_min=0.01)),
    "alpha08": (24, 32, False, "ortho", dict(BASE, niter=8, thresh_op="garrote", thresh_model="exponential", alpha=0.8)),
    "hard_pct": (24, 32, False, "ortho", dict(niter=8, thresh_op="hard-percentile", thresh_model="linear", decay_kind="factors", eps=0, p_max=99.0, p_min=5.0)),
    "tiny_8x8": (8, 8, False, "backward", dict(BASE, niter=5, thresh_op="soft", thresh_model="exponential")),
    "niter1": (16, 16, False, "ortho", dict(BASE, niter=1, thresh_op="hard", thresh_model="exponential")),
    "cplx_hard_exp": (64, 64, False, "ortho", dict(BASE, niter=20, thresh_op="hard", thresh_model="exponential")),
}
PAIR_SHAPES = [(2, 3), (8, 8), (7, 12), (33, 20)]
NORMS = ("backward", "ortho")


def run_ref(x, mask, norm, params):
    info = {}
    path = os.path.join("/tmp", f"golden_dct_{os.getpid()}.out")
    if os.path.exists(path):
        os.remove(path)
    with np.errstate(all="ignore"):
        y = ref.POCS_algorithm(x, mask, transform=partial(scipy.fft.dctn, norm=norm), itransform=partial(scipy.fft.idctn, norm=norm),
                               transform_kind="DCT", results_dict=info, path_results=path, **params)
    with open(path) as f:
        parts = f.read().strip().split(";")
    os.remove(path)
    return y, int(info["niterations"]), np.array([float(p) for p in parts[2:]], dtype=np.float64)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    out, names, tight = {}, [], 0
    for name, (nil, nxl, real, norm, params) in CASES.items():
        m = trace_mask(nil, nxl, MISSING, SEED)
        xo = field(nil, nxl, SEED, real) * m
        xd = xo.astype(np.float64 if real else np.complex128)
        y_s, n_s, _ = run_ref(xo.copy(), m, norm, params)
        y_d, n_d, c_d = run_ref(xd.copy(), m, norm, params)
        assert y_d.dtype == xd.dtype, (name, y_d.dtype)   # (y_s: NumPy >= 2 widens the soft / garrote operators, FPOCS and APOCS to double)
        out[f"{name}_x"] = xo
        out[f"{name}_mask"] = m
        out[f"{name}_norm"] = np.array(norm, dtype="U16")
        out[f"{name}_out"] = y_s
        out[f"{name}_out_f64"] = y_d
        out[f"{name}_niter"] = np.array([n_s, n_d])
        out[f"{name}_costs_f64"] = c_d
        out[f"{name}_params"] = np.array([f"{k}={v!r}" for k, v in params.items()], dtype="U64")
        names.append(name)
        spread = rel_l2(y_s, y_d)
        tight += 5 * spread < 1e-5
        print(f"{name:20s} {nil}x{nxl} {norm:8s} out {y_s.dtype}/{y_d.dtype} niter {n_s}/{n_d} single-vs-double rel-L2 {spread:.2e}")
    # the 1e-5 bar of the golden test binds only where five times the reference's own spread stays below it
    assert tight >= 10, f"only {tight} cases have 5 x spread < 1e-5"
    assert out["pmin_adaptive_early_niter"][1] < CASES["pmin_adaptive_early"][4]["niter"], "the early exit did not trigger"
    out["names"] = np.array(names, dtype="U32")

    # SciPy's own pairs: a batch of 3 slices, the middle one all zero
    rng = np.random.default_rng(SEED)
    for (n1, n2) in PAIR_SHAPES:
        x = (rng.standard_normal((3, n1, n2)) + 1j * rng.standard_normal((3, n1, n2))).astype(np.complex64)
        x[1] = 0
        key = f"pair_{n1}x{n2}"
        out[key + "_x"] = x
        for norm in NORMS:
            out[f"{key}_{norm}_dctn"] = scipy.fft.dctn(x.astype(np.complex128), axes=(-2, -1), norm=norm)
            out[f"{key}_{norm}_idctn"] = scipy.fft.idctn(x.astype(np.complex128), axes=(-2, -1), norm=norm)
    out["pair_shapes"] = np.array(PAIR_SHAPES)

    # schedules of the reference on DCT spectra (host test of get_threshold_decay)
    idx = 0
    for sname, real in (("tiny_8x8", False), ("niter1", False)):
        X0 = scipy.fft.dctn(out[f"{sname}_x"].astype(np.complex128), norm="ortho")
        out[f"sched_X0_{sname}"] = X0
        for model in ("linear", "exponential", "exponential-2", "inverse_proportional"):
            for kind, p_max, p_min in (("values", 0.99, 1e-3), ("values", 0.99, "adaptive"), ("factors", 2.0, 0.01)):
                tau = ref.get_threshold_decay(model, 9, "DCT", p_max, p_min, X0, kind)
                out[f"sched{idx:02d}_tau"] = np.asarray(tau)
                out[f"sched{idx:02d}_meta"] = np.array([sname, model, kind, str(p_max), str(p_min), "9"], dtype="U32")
                idx += 1
    out["sched_count"] = np.array([idx])

    path = os.path.join(HERE, "dct.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "pocs.npz"))
    print(f"dct.npz: {size} bytes ({len(names)} cases, {tight} with 5 x spread < 1e-5); pocs.npz: {limit}")
    assert size < limit


if __name__ == "__main__":
    main()
