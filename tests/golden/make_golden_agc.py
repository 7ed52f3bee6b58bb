#!/opt/conda/bin/python3.9
"""Golden vectors for the step-15 automatic gain control, produced by the REFERENCE's own functions.

Run in the build container only (the reference does not travel):

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_golden_agc.py

``functions/signal.py`` and ``functions/utils.py`` import with NumPy / SciPy alone, so no stand-in module is needed (unlike
make_golden_helpers.py).  Recorded (data only, no source text):

  * ``AGC(x, win, kind, squared=...)`` for kind rms / mean / median x squared off / on x win 1, 10 (even), 31 (odd), 301 (> nt);
    on a 1-D trace, a 2-D profile (time on axis -1) and a 3-D slice-major cube (time on axis 0), each with all-zero traces;
    mean runs on positive data, rms and median on signed data;
  * ``AGC(..., return_gain_func=True)``: the gain functions of the 3-D cube at win 31;
  * ``get_AGC_samples(win, convert_twt(dt, units, 's'))`` for a table of (win, dt, units), including (0.01 s, 0.1 ms) -> 101.

The reference's AGC scales its argument in place (``x *= 1 / g``): every call gets a copy.
"""
import os

import numpy as np

from pseudo_3D_interpolation.functions.signal import AGC, get_AGC_samples
from pseudo_3D_interpolation.functions.utils import convert_twt

HERE = os.path.dirname(os.path.abspath(__file__))
NT = 200
KINDS = ("rms", "mean", "median")
WINS = (1, 10, 31, 301)


def inputs():
    rng = np.random.default_rng(15)
    signed = {
        "1d": rng.standard_normal(NT).astype(np.float32),
        "2d": rng.standard_normal((12, NT)).astype(np.float32),
        "3d": rng.standard_normal((NT, 5, 6)).astype(np.float32),
    }
    # ties for the median: a coarse grid of values in one profile row and one cube trace
    signed["2d"][3] = np.round(signed["2d"][3] * 2) / 2
    signed["3d"][:, 1, 2] = np.round(signed["3d"][:, 1, 2])
    positive = {k: (np.abs(v) + np.float32(0.05)).astype(np.float32) for k, v in signed.items()}
    for d in (signed, positive):          # all-zero traces
        d["2d"][5] = 0
        d["3d"][:, 2, 3] = 0
        d["3d"][:, 4, 0] = 0
    return signed, positive


AXIS = {"1d": -1, "2d": -1, "3d": 0}


def main():
    signed, positive = inputs()
    out = {}
    for shape in ("1d", "2d", "3d"):
        out[f"x/signed/{shape}"] = signed[shape]
        out[f"x/positive/{shape}"] = positive[shape]
    for shape in ("1d", "2d", "3d"):
        for kind in KINDS:
            x = positive[shape] if kind == "mean" else signed[shape]
            for sq in (False, True):
                for win in WINS:
                    y = AGC(x.copy(), win, kind=kind, squared=sq, axis=AXIS[shape])
                    assert y.dtype == np.float32 and y.shape == x.shape
                    out[f"y/{shape}/{kind}/{int(sq)}/{win}"] = y
    for kind in KINDS:
        x = positive["3d"] if kind == "mean" else signed["3d"]
        y, g = AGC(x.copy(), 31, kind=kind, return_gain_func=True, axis=0)
        out[f"gain/3d/{kind}/y"] = y
        out[f"gain/3d/{kind}/g"] = g
    table = [(0.01, 0.1, "ms"), (0.01, 1e-4, "s"), (0.05, 0.125, "ms"), (0.2, 1.0, "ms"), (0.02, 250.0, "us"), (0.1, 0.05, "ms"),
             (0.035, 0.25, "ms"), (0.5, 2.0, "ms")]
    win = np.array([t[0] for t in table])
    dt = np.array([t[1] for t in table])
    units = np.array([t[2] for t in table])
    dt_s = np.array([convert_twt(d, u, "s") for d, u in zip(dt, units)])
    out["samples/win"], out["samples/dt"], out["samples/units"], out["samples/dt_s"] = win, dt, units, dt_s
    out["samples/n"] = np.array([get_AGC_samples(w, d) for w, d in zip(win, dt_s)], np.int64)
    assert get_AGC_samples(0.01, 1e-4) == 101
    path = os.path.join(HERE, "agc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
