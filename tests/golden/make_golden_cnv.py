"""Fixtures of steps 9 and 16 (tests/golden/cnv.npz) from the REFERENCE's own check_coordinate_scalar (functions/header.py).

    python tests/golden/make_golden_cnv.py /path/to/reference

The reference's header module imports segyio at module level; an empty stand-in goes into ``sys.modules`` first.  The function is run unchanged.
Recorded per case: the requested scalar (as text; 'None' for None), the first x and y coordinate, and the pair it returned.  'auto' counts the
characters in front of the decimal point of the FIRST coordinate's text, so a minus sign counts as a digit; the cases cover 6, 7, 9 and 10
digits, negative and sub-unit coordinates, every fixed scalar, None and 0."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/reference'
sys.path.insert(0, REF)
sys.modules['segyio'] = types.ModuleType('segyio')

from pseudo_3D_interpolation.functions.header import check_coordinate_scalar  # noqa: E402

AUTO = [(123456.78, 5412345.6), (412345.25, 123456.5), (1234567.5, 7654321.25), (123456789.5, 1234.5), (1234567890.5, 12.25), (-23456.5, 1234.5),
        (-123456.75, -7654321.5), (0.25, 0.5), (-0.75, 0.125), (5.0, 9.5), (99999.0, 100000.0)]
cases = [('auto', x, y) for x, y in AUTO] + [(s, 412345.25, 5412345.5) for s in (-1000, -100, -10, 0, 10, 100, 1000, None)]
asked, xs, ys, scalars, mults = [], [], [], [], []
for want, x, y in cases:
    scalar, mult = check_coordinate_scalar(want, xcoords=np.array([[x, x + 1.0]]), ycoords=np.array([[y, y + 1.0]]))
    asked.append(str(want))
    xs.append(x)
    ys.append(y)
    scalars.append(float(scalar))
    mults.append(float(mult))
assert len({(s, m) for a, s, m in zip(asked, scalars, mults) if a == 'auto'}) >= 5          # the digit count matters
assert scalars[AUTO.index((-23456.5, 1234.5))] == scalars[AUTO.index((412345.25, 123456.5))]        # '-23456' counts six characters
np.savez(os.path.join(HERE, 'cnv.npz'), asked=np.array(asked), x=np.array(xs), y=np.array(ys), scalar=np.array(scalars), mult=np.array(mults))
for row in zip(asked, xs, ys, scalars, mults):
    print(*row)
