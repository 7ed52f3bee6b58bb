"""The persistent row pass of 1024-sample rows (row_pipe32_kernel) keeps its bits: SHA-256 digests of `out`, `done` and `sums` of small jobs
against tests/golden/row_pipe32_bits.json.

The digests were recorded ONCE, by this script, on the commit before the exchange reads of the transform were batched (the parent of the
commit that added this file), and are not recorded again when the kernels change: a change of schedule inside the row pass -- the order of
LDS reads, what is hoisted out of the unit loop -- must not change a single bit of what a job returns.
Recording command (GPU needed; writes the JSON, does not compare):

    python3 tests/test_gpu_row_pipe32_bits.py --record tests/golden/row_pipe32_bits.json

Jobs: nxl = 1024, 80 % of the traces missing, the slices of oracle.synthetic_slice with the seeds of tests/test_gpu_row_pass_no_sums.py, FOUR
iterations (a first, two steady-state and a last pass).  Shapes: 256 x 20 slices = 2560 units of two rows, one full trip of 2048 units and a
ragged second one on 256 compute units (on a device with another count the job gets more slices, so that it still exceeds one trip; slices are
independent, and the digests are taken over the first 20); 96 x 3 slices = 144 units, under one trip; 96 x 50 slices = 2400 units over two
trips with 48 units per slice, which does not divide a trip of 2048 (a wavefront changes its row pair from trip to trip).  complex64 cubes, and float32 cubes through the complex passes
(P3D_NO_REAL=1); hard and soft threshold; sparse spectra (the default) and dense ones (P3D_NO_SPARSE=1); with and without the cost sums.
Extra: the early exit (eps > 0) at four iterations as everywhere and at six, where a slice can stop before the last iteration and the
finalize pass runs; one APOCS job (alpha = 0.8; alpha = 1 everywhere else).

(A form of the kernel that keeps one row pair per wavefront and derives its tables once was built behind a switch, P3D_NO_ROWFIX, held to these
digests with the switch on and off, and left out again: it measured no faster, profiles/rowpass_batched_exchange.txt.  A later attempt runs every
case under both settings, as that one did.)
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "row_pipe32_bits.json")
KEEP = 20            # slices the digests cover (the recorded device ran exactly these)
SWITCHES = ("P3D_NO_REAL", "P3D_NO_SPARSE", "P3D_NO_PIPE32")


def _cases():
    """(id, nil, nslices, dtype, op, dense, want_sums, eps, niter, version, alpha)"""
    out = []
    for nil, n in ((256, 20), (96, 3)):
        for dt in ("c64", "f32"):
            for op in ("hard", "soft"):
                for dense in (False, True):
                    for sums in (True, False):
                        out.append((f"{nil}x{n}-{dt}-{op}-{'dense' if dense else 'sparse'}-{'sums' if sums else 'nosums'}", nil, n, dt, op, dense, sums, 0.0, 4, "regular", 1.0))
    out.append(("256x20-c64-hard-sparse-eps-4it", 256, 20, "c64", "hard", False, True, 0.25, 4, "regular", 1.0))
    out.append(("256x20-c64-hard-sparse-eps-6it", 256, 20, "c64", "hard", False, True, 0.25, 6, "regular", 1.0))
    out.append(("256x20-c64-hard-sparse-apocs", 256, 20, "c64", "hard", False, True, 0.0, 4, "adaptive", 0.8))
    out.append(("96x50-c64-hard-sparse-nosums", 96, 50, "c64", "hard", False, False, 0.0, 4, "regular", 1.0))
    return out


CASES = _cases()
_jobs = {}


def _slices(nil, n):
    """Slice count of the job: the 256 x 20 job must exceed one trip of 8 units per compute unit."""
    if (nil, n) != (256, 20):
        return n
    from pseudo_3d_interpolation_amd import _ffi as ffi
    cus = ffi.device_cus() if hasattr(ffi, "device_cus") else 256
    return max(n, (cus * 8) // (nil // 2) + 4)


def _job(nil, n):
    """(mask, complex64 cube), computed once per shape and never written to."""
    if (nil, n) not in _jobs:
        from oracle import pocs_oracle as orc
        mask = orc.synthetic_mask(nil, 1024, 0.8)
        cube = (np.stack([orc.synthetic_slice(nil, 1024, 700 + s) for s in range(n)]) * mask).astype(np.complex64)
        cube.setflags(write=False)
        _jobs[(nil, n)] = (mask, cube)
    return _jobs[(nil, n)]


def _digests(case, setenv):
    from pseudo_3d_interpolation_amd import _ffi as ffi
    from pseudo_3d_interpolation_amd.functions.POCS import _schedule_from_stats
    _, nil, n0, dt, op, dense, want_sums, eps, niter, version, alpha = case
    n = _slices(nil, n0)
    mask, cube = _job(nil, n)
    if dt == "f32":
        cube = np.ascontiguousarray(cube.real)
        setenv("P3D_NO_REAL", "1")
    if dense:
        setenv("P3D_NO_SPARSE", "1")
    dtype = ffi.P3D_F32 if dt == "f32" else ffi.P3D_C64
    maskf = mask.astype(np.float32)
    with ffi.Plan(nil, 1024, n) as plan:
        x, o, m = plan.alloc(cube.nbytes).upload(cube), plan.alloc(cube.nbytes), plan.alloc(maskf.nbytes).upload(maskf)
        st = plan.prime_dev(x.ptr, dtype, m.ptr, n)
        tau = _schedule_from_stats(st, nil * 1024, "exponential", niter, 0.99, 1e-2, "values")
        done, sums, _ = plan.run_dev(x.ptr, dtype, m.ptr, tau, niter, o.ptr, n, thresh_op=op, version=version, eps=eps, alpha=alpha, primed=True, want_sums=want_sums)
        got = o.download(cube.shape, cube.dtype)
        for b in (x, o, m):
            b.free()
    keep = min(KEEP, n0)
    done = np.ascontiguousarray(np.asarray(done, np.int32)[:keep])
    res = {"out": hashlib.sha256(np.ascontiguousarray(got[:keep]).tobytes()).hexdigest(), "done": hashlib.sha256(done.tobytes()).hexdigest()}
    if want_sums:
        res["sums"] = hashlib.sha256(np.ascontiguousarray(np.asarray(sums, np.float64)[:, :keep]).tobytes()).hexdigest()
    return res, done


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_row_pass_bits(case, golden, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    got, done = _digests(case, monkeypatch.setenv)
    print(case[0], got, "done", done.tolist())
    assert got == golden[case[0]], (case[0], list(done))


def _record(path):
    sys.path.insert(0, os.path.dirname(HERE))
    table = {}
    for case in CASES:
        for name in SWITCHES:
            os.environ.pop(name, None)
        table[case[0]], done = _digests(case, os.environ.__setitem__)
        print(case[0], table[case[0]]["out"][:16], "done", done.tolist(), flush=True)
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    _record(sys.argv[2])
