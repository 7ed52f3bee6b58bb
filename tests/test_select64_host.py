"""Host side of the order statistics in the double-precision FFT loop (no GPU): the library exports the new entries, _ffi.Plan64 has the wrappers and
hands the right tables over, and ``pocs_cube`` routes a complex128 FFT job with a percentile operator to ``p3d_pocs64_run`` without a warning while the
DCT job keeps its warning -- against a fake library, the pattern of test_ffi_plan_wrappers.py."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi

NIL, NXL, N, NITER = 4, 6, 2, 3
ENTRIES = ("p3d_pocs64_percentile", "p3d_pocs64_sorted_spectrum", "p3d_pocs64_data_driven_pick")
LIB = os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "libp3d_hip.so")


@pytest.mark.skipif(not os.path.isfile(LIB), reason="needs the built library (python -c 'import __graft_entry__ as g; g.build()')")
def test_library_exports_the_entry_points():
    import subprocess
    names = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.splitlines() if line}
    assert set(ENTRIES) <= names, sorted(set(ENTRIES) - names)


def _addr(v):
    return v.value if hasattr(v, "value") else v


class FakeLib:
    """Every attribute is an entry that records (name, args) and returns P3D_OK; the statistics entries fill their table with ones, the sort entry its
    peaks with 2 + 1j, the pick entry its counts with `count`."""

    def __init__(self, count=5):
        self.calls, self.count = [], count

    def __getattr__(self, name):
        def entry(*args):
            rec = {"name": name, "args": args}
            if name.endswith("_run"):
                prm = args[6]._obj
                rec["dtype"], rec["n"], rec["prm"] = args[2], args[8], (prm.niter, prm.thresh_op, prm.version, prm.flags)
                rec["tau"] = np.frombuffer(C.string_at(_addr(args[4]), args[8] * prm.niter * 16), np.float64).reshape(args[8], prm.niter, 2)
            elif "stats" in name:
                ones = np.ones(args[3] * 6)
                C.memmove(_addr(args[4]), ones.ctypes.data, ones.nbytes)
            elif name == "p3d_pocs64_sorted_spectrum":
                rec["dtype"], rec["n"] = args[2], args[3]
                peaks = np.tile([2.0, 1.0], args[3])
                C.memmove(_addr(args[4]), peaks.ctypes.data, peaks.nbytes)
            elif name == "p3d_pocs64_data_driven_pick":
                n, niter = args[1], args[2]
                rec["bounds"] = np.frombuffer(C.string_at(_addr(args[3]), n * 32), np.float64).reshape(n, 4)
                picks = np.arange(n * niter * 2, dtype=np.float64)
                C.memmove(_addr(args[4]), picks.ctypes.data, picks.nbytes)
                counts = np.full(n, self.count, np.int64)
                C.memmove(_addr(args[5]), counts.ctypes.data, counts.nbytes)
            elif name == "p3d_pocs64_percentile":
                rec["perc"] = np.frombuffer(C.string_at(_addr(args[3]), args[2] * 8), np.float64)
            self.calls.append(rec)
            return _ffi.P3D_OK
        return entry

    def named(self, name):
        return [c for c in self.calls if c["name"] == name]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    return lib


@pytest.fixture
def plan(fake):
    p = object.__new__(_ffi.Plan64)
    p.nil, p.nxl, p.max_slices, p.device, p.handle = NIL, NXL, N, 0, C.c_void_p(0x1234)
    yield p
    p.handle = None   # (nothing to destroy)


def test_plan64_wrappers_marshal_their_tables(plan, fake):
    x = np.ones((N, NIL, NXL), np.float32)
    assert np.array_equal(plan.sorted_spectrum(x), np.full(N, 2 + 1j)) and plan.sorted_spectrum(x).dtype == np.complex128
    call = fake.named("p3d_pocs64_sorted_spectrum")[0]
    assert (call["dtype"], call["n"]) == (_ffi.P3D_F32, N)                     # (the cube goes over in its own dtype)
    assert plan.sorted_spectrum_dev(0x4000, _ffi.P3D_C128, N).shape == (N,)
    assert fake.named("p3d_pocs64_sorted_spectrum")[-1]["args"][1].value == 0x4000
    picks, count = plan.data_driven_pick([1 + 2j, 3 + 4j], [5 + 6j, 7 + 8j], NITER)
    assert np.array_equal(fake.named("p3d_pocs64_data_driven_pick")[0]["bounds"], [[1, 2, 5, 6], [3, 4, 7, 8]])
    assert picks.dtype == np.complex128 and picks.shape == (N, NITER) and picks[1, 2] == 10 + 11j and np.array_equal(count, [5, 5])
    thr = plan.percentile(np.ones((N, NIL, NXL), np.complex64), 37.5)
    assert thr.shape == (N,) and np.array_equal(fake.named("p3d_pocs64_percentile")[0]["perc"], [37.5, 37.5])
    with pytest.raises(ValueError):
        plan.percentile(np.ones((N, NIL + 1, NXL)), 50.0)
    # Plan64.run hands the percentile flag over as Plan.run does
    plan.run(np.ones((N, NIL, NXL), np.complex128), np.ones((NIL, NXL)), 50.0, NITER, thresh_op="garrote-percentile")
    assert fake.named("p3d_pocs64_run")[0]["prm"][:2] == (NITER, _ffi.P3D_OP["garrote"] | 16)


@pytest.fixture
def P(fake, monkeypatch):
    """functions.POCS with empty plan caches on the fake library (and the caches it fills dropped again)."""
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    for cache in ("_plans", "_workers", "_batch_bufs", "_holders", "_shearlet_plans"):
        monkeypatch.setattr(mod, cache, {})
    monkeypatch.delenv("P3D_PRECISION", raising=False)
    yield mod
    mod.release_plans()


PCT = dict(niter=NITER, thresh_model="linear", decay_kind="factors", p_max=97, p_min=60, eps=0)


@pytest.mark.parametrize("op", ["hard-percentile", "soft-percentile", "garrote-percentile"])
@pytest.mark.parametrize("dtype,precision", [(np.complex128, None), (np.float64, None), (np.complex64, "reference")])
def test_fft_percentile_jobs_take_the_double_loop_without_a_warning(P, fake, op, dtype, precision):
    x = np.ones((N, NIL, NXL), dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = P.pocs_cube(x, np.ones((NIL, NXL)), thresh_op=op, precision=precision, **PCT)
    assert y.dtype == x.dtype
    (call,) = fake.named("p3d_pocs64_run")
    assert call["prm"][:2] == (NITER, _ffi.P3D_OP[op]) and _ffi.P3D_OP[op] & 16 and call["dtype"] == _ffi.Plan64._DT[np.dtype(dtype)] and call["n"] == N
    assert np.array_equal(call["tau"][..., 0], np.broadcast_to([97.0, 78.5, 60.0], (N, NITER)))   # the percentages are the schedule
    assert not fake.named("p3d_pocs_run_dev") and not fake.named("p3d_pocs_run")


def test_fft_extent_limit_is_the_only_warning_left(P, fake):
    x = np.ones((1, 2, 5121), np.complex64)
    with pytest.warns(RuntimeWarning, match=r"does not cover slice extents above 5120 \(2 x 5121\)"):
        P.pocs_cube(x, np.ones((2, 5121)), thresh_op="hard-percentile", precision="reference", **PCT)
    assert not fake.named("p3d_pocs64_run") and len(fake.named("p3d_pocs_run_dev")) == 1


def test_dct_percentile_jobs_still_warn_and_run_the_float32_kernels(P, fake):
    x = np.ones((N, NIL, NXL), np.complex128)
    with pytest.warns(RuntimeWarning, match="does not cover thresh_op='soft-percentile'"):
        P.pocs_cube(x, np.ones((NIL, NXL)), transform_kind="DCT", precision="reference", thresh_op="soft-percentile", **PCT)
    assert not fake.named("p3d_pocs64_run") and not fake.named("p3d_pocs64_dct_run") and len(fake.named("p3d_pocs_dct_run_dev")) == 1
    with pytest.warns(RuntimeWarning, match="does not cover the DCT transform"):   # (no precision='reference': the DCT warning as before)
        P.pocs_cube(x, np.ones((NIL, NXL)), transform_kind="DCT", thresh_op="soft", **PCT)


def test_data_driven_schedule_comes_from_the_plan64_sort(P, fake):
    x = np.ones((N, NIL, NXL), np.complex128)
    x[1] = 0                                                   # an empty slice: no picks wanted, none checked
    prm = dict(niter=NITER, thresh_op="soft", thresh_model="data-driven", p_max=0.5, p_min=0.25, eps=0)
    P.pocs_cube(x, np.ones((NIL, NXL)), **prm)
    (sort,), (pick,), (run,) = fake.named("p3d_pocs64_sorted_spectrum"), fake.named("p3d_pocs64_data_driven_pick"), fake.named("p3d_pocs64_run")
    assert sort["dtype"] == _ffi.P3D_C128 and not fake.named("p3d_pocs_sorted_spectrum")
    assert np.array_equal(pick["bounds"], np.broadcast_to([0.5, 0.25, 1.0, 0.5], (N, 4)))   # p * x_fwd.max() with x_fwd.max() = 2 + 1j
    assert np.array_equal(run["tau"][0], [[0, 1], [2, 3], [4, 5]]) and not run["tau"][1].any()
    fake.count = 0
    with pytest.raises(IndexError):                            # v[0] of an empty selection (POCS.py:360)
        P.pocs_cube(x, np.ones((NIL, NXL)), **prm)
