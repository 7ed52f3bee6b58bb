"""Host side of the double-precision DCT loop (no GPU): the built library exports its entry points, _ffi.Plan64 has the wrappers, and what the wrappers
refuse is refused before any call reaches the library -- against a fake library, the pattern of test_ffi_plan_wrappers.py."""
import ctypes as C
import os

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi

NIL, NXL, N, NITER = 4, 6, 2, 2
ENTRIES = ("p3d_dct2_c128", "p3d_pocs64_dct_stats", "p3d_pocs64_dct_run")
LIB = os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "libp3d_hip.so")


@pytest.mark.skipif(not os.path.isfile(LIB), reason="needs the built library (python -c 'import __graft_entry__ as g; g.build()')")
def test_library_exports_the_entry_points():
    import subprocess
    names = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.splitlines() if line}
    assert set(ENTRIES) <= names, sorted(set(ENTRIES) - names)


def test_plan64_has_the_wrappers():
    for name in ("dct2", "dct_stats_dev", "dct_run", "dct_run_dev"):
        assert callable(getattr(_ffi.Plan64, name)), name


class FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return _ffi.P3D_OK
        return entry


@pytest.fixture
def plan(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: fake)
    p = object.__new__(_ffi.Plan64)
    p.nil, p.nxl, p.max_slices, p.device, p.handle = NIL, NXL, N, 0, C.c_void_p(0x1234)
    yield p, fake
    p.handle = None   # (nothing to destroy)


def test_bad_norm_and_percentile_operator_raise_before_any_call(plan):
    p, fake = plan
    x = np.ones((N, NIL, NXL), np.complex128)
    m = np.ones((NIL, NXL), np.float64)
    out = np.empty_like(x)
    with pytest.raises(_ffi.UnsupportedError, match="norm"):
        p.dct2(x, norm="forward")
    with pytest.raises(_ffi.UnsupportedError, match="norm"):
        p.dct_stats_dev(x.ctypes.data, _ffi.P3D_C128, N, norm="forward")
    with pytest.raises(_ffi.UnsupportedError, match="norm"):
        p.dct_run(x, m, 0.5, NITER, norm="forward")
    with pytest.raises(_ffi.UnsupportedError, match="norm"):
        p.dct_run_dev(x.ctypes.data, _ffi.P3D_C128, m.ctypes.data, 0.5, NITER, out.ctypes.data, N, norm=3)
    for op in ("hard-percentile", "soft-percentile", "garrote-percentile", "nonsense"):
        with pytest.raises(_ffi.UnsupportedError, match="hard, soft and garrote"):
            p.dct_run(x, m, 50.0, NITER, thresh_op=op)
        with pytest.raises(_ffi.UnsupportedError, match="hard, soft and garrote"):
            p.dct_run_dev(x.ctypes.data, _ffi.P3D_C128, m.ctypes.data, 50.0, NITER, out.ctypes.data, N, thresh_op=op, norm="ortho")
    assert fake.calls == []


def test_wrappers_hand_entry_norm_and_dtype_over(plan):
    p, fake = plan
    x = np.ones((N, NIL, NXL), np.float32)
    m = np.ones((N, NIL, NXL), np.uint8)              # one mask per slice
    out, done, sums, ms = p.dct_run(x, m, 0.5, NITER, thresh_op="garrote", version="adaptive", alpha=0.9, norm="ortho")
    (name, args), = fake.calls
    assert name == "p3d_pocs64_dct_run" and args[2] == _ffi.P3D_F32 and args[8] == N and args[-1] == 1
    prm = args[6]._obj
    assert (prm.niter, prm.thresh_op, prm.version, prm.flags, prm.alpha) == (NITER, 2, 2, _ffi.P3D_FLAG_MASK_PER_SLICE, 0.9)
    assert out.dtype == np.float32 and out.shape == x.shape and sums.shape == (NITER + 1, N) and done.shape == (N,)
    X = p.dct2(np.ones((NIL, NXL)), inverse=True)
    name, args = fake.calls[-1]
    assert name == "p3d_dct2_c128" and args[3:] == (1, 1, 0) and X.shape == (NIL, NXL) and X.dtype == np.complex128
    st = p.dct_stats_dev(x.ctypes.data, _ffi.P3D_F32, N, norm="backward")
    name, args = fake.calls[-1]
    assert name == "p3d_pocs64_dct_stats" and args[2:4] == (_ffi.P3D_F32, N) and args[-1] == 0 and st.shape == (N, 6)
