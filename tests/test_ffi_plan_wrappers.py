"""The six plan classes of _ffi.py against a fake library: what each wrapper hands to its C entry (entry name, dtype code, mask bytes, threshold
table, `active` bytes, PocsParams, NULL sums) and what it returns.  No GPU and no built library: `_ffi.lib` is replaced by an object whose entries
record their arguments and return P3D_OK; the plans are made with object.__new__ and the few attributes the wrappers read."""
import ctypes as C

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi

NIL, NXL, N, NITER, NSH, NLEV = 4, 6, 2, 2, 3, 2
HANDLE = 0x1234


def _addr(v):
    return v.value if hasattr(v, "value") else v


class FakeLib:
    """Every attribute is an entry that records (name, args) and returns P3D_OK.  The *_run entries share one signature -- (plan, x, dtype, mask, tau,
    active, prm, out, n, niter_done, sums, elapsed_ms) -- and read their tables while the call is live; `width` thresholds per slice and iteration,
    `mask_dtype` float32 / float64."""

    def __init__(self, width=1, mask_dtype=np.float32):
        self.calls, self.width, self.mask_dtype = [], width, np.dtype(mask_dtype)

    def __getattr__(self, name):
        def entry(*args):
            rec = {"name": name, "args": args}
            if name.endswith("_run") or name.endswith("_run_dev"):
                prm = args[6]._obj
                n, niter = args[8], prm.niter
                rec["handle"], rec["dtype"], rec["n"] = _addr(args[0]), args[2], n
                rec["x"], rec["out"] = _addr(args[1]), _addr(args[7])
                rec["mask"] = np.frombuffer(C.string_at(_addr(args[3]), NIL * NXL * self.mask_dtype.itemsize), self.mask_dtype).reshape(NIL, NXL)
                rec["tau"] = np.frombuffer(C.string_at(_addr(args[4]), n * niter * self.width * 16), np.float64).reshape(n, niter, self.width, 2)
                rec["active"] = None if args[5] is None else C.string_at(_addr(args[5]), n)
                rec["prm"] = (prm.niter, prm.thresh_op, prm.version, prm.flags, prm.eps, prm.alpha)
                rec["sums_null"] = args[10] is None
            self.calls.append(rec)
            return _ffi.P3D_OK
        return entry

    def named(self, name):
        return [c for c in self.calls if c["name"] == name]


# class -> (attributes beyond nil / nxl / max_slices / device / handle, run entry, stats entry, destroy entry, thresholds per slice and iteration,
#           tau shape after (n, niter), mask dtype, stats shape after n)
CASES = {
    "Plan": ({}, "p3d_pocs_run", "p3d_pocs_stats", "p3d_plan_destroy", 1, (), np.float32, (6,)),
    "Plan64": ({}, "p3d_pocs64_run", "p3d_pocs64_stats", "p3d_plan64_destroy", 1, (), np.float64, (6,)),
    "WaveletPlan": ({"nlev": NLEV}, "p3d_wavelet_run", "p3d_wavelet_stats", "p3d_wavelet_plan_destroy", NLEV * 3, (NLEV, 3), np.float32, (NLEV, 3, 4)),
    "WaveletPlan64": ({"nlev": NLEV}, "p3d_wavelet64_run", "p3d_wavelet64_stats", "p3d_wavelet64_plan_destroy", NLEV * 3, (NLEV, 3), np.float64, (NLEV, 3, 4)),
    "ShearletPlan": ({"nsh": NSH}, "p3d_shearlet_run", "p3d_shearlet_stats", "p3d_shearlet_plan_destroy", NSH, (NSH,), np.float32, (NSH, 5)),
    "ShearletPlan64": ({"nsh": NSH}, "p3d_shearlet64_run", "p3d_shearlet64_stats", "p3d_shearlet64_plan_destroy", NSH, (NSH,), np.float64, (NSH, 5)),
}
DOUBLE = ("Plan64", "WaveletPlan64", "ShearletPlan64")


@pytest.fixture(params=sorted(CASES))
def case(request, monkeypatch):
    name = request.param
    extra, run_entry, stats_entry, destroy_entry, width, tshape, mdt, sshape = CASES[name]
    fake = FakeLib(width, mdt)
    monkeypatch.setattr(_ffi, "lib", lambda: fake)
    plan = object.__new__(getattr(_ffi, name))
    plan.nil, plan.nxl, plan.max_slices, plan.device, plan.handle = NIL, NXL, N, 0, C.c_void_p(HANDLE)
    for k, v in extra.items():
        setattr(plan, k, v)
    yield name, plan, fake, run_entry, stats_entry, destroy_entry, width, tshape, np.dtype(mdt), sshape
    plan.handle = None   # (nothing to destroy)


def _cube(dtype, n=N):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, NIL, NXL))
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal((n, NIL, NXL))
    return x.astype(dtype)


MASK = (np.arange(NIL * NXL).reshape(NIL, NXL) % 3 != 0).astype(np.int64)   # (an integer mask: the wrapper converts it)


def test_run_marshals_dtype_mask_and_returns(case):
    name, plan, fake, run_entry, *_, width, tshape, mdt, _s = case
    double = name in DOUBLE
    # dtype code handed over for each input type: the float32 plans narrow double-precision cubes, the others keep all four
    codes = {np.float32: _ffi.P3D_F32, np.complex64: _ffi.P3D_C64, np.float64: _ffi.P3D_F64 if double else _ffi.P3D_F32,
             np.complex128: _ffi.P3D_C128 if double else _ffi.P3D_C64}
    assert (_ffi.P3D_C64, _ffi.P3D_F32, _ffi.P3D_C128, _ffi.P3D_F64) == (0, 1, 2, 3)
    for dt, code in codes.items():
        fake.calls.clear()
        out, done, sums, ms = plan.run(_cube(dt), MASK, 0.5, NITER)
        (call,) = fake.calls
        assert call["name"] == run_entry and call["handle"] == HANDLE and call["n"] == N
        assert call["dtype"] == code
        out_dt = np.dtype(dt) if double else np.dtype(np.complex64 if np.dtype(dt).kind == "c" else np.float32)
        assert out.shape == (N, NIL, NXL) and out.dtype == out_dt and call["out"] == out.ctypes.data
        assert done.shape == (N,) and done.dtype == np.int32
        assert sums.shape == (NITER + 1, N) and sums.dtype == np.float64 and not call["sums_null"]
        assert isinstance(ms, float)
        assert call["mask"].dtype == mdt and np.array_equal(call["mask"], MASK.astype(mdt))
        assert call["active"] is None
        assert call["prm"] == (NITER, 0, 0, 0, 0.0, 1.0)
    # a single slice may come as a 2-D array
    fake.calls.clear()
    out = plan.run(_cube(np.float32)[0], MASK, 0.5, NITER)[0]
    assert out.shape == (1, NIL, NXL) and fake.calls[0]["n"] == 1


def test_run_threshold_tables(case):
    name, plan, fake, run_entry, _st, _de, width, tshape, _m, _s = case
    x = _cube(np.complex64)
    # a real scalar
    plan.run(x, MASK, 0.25, NITER)
    t = fake.calls[-1]["tau"]
    assert t.shape == (N, NITER, width, 2) and np.all(t[..., 0] == 0.25) and np.all(t[..., 1] == 0.0)
    # a real array that needs broadcasting: one value per iteration, every slice (and every level / shearlet)
    per_iter = np.array([3.0, 1.5]).reshape((NITER,) + (1,) * len(tshape))
    plan.run(x, MASK, per_iter, NITER)
    t = fake.calls[-1]["tau"]
    assert np.all(t[:, 0, :, 0] == 3.0) and np.all(t[:, 1, :, 0] == 1.5) and np.all(t[..., 1] == 0.0)
    # a complex array of the full shape
    full = (np.arange(N * NITER * width) + 1j * (100 + np.arange(N * NITER * width))).reshape((N, NITER) + tshape)
    plan.run(x, MASK, full, NITER)
    t = fake.calls[-1]["tau"]
    assert np.array_equal(t[..., 0].ravel(), np.arange(N * NITER * width, dtype=np.float64))
    assert np.array_equal(t[..., 1].ravel(), 100.0 + np.arange(N * NITER * width))
    assert all(c["name"] == run_entry for c in fake.calls)


def test_run_active_and_params(case):
    name, plan, fake, *_ = case
    x = _cube(np.complex64)
    plan.run(x, MASK, 0.5, NITER, thresh_op="soft", version="adaptive", eps=1e-3, alpha=0.75, active=[True, False])
    call = fake.calls[-1]
    assert call["active"] == b"\x01\x00"
    assert call["prm"] == (NITER, 1, 2, 0, 1e-3, 0.75)
    plan.run(x, MASK, 50.0, NITER, thresh_op="hard-percentile", version="fast")
    assert fake.calls[-1]["prm"] == (NITER, 16, 1, 0, 0.0, 1.0)
    plan.run(x, MASK, 0.5, NITER, thresh_op="garrote")
    assert fake.calls[-1]["prm"][1] == 2
    n_before = len(fake.calls)
    with pytest.raises(_ffi.UnsupportedError):
        plan.run(x, MASK, 0.5, NITER, thresh_op="nonsense")
    assert len(fake.calls) == n_before   # refused before any call


def test_run_dev_passes_pointers_through(case):
    name, plan, fake, run_entry, _st, _de, width, tshape, mdt, _s = case
    dev_entry = "p3d_pocs_run_dev" if name == "Plan" else run_entry
    x = _cube(np.complex64)
    m = np.ascontiguousarray(MASK, dtype=mdt)
    out = np.empty_like(x)
    res = plan.run_dev(x.ctypes.data, _ffi.P3D_C64, m.ctypes.data, 0.5, NITER, out.ctypes.data, N, thresh_op="soft", eps=0.5, active=np.array([0, 1]))
    done, sums, ms = res
    (call,) = fake.calls
    assert call["name"] == dev_entry and call["handle"] == HANDLE and call["dtype"] == _ffi.P3D_C64 and call["n"] == N
    assert call["x"] == x.ctypes.data and call["out"] == out.ctypes.data and np.array_equal(call["mask"], m)
    assert call["active"] == b"\x00\x01" and call["prm"] == (NITER, 1, 0, 0, 0.5, 1.0)
    assert call["tau"].shape == (N, NITER, width, 2) and np.all(call["tau"][..., 0] == 0.5)
    assert done.shape == (N,) and done.dtype == np.int32 and sums.shape == (NITER + 1, N) and sums.dtype == np.float64 and isinstance(ms, float)
    with pytest.raises(_ffi.UnsupportedError):
        plan.run_dev(x.ctypes.data, _ffi.P3D_C64, m.ctypes.data, 0.5, NITER, out.ctypes.data, N, thresh_op="nonsense")
    assert len(fake.calls) == 1


def test_plan_run_dev_profile_primed_and_no_sums(monkeypatch):
    fake = FakeLib(1, np.float32)
    monkeypatch.setattr(_ffi, "lib", lambda: fake)
    plan = object.__new__(_ffi.Plan)
    plan.nil, plan.nxl, plan.max_slices, plan.device, plan.handle = NIL, NXL, N, 0, C.c_void_p(HANDLE)
    x, m = _cube(np.float32), MASK.astype(np.float32)
    out = np.empty_like(x)
    done, sums, ms = plan.run_dev(x.ctypes.data, _ffi.P3D_F32, m.ctypes.data, 0.5, NITER, out.ctypes.data, N, profile=True, primed=True, want_sums=False)
    call = fake.calls[-1]
    assert call["name"] == "p3d_pocs_run_dev" and call["dtype"] == _ffi.P3D_F32
    assert call["prm"] == (NITER, 0, 0, 3, 0.0, 1.0)      # P3D_FLAG_PROFILE | P3D_FLAG_PRIMED
    assert call["sums_null"] and sums is None and done.shape == (N,)
    plan.run_dev(x.ctypes.data, _ffi.P3D_F32, m.ctypes.data, 0.5, NITER, out.ctypes.data, N, primed=True)
    assert fake.calls[-1]["prm"][3] == 2 and not fake.calls[-1]["sums_null"]
    plan.run(x, MASK, 0.5, NITER, profile=True)
    assert fake.calls[-1]["name"] == "p3d_pocs_run" and fake.calls[-1]["prm"][3] == 1
    plan.handle = None


def test_stats_shapes_and_entries(case):
    name, plan, fake, _run, stats_entry, _de, _w, _t, _m, sshape = case
    st = plan.stats(_cube(np.float32))
    assert st.shape == (N,) + sshape and st.dtype == np.float64
    assert fake.calls[-1]["name"] == stats_entry and fake.calls[-1]["args"][2] == _ffi.P3D_F32 and fake.calls[-1]["args"][3] == N
    x = _cube(np.complex64)
    st = plan.stats_dev(x.ctypes.data, _ffi.P3D_C64, N)
    assert st.shape == (N,) + sshape and st.dtype == np.float64
    call = fake.calls[-1]
    assert call["name"] == ("p3d_pocs_stats_dev" if name == "Plan" else stats_entry)
    assert _addr(call["args"][1]) == x.ctypes.data and call["args"][2] == _ffi.P3D_C64 and call["args"][3] == N


def test_cube_refuses_wrong_shapes(case):
    name, plan, fake, *_ = case
    with pytest.raises(ValueError):
        plan._cube(np.zeros((N, NIL, NXL + 1), np.float32))
    with pytest.raises(ValueError):
        plan._cube(np.zeros((N + 1, NIL, NXL), np.float32))
    with pytest.raises(ValueError):
        plan._cube(np.zeros((NIL * NXL,), np.float32))
    with pytest.raises(ValueError):
        plan.run(_cube(np.float32), MASK[:, :-1], 0.5, NITER)    # the mask must have the slice's shape
    assert fake.calls == []
    xc, code = plan._cube(np.zeros((NIL, NXL), np.float32))
    assert xc.shape == (1, NIL, NXL) and xc.flags.c_contiguous and code == _ffi.P3D_F32


def test_close_destroys_once(case):
    name, plan, fake, _run, _st, destroy_entry, *_ = case
    with plan as entered:
        assert entered is plan
    assert [c["name"] for c in fake.calls] == [destroy_entry] and _addr(fake.calls[0]["args"][0]) == HANDLE
    plan.close()
    plan.__del__()
    assert len(fake.calls) == 1 and plan.handle is None
