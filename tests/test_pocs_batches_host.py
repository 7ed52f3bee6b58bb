"""The batch routes of ``functions.POCS.pocs_cube`` against a fake library (no GPU, no built library; the pattern of test_select64_host.py and
test_ffi_plan_wrappers.py): which entries every batch of every route calls, in which order, on which pointers (device buffers or the caller's own
arrays), with which ``n``, flag word and ``active`` table -- and the exceptions and warnings the routing raises.  Every job is a cube of 5 slices at
``batch_slices=2`` (three batches, the last of one slice) whose slice 3 is all zeros, once with a shared mask and once with one mask per slice.  The
fake never transforms anything: a download fills its destination with the byte 0x3f."""
import ctypes as C
import warnings

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi

NS, NIL, NXL, STEP, NITER, NSH, NLEV = 5, 8, 12, 2, 3, 3, 2
BATCHES = ((0, 2), (2, 2), (4, 1))            # (first slice, slices)
ACTIVE = (b"\x01\x01", b"\x01\x00", b"\x01")  # slice 3 is empty
DEVICE_BASE = 0x7D0000000000                  # the fake's "device" addresses: never dereferenced
FILL = 0x3F
H2D, D2H = "p3d_memcpy_h2d", "p3d_memcpy_d2h"


def _addr(v):
    return v.value if hasattr(v, "value") else v


def _fill(ptr, arr):
    C.memmove(_addr(ptr), arr.ctypes.data, arr.nbytes)


class FakeLib:
    """Every attribute is an entry that records its name and what the tests look at, and returns P3D_OK.  Plan handles and device buffers get
    addresses of their own; the wavelet plans have 2 levels; the statistics entries fill their whole table with ones, the sort entries their peaks
    with 2 + 1j, the pick entries their picks with ones and their counts with 5.  ``fused``: the answer of p3d_shearlet64_fused_shape / _info."""

    def __init__(self, fused=0):
        self.events, self.fused, self.nsh, self._handles, self._buffers = [], fused, None, 0, 0

    def __getattr__(self, name):
        def entry(*args):
            rec = {"name": name}
            self.events.append(rec)
            if name.endswith("_create"):
                self._handles += 1
                args[0]._obj.value = 0x1000 * self._handles
                if "shearlet" in name:
                    self.nsh = args[4]
            elif name == "p3d_malloc":
                self._buffers += 1
                args[1]._obj.value = DEVICE_BASE + (self._buffers << 32)
            elif name == H2D:
                rec["dst"], rec["data"] = _addr(args[1]), C.string_at(_addr(args[2]), args[3])
            elif name == D2H:
                rec["dst"], rec["src"], rec["nbytes"] = _addr(args[1]), _addr(args[2]), args[3]
                C.memset(rec["dst"], FILL, args[3])
            elif name in ("p3d_wavelet_info", "p3d_wavelet64_info"):
                if args[1] is not None:
                    args[1]._obj.value = NLEV
            elif name == "p3d_shearlet64_info":
                args[1]._obj.value = self.fused
            elif name == "p3d_shearlet64_fused_shape":
                return self.fused
            elif "stats" in name or name == "p3d_pocs_prime_dev":
                n, table = (args[4], args[5]) if name == "p3d_pocs_prime_dev" else (args[3], args[4])
                per = NLEV * 3 * 4 if "wavelet" in name else self.nsh * 5 if "shearlet" in name else 6
                rec["x"], rec["dtype"], rec["n"], rec["extra"] = _addr(args[1]), args[2], n, args[5:]
                _fill(table, np.ones(n * per))
            elif name == "p3d_pocs_sorted_spectrum":
                rec["x"], rec["n"] = _addr(args[1]), args[2]
                _fill(args[3], np.tile(np.float32([2.0, 1.0]), args[2]))
            elif name == "p3d_pocs64_sorted_spectrum":
                rec["x"], rec["dtype"], rec["n"] = _addr(args[1]), args[2], args[3]
                _fill(args[4], np.tile([2.0, 1.0], args[3]))
            elif name.endswith("_data_driven_pick"):
                n, niter = args[1], args[2]
                _fill(args[4], np.ones(n * niter * 2, np.float64 if "64" in name else np.float32))
                _fill(args[5], np.full(n, 5, np.int64))
            elif name.endswith("_run") or name.endswith("_run_dev"):
                prm = args[6]._obj
                rec.update(x=_addr(args[1]), dtype=args[2], mask=_addr(args[3]), out=_addr(args[7]), n=args[8], flags=prm.flags, niter=prm.niter,
                           active=C.string_at(_addr(args[5]), args[8]), extra=args[12:])
            return _ffi.P3D_OK
        return entry

    def named(self, *names):
        return [e for e in self.events if e["name"] in names]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    return lib


@pytest.fixture
def P(fake, monkeypatch):
    """functions.POCS with empty caches on the fake library (and what the test put into them released again)."""
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    for cache in ("_plans", "_workers", "_batch_bufs", "_holders", "_shearlet_plans"):
        if hasattr(mod, cache):
            monkeypatch.setattr(mod, cache, {})
    monkeypatch.delenv("P3D_PRECISION", raising=False)
    yield mod
    mod.release_plans()


PSI = np.random.default_rng(3).random((NIL, NXL, NSH))
F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128

# route -> (cube dtype, keyword arguments, entries between the upload and the run entry, those of them that take the batch's pointer, run entry,
#           resident on the device, mask dtype of the plan, dtype code handed over, what the entries take behind the common arguments)
ROUTES = {
    "float32 DCT": (C64, dict(transform_kind="DCT"), ["p3d_pocs_dct_stats_dev"], "p3d_pocs_dct_run_dev", True, F32, _ffi.P3D_C64, (0,)),
    "float32 FFT data-driven": (C64, dict(thresh_model="data-driven"), ["p3d_pocs_sorted_spectrum", "p3d_pocs_data_driven_pick"], "p3d_pocs_run_dev",
                                True, F32, _ffi.P3D_C64, ()),
    "float32 FFT strided out": (F32, dict(out="strided"), ["p3d_pocs_stats_dev"], "p3d_pocs_run_dev", True, F32, _ffi.P3D_F32, ()),
    "float32 WAVELET": (F32, dict(transform_kind="WAVELET", wavelet="db2"), ["p3d_wavelet_stats"], "p3d_wavelet_run", True, F32, _ffi.P3D_F32, ()),
    "float32 SHEARLET": (C64, dict(transform_kind="SHEARLET", auxiliary_data=PSI), ["p3d_shearlet_stats"], "p3d_shearlet_run", True, F32, _ffi.P3D_C64, ()),
    "double FFT complex128": (C128, dict(), ["p3d_pocs64_stats"], "p3d_pocs64_run", True, F64, _ffi.P3D_C128, ()),
    "double FFT complex64 reference": (C64, dict(precision="reference"), ["p3d_pocs64_stats"], "p3d_pocs64_run", True, F64, _ffi.P3D_C64, ()),
    "double FFT data-driven": (C128, dict(thresh_model="data-driven"), ["p3d_pocs64_sorted_spectrum", "p3d_pocs64_data_driven_pick"], "p3d_pocs64_run",
                               True, F64, _ffi.P3D_C128, ()),
    "double DCT": (F64, dict(transform_kind="DCT", precision="reference", dct_norm="ortho"), ["p3d_pocs64_dct_stats"], "p3d_pocs64_dct_run", True, F64,
                   _ffi.P3D_F64, (1,)),
    "double WAVELET": (F64, dict(transform_kind="WAVELET", wavelet="db2"), ["p3d_wavelet64_stats"], "p3d_wavelet64_run", False, F64, _ffi.P3D_F64, ()),
    "double SHEARLET": (C128, dict(transform_kind="SHEARLET", auxiliary_data=PSI), ["p3d_shearlet64_stats"], "p3d_shearlet64_run", False, F64,
                        _ffi.P3D_C128, ()),
    # a single-precision cube on extents where the double-precision loop is the fused one takes it by default, as it is (no widening on the host)
    "double SHEARLET complex64 fused": (C64, dict(transform_kind="SHEARLET", auxiliary_data=PSI, fused=1), ["p3d_shearlet64_stats"], "p3d_shearlet64_run",
                                        False, F64, _ffi.P3D_C64, ()),
}


def _job(dtype, mask_dtype, per_slice):
    rng = np.random.default_rng(11)
    cube = rng.standard_normal((NS, NIL, NXL)) + 2.0
    if np.dtype(dtype).kind == "c":
        cube = cube + 1j * rng.standard_normal((NS, NIL, NXL))
    cube = np.ascontiguousarray(cube.astype(dtype))
    cube[3] = 0
    mask = (rng.random((NS, NIL, NXL) if per_slice else (NIL, NXL)) < 0.6).astype(mask_dtype)   # (the plan's own mask dtype: handed over as it is)
    return cube, mask


def _inside(addr, arr):
    base = arr if arr.base is None else arr.base
    return base.ctypes.data <= addr < base.ctypes.data + base.nbytes


@pytest.mark.parametrize("per_slice", [False, True], ids=["shared-mask", "mask-per-slice"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_batch_of_every_route(P, fake, route, per_slice):
    dtype, kw, between, run_entry, resident, mdt, code, extra = ROUTES[route]
    kw = dict(kw)
    fake.fused = kw.pop("fused", 0)
    cube, mask = _job(dtype, mdt, per_slice)
    backing = out = None
    if kw.get("out") == "strided":
        backing = np.full((NS, NIL, 2 * NXL), 7, dtype)
        kw["out"] = out = backing[:, :, ::2]
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = P.pocs_cube(cube, mask, niter=NITER, thresh_op="soft", eps=0, batch_slices=STEP, results=results, **kw)

    assert y.shape == cube.shape and y.dtype == cube.dtype and (out is None or y is out)
    assert len(results) == NS and all(set(r) == {"niterations", "runtime", "cost", "costs"} for r in results)
    assert not fake.named("p3d_pocs_prime_dev", "p3d_pocs_run", "p3d_pocs_stats")       # the batch routes, on raw pointers
    runs = [e for e in fake.events if e["name"].endswith("_run") or e["name"].endswith("_run_dev")]
    assert [r["name"] for r in runs] == [run_entry] * 3
    assert [r["n"] for r in runs] == [n for _, n in BATCHES]
    assert [r["active"] for r in runs] == list(ACTIVE)
    assert all(r["flags"] == (_ffi.P3D_FLAG_MASK_PER_SLICE if per_slice else 0) for r in runs)
    assert all(r["dtype"] == code and r["niter"] == NITER and r["extra"] == extra for r in runs)

    seen = fake.named(H2D, D2H, run_entry, *between)
    per = cube[0].nbytes
    mask_part = mask[0].nbytes if per_slice else 0
    if not resident:
        # host pointers: addresses inside the caller's cube and mask and inside the returned array; nothing is copied by the wrapper
        assert [e["name"] for e in seen] == (between + [run_entry]) * 3
        for (lo, n), batch in zip(BATCHES, np.split(np.array(seen), 3)):
            for e in batch:
                assert e["x"] == cube.ctypes.data + lo * per and e["n"] == n and e["dtype"] == code
            assert batch[-1]["mask"] == mask.ctypes.data + lo * mask_part
            assert batch[-1]["out"] == y.ctypes.data + lo * per
        return

    uploads = [H2D, H2D] if per_slice else [H2D]
    batch_names = uploads + between + [run_entry, D2H]
    assert [e["name"] for e in seen] == ([] if per_slice else [H2D]) + batch_names * 3
    if not per_slice:                                # the shared mask: once, before the first batch
        assert seen[0]["data"] == mask.tobytes()
        seen = seen[1:]
    x_dev, m_dev, o_dev = runs[0]["x"], runs[0]["mask"], runs[0]["out"]
    assert len({x_dev, m_dev, o_dev}) == 3 and min(x_dev, m_dev, o_dev) > DEVICE_BASE
    for (lo, n), batch in zip(BATCHES, np.split(np.array(seen), 3)):
        batch = list(batch)
        assert batch[0]["dst"] == x_dev and batch[0]["data"] == cube[lo:lo + n].tobytes()
        if per_slice:                                # ... one mask per slice: the batch's own part
            assert batch[1]["dst"] == m_dev and batch[1]["data"] == mask[lo:lo + n].tobytes()
        for e in batch[len(uploads):-2]:
            if "x" in e:                             # (the pick entries work on what the sort entry left in the plan)
                assert e["x"] == x_dev and e["n"] == n and e.get("dtype", code) == code and e.get("extra", extra) == extra
        run, down = batch[-2:]
        assert (run["x"], run["mask"], run["out"]) == (x_dev, m_dev, o_dev)
        assert down["src"] == o_dev and down["nbytes"] == n * per
        if out is None:
            assert down["dst"] == y.ctypes.data + lo * per          # straight into the result
        else:
            assert not _inside(down["dst"], backing)                # through an array of the wrapper's own and an assignment
    assert np.all(np.ascontiguousarray(y).view(np.uint8) == FILL)
    if backing is not None:
        assert np.all(backing[:, :, 1::2] == 7)


# ---- what the routing raises and warns about -----------------------------------------------------------------------------------------------------
KW = dict(niter=NITER, thresh_op="soft", eps=0)
PCT = dict(niter=NITER, thresh_model="linear", decay_kind="factors", p_max=97, p_min=60, eps=0)


def _no_runs(fake):
    return not [e for e in fake.events if "_run" in e["name"]]


@pytest.mark.parametrize("dtype", [C64, C128])
def test_psi_of_the_wrong_shape(P, fake, dtype):
    cube, mask = _job(dtype, F32, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with pytest.raises(ValueError, match=rf"^Psi must be \({NIL}, {NXL}, nshearlets\), got shape \({NXL}, {NIL}, {NSH}\)$"):
            P.pocs_cube(cube, mask, transform_kind="SHEARLET", auxiliary_data=np.ones((NXL, NIL, NSH)), **KW)
    assert _no_runs(fake)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_wavelet_with_factors_fails_as_the_reference_does(P, fake, dtype):
    cube, mask = _job(dtype, F32, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with pytest.raises(IndexError, match=r'^list index out of range \(decay_kind="factors" yields one tau per iteration, the WAVELET thresholding '
                                             r'needs one per level and detail\)$'):
            P.pocs_cube(cube, mask, transform_kind="WAVELET", wavelet="db2", decay_kind="factors", **KW)
        # (the inverse-proportional model does not read the end points: it runs)
        P.pocs_cube(cube, mask, transform_kind="WAVELET", wavelet="db2", decay_kind="factors", thresh_model="inverse-proportional", **KW)
    assert len(fake.named("p3d_wavelet64_run" if dtype is F64 else "p3d_wavelet_run")) == 1


@pytest.mark.parametrize("kind,extra", [("WAVELET", dict(wavelet="db2")), ("SHEARLET", dict(auxiliary_data=PSI))])
def test_percentile_operators_are_refused(P, fake, kind, extra):
    cube, mask = _job(C64, F32, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with pytest.raises(NotImplementedError, match=rf"^thresh_op 'hard-percentile' is not available for the {kind} transform$"):
            P.pocs_cube(cube, mask, transform_kind=kind, thresh_op="hard-percentile", **PCT, **extra)
    # a double-precision cube: the warning about the missing double-precision loop comes first
    with pytest.warns(RuntimeWarning, match=rf"implied by the complex128 cube, but the double-precision loop does not cover the {kind} transform: this call "
                                            r"runs the float32 kernels"):
        with pytest.raises(NotImplementedError, match=rf"not available for the {kind} transform$"):
            P.pocs_cube(cube.astype(C128), mask, transform_kind=kind, thresh_op="hard-percentile", **PCT, **extra)
    assert _no_runs(fake)


def test_shearlet_without_psi(P, fake):
    cube, mask = _job(C64, F32, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with pytest.raises(ValueError, match=r"^SHEARLET requires pre-computed shearlets in Fourier domain \(Psi\)$"):
            P.pocs_cube(cube, mask, transform_kind="SHEARLET", **KW)
    with pytest.warns(RuntimeWarning, match="does not cover the SHEARLET transform"):
        with pytest.raises(ValueError, match=r"requires pre-computed shearlets"):
            P.pocs_cube(cube.astype(C128), mask, transform_kind="SHEARLET", **KW)
    assert _no_runs(fake)


def test_the_three_warnings_and_the_kernels_that_run_then(P, fake):
    cube, mask = _job(C128, F32, False)
    text = (r"^double-precision arithmetic was %s, but the double-precision loop does not cover %s: this call runs the float32 kernels "
            r'\(pass precision="float32" to say so explicitly\)$')
    with pytest.warns(RuntimeWarning, match=text % ("implied by the complex128 cube", "the DCT transform")):
        y = P.pocs_cube(cube, mask, transform_kind="DCT", batch_slices=STEP, **KW)
    assert y.dtype == C128 and len(fake.named("p3d_pocs_dct_run_dev")) == 3 and not fake.named("p3d_pocs64_dct_run")
    assert all(e["dtype"] == _ffi.P3D_C64 for e in fake.named("p3d_pocs_dct_run_dev"))      # narrowed on the way in, widened on the way out
    assert [e["nbytes"] for e in fake.named(D2H)] == [n * NIL * NXL * 8 for _, n in BATCHES] and not any(_inside(e["dst"], y) for e in fake.named(D2H))
    fake.events.clear()
    with pytest.warns(RuntimeWarning, match=text % ("requested", "thresh_op='soft-percentile'")):
        P.pocs_cube(cube, mask, transform_kind="DCT", precision="reference", thresh_op="soft-percentile", **PCT)
    assert len(fake.named("p3d_pocs_dct_run_dev")) == 1 and not fake.named("p3d_pocs64_dct_run")
    fake.events.clear()
    wide = np.ones((1, 2, 5121), C64)
    with pytest.warns(RuntimeWarning, match=text % ("requested", r"slice extents above 5120 \(2 x 5121\)")):
        P.pocs_cube(wide, np.ones((2, 5121)), precision="reference", **KW)
    assert len(fake.named("p3d_pocs_prime_dev")) == 1 and len(fake.named("p3d_pocs_run_dev")) == 1 and not fake.named("p3d_pocs64_run")
