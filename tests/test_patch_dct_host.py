"""The routing of windowed DCT jobs in ``functions.POCS._pocs_cube_patched``, without a GPU: the library is replaced by fakes that record which loop a job
was sent to.  A DCT job goes to the single-kernel DCT loop exactly when ``PatchPlan.route(..., transform='DCT', norm=...)`` takes it; percentile operators,
APOCS and everything else the route refuses run the plan's generic DCT loop on the patch cube with one materialised mask window per job, as before;
``data-driven`` raises for DCT before anything is uploaded, as before; FFT jobs ask the route without the new arguments, as before."""
import ctypes
import os

import numpy as np
import pytest

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import POCS as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeBuf:
    ptr = 0

    def __init__(self, log):
        self.log = log

    def upload(self, arr):
        return self

    def download(self, shape, dtype):
        return np.zeros(shape, dtype)

    def download_into(self, dst):
        dst[...] = 0

    def free(self):
        pass


class FakePlan:
    handle = 1

    def __init__(self, nil, nxl, log):
        self.nil, self.nxl, self.log = nil, nxl, log

    def alloc(self, nbytes):
        return FakeBuf(self.log)

    def _loop(self, name, niter, n, **kw):
        self.log.append((name, kw))
        return np.full(n, niter, np.int32), np.ones((niter + 1, n)), 0.0

    def run_dev(self, x_ptr, dt, mask_ptr, tau, niter, out_ptr, n, **kw):
        return self._loop("plan.run_dev", niter, n, **kw)

    def dct_run_dev(self, x_ptr, dt, mask_ptr, tau, niter, out_ptr, n, **kw):
        return self._loop("plan.dct_run_dev", niter, n, **kw)


class FakePatchPlan:
    """The rule of p3d_patch_route / p3d_patch_dct_route on binary masks and a resident window shape."""
    test_hook = None
    log = None

    def __init__(self, plan, nil, nxl, s_il, s_xl, t_il, t_xl, step):
        self.plan, self.max_slices, self.npatch = plan, step, len(s_il) * len(s_xl)

    def close(self):
        pass

    def gather_dev(self, *a):
        pass

    def mask_dev(self, mask_ptr, mask_slices, nslices, windows_ptr=None):
        if windows_ptr is not None:
            self.log.append(("mask windows", {}))
        return False

    def route(self, thresh_op="hard", version="regular", **kw):
        self.log.append(("route", dict(kw, thresh_op=thresh_op, version=version)))
        return thresh_op in ("hard", "soft", "garrote") and version in ("regular", "fast") and kw.get("norm", "ortho") in (None, "backward", "ortho")

    def run_dev(self, patches_ptr, dt, tau, niter, out_ptr, nslices, **kw):
        return self.plan._loop("patch.run_dev", niter, nslices * self.npatch, **kw)

    def dct_run_dev(self, patches_ptr, dt, tau, niter, out_ptr, nslices, **kw):
        return self.plan._loop("patch.dct_run_dev", niter, nslices * self.npatch, **kw)

    def blend_dev(self, *a):
        pass


@pytest.fixture
def fakes(monkeypatch):
    log = []
    FakePatchPlan.log = log
    monkeypatch.setattr(P, "_get_plan", lambda w_il, w_xl, n, device, slot=0: FakePlan(w_il, w_xl, log))
    monkeypatch.setattr(P, "_plans", {})
    monkeypatch.setattr(_ffi, "PatchPlan", FakePatchPlan)
    monkeypatch.setattr(P, "_tau_of_batch", lambda kind, job, nil, nxl, dct_norm=None: (lambda plan, chunk, x_ptr, dt, n, active: np.ones((n, job.niter), np.complex128)))
    return log


def _run(**kw):
    x = np.ones((2, 40, 48), np.complex64)
    args = dict(niter=3, thresh_op="soft", thresh_model="linear", eps=0, p_max=0.9, p_min=0.1, patch_shape=32, patch_overlap=16)
    args.update(kw)
    return P.pocs_cube(x, np.ones((40, 48), np.float32), **args)


def _names(log):
    return [n for n, _ in log]


@pytest.mark.parametrize("norm", ["ortho", "backward"])
@pytest.mark.parametrize("version", ["regular", "fast"])
def test_a_routed_dct_job_runs_the_single_kernel_dct_loop(fakes, norm, version):
    _run(transform_kind="DCT", dct_norm=norm, version=version)
    assert _names(fakes) == ["route", "patch.dct_run_dev"]
    assert fakes[0][1] == dict(thresh_op="soft", version=version, transform="DCT", norm=norm)
    assert fakes[1][1]["norm"] == norm and fakes[1][1]["thresh_op"] == "soft" and fakes[1][1]["version"] == version and "mask_per_slice" not in fakes[1][1]


@pytest.mark.parametrize("kw", [dict(thresh_op="hard-percentile", thresh_model="linear", decay_kind="factors", p_max=97.0, p_min=60.0), dict(version="adaptive", alpha=0.8)],
                         ids=["percentile", "apocs"])
def test_what_the_route_refuses_runs_the_generic_dct_loop_as_before(fakes, kw):
    _run(transform_kind="DCT", dct_norm="ortho", **kw)
    assert _names(fakes) == ["route", "mask windows", "plan.dct_run_dev"]
    assert fakes[2][1]["norm"] == "ortho" and fakes[2][1]["mask_per_slice"] is True


def test_fft_jobs_ask_the_route_as_before(fakes):
    _run()
    assert fakes == [("route", dict(thresh_op="soft", version="regular")), fakes[1]] and fakes[1][0] == "patch.run_dev" and "norm" not in fakes[1][1]
    del fakes[:]
    _run(version="adaptive", alpha=0.8)
    assert _names(fakes) == ["route", "mask windows", "plan.run_dev"]


def test_data_driven_raises_for_dct_before_anything_is_uploaded(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the device")
    for name in ("Plan", "PatchPlan", "lib"):
        monkeypatch.setattr(_ffi, name, boom)
    with pytest.raises(NotImplementedError, match="data-driven"):
        _run(transform_kind="DCT", thresh_model="data-driven")


def test_route_wrapper_refuses_unknown_names_without_the_library(monkeypatch):
    """``PatchPlan.route`` answers False for an operator, transform or norm the library has no code for, before calling it."""
    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_ffi, "lib", boom)
    pp = object.__new__(_ffi.PatchPlan)
    pp.handle = None
    assert not pp.route("no-such-operator", transform="DCT", norm="ortho")
    assert not pp.route("soft", transform="WAVELET")
    assert not pp.route("soft", transform="DCT", norm="forward")


def test_library_exports_the_dct_patch_entries():
    if not os.path.isfile(_ffi.LIB_PATH):
        pytest.skip("needs the built library")
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "p3d.h")).read()
    for name in ("p3d_patch_dct_route", "p3d_patch_dct_run_dev"):
        assert hasattr(lib, name) and name in _ffi.PROTOTYPES and f"{name}(" in header, name
    assert lib.p3d_abi_version() == 1
    one = ctypes.c_int(7)
    assert lib.p3d_patch_dct_route(None, None, 0, ctypes.byref(one)) == _ffi.P3D_ERR_INVALID      # a NULL plan is an argument error, and needs no device
