"""Windowed POCS, everything that needs no GPU: the window geometry, the tapers, the argument errors (all raised before anything is uploaded), the unchanged
per-slice signature, the YAML keys of the step-13 driver, the route of the sharded entry and the C entry points."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import yaml

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import POCS as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import patch_numpy as pn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,w,o,want", [(64, 64, 32, [0]), (80, 32, 16, [0, 16, 32, 48]), (72, 32, 16, [0, 16, 32, 40]), (100, 32, 24, list(range(0, 68, 8)) + [68]),
                                         (45, 32, 8, [0, 13]), (33, 32, 0, [0, 1])])
def test_patch_starts(n, w, o, want):
    got = P.patch_starts(n, w, o)
    assert got == want == pn.starts(n, w, o)
    assert got[0] == 0 and got[-1] == n - w and all(b > a for a, b in zip(got, got[1:]))
    assert all(b - a <= w - o for a, b in zip(got, got[1:]))       # no gap wider than the step: every point is covered


@pytest.mark.parametrize("w", [1, 2, 31, 32, 64, 128])
def test_tapers_are_strictly_positive(w):
    hann, box = P.patch_taper(w, "hann"), P.patch_taper(w, "boxcar")
    assert hann.dtype == np.float64 and hann.shape == (w,) and np.all(hann > 0) and np.all(hann.astype(np.float32) > 0)
    assert np.allclose(hann, hann[::-1]) and np.allclose(hann, pn.taper(w, "hann"), rtol=0, atol=1e-15)
    assert np.array_equal(box, np.ones(w))


def _job(dtype=np.complex64, shape=(2, 40, 48)):
    x = np.ones(shape, dtype)
    return x, np.ones(shape[1:], np.float32)


@pytest.fixture
def no_upload(monkeypatch):
    """Every way onto the device raises: the errors below are raised before anything is uploaded."""
    def boom(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_ffi, "Plan", boom)
    monkeypatch.setattr(_ffi, "PatchPlan", boom)
    monkeypatch.setattr(_ffi, "lib", boom)


@pytest.mark.parametrize("kw", [dict(patch_shape=41), dict(patch_shape=(32, 49)), dict(patch_shape=32, patch_overlap=-1), dict(patch_shape=32, patch_overlap=32),
                                dict(patch_shape=(32, 16), patch_overlap=(8, 16)), dict(patch_shape=32, patch_taper="tukey"), dict(patch_shape=(32, 32, 32))])
def test_geometry_errors(no_upload, kw):
    x, m = _job()
    with pytest.raises(ValueError):
        P.pocs_cube(x, m, **kw)


@pytest.mark.parametrize("kw", [dict(transform_kind="WAVELET"), dict(transform_kind="SHEARLET", auxiliary_data=np.ones((40, 48, 3))), dict(precision="reference")])
def test_uncovered_jobs_name_the_argument(no_upload, kw):
    x, m = _job(np.float32)
    with pytest.raises(NotImplementedError, match="patch_shape"):
        P.pocs_cube(x, m, patch_shape=32, **kw)


@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
def test_double_cubes_name_the_argument(no_upload, dtype, monkeypatch):
    monkeypatch.delenv("P3D_PRECISION", raising=False)
    x, m = _job(dtype)
    with pytest.raises(NotImplementedError, match="patch_shape"):
        P.pocs_cube(x, m, patch_shape=32)


def test_the_per_slice_signature_is_the_references():
    names = ["x", "mask", "auxiliary_data", "transform", "itransform", "transform_kind", "niter", "thresh_op", "thresh_model", "eps", "alpha", "p_max", "p_min",
             "sqrt_decay", "decay_kind", "verbose", "version", "results_dict", "path_results"]
    assert list(inspect.signature(P.POCS_algorithm).parameters) == names
    for f in (P.POCS, P.FPOCS, P.APOCS):
        assert f.func is P.POCS_algorithm
    sig = inspect.signature(P.pocs_cube).parameters
    assert sig["patch_shape"].default is None and sig["patch_overlap"].default is None and sig["patch_taper"].default == "hann"


def _step13(tmp_path, monkeypatch, extra):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, save_cube
    n, nil, nxl = 3, 40, 48
    ds = Cube({"env": np.ones((n, nil, nxl), np.float32), "fold": np.ones((nil, nxl), np.int32)}, {"env": ("twt", "iline", "xline"), "fold": ("iline", "xline")},
              {"twt": np.arange(n) * 1.0, "iline": np.arange(nil), "xline": np.arange(nxl)}, {"history": "", "text": ""}, {}, {})
    path = save_cube(ds, str(tmp_path / "cube.npz"))
    meta = dict(transform_kind="fft", niter=4, eps=0, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=0.1, **extra)
    yml = tmp_path / "pocs.yml"
    yml.write_text(yaml.safe_dump(dict(dim="twt", var="env", batch_chunk=2, output_runtime_results=False, metadata=meta)))
    calls = []

    def fake(cube, mask, results=None, out=None, **kw):
        calls.append(kw)
        out[...] = cube
        return out
    monkeypatch.setattr(step13, "pocs_cube", fake)
    step13.main(["13", path, "--path_pocs_parameter", str(yml), "--path_output_dir", str(tmp_path / "out")])
    return calls, sorted(os.listdir(tmp_path / "out"))


def test_step13_yaml_keys_reach_pocs_cube(tmp_path, monkeypatch):
    calls, names = _step13(tmp_path, monkeypatch, dict(patch_shape=[32, 16], patch_overlap=8, patch_taper="boxcar"))
    assert calls and all(kw["patch_shape"] == [32, 16] and kw["patch_overlap"] == 8 and kw["patch_taper"] == "boxcar" for kw in calls)
    batch_files = [f for f in names if f.endswith(".npz")]
    assert batch_files and all(f.startswith("cube_FFT_soft_niter-4_patch-32x16_") for f in batch_files)
    with open(tmp_path / "out" / "parameter_cube_FFT_soft_niter-4.yml") as fh:
        written = yaml.safe_load(fh)
    assert written["patch_shape"] == [32, 16] and written["patch_overlap"] == 8 and written["patch_taper"] == "boxcar"


def test_step13_prefix_is_unchanged_without_the_keys(tmp_path, monkeypatch):
    calls, names = _step13(tmp_path, monkeypatch, {})
    assert calls and all("patch_shape" not in kw for kw in calls)
    batch_files = [f for f in names if f.endswith(".npz")]
    assert batch_files and all(f.startswith("cube_FFT_soft_niter-4_0") and "patch" not in f for f in batch_files)


def test_step13_one_int_for_both_axes(tmp_path, monkeypatch):
    _, names = _step13(tmp_path, monkeypatch, dict(patch_shape=32))
    assert any(f.startswith("cube_FFT_soft_niter-4_patch-32x32_") for f in names)


def test_sharded_entry_sends_a_patch_job_through_pocs_cube(monkeypatch):
    torch = pytest.importorskip("torch")
    from pseudo_3d_interpolation_amd import sharding
    seen = []

    def fake(block, mask, device=0, **params):
        seen.append(params)
        return np.asarray(block) * 2

    monkeypatch.setattr(P, "pocs_cube", fake)
    monkeypatch.setattr(sharding, "_upload", lambda arr, dev: torch.from_numpy(arr))
    x, m = _job()
    out = sharding.pocs_block_on_device(x, m, patch_shape=32, patch_overlap=16, thresh_op="soft")
    assert len(seen) == 1 and seen[0]["patch_shape"] == 32 and seen[0]["patch_overlap"] == 16
    assert np.array_equal(out.numpy(), x * 2)


def test_library_exports_the_patch_entries():
    if not os.path.isfile(_ffi.LIB_PATH):
        pytest.skip("needs the built library")
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    names = ["p3d_patch_plan_create", "p3d_patch_plan_destroy", "p3d_patch_plan_info", "p3d_patch_gather_dev", "p3d_patch_mask_dev", "p3d_patch_route",
             "p3d_patch_run_dev", "p3d_patch_blend_dev"]
    header = open(os.path.join(ROOT, "include", "p3d.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in _ffi.PROTOTYPES and f"{name}(" in header, name
    assert lib.p3d_abi_version() == 1
    # a NULL plan is an argument error, not a crash -- and needs no device
    out = ctypes.c_void_p()
    starts = (ctypes.c_int32 * 1)(0)
    taper = (ctypes.c_float * 4)(1, 1, 1, 1)
    assert lib.p3d_patch_plan_create(ctypes.byref(out), None, 8, 8, starts, 1, starts, 1, taper, taper, 1) == _ffi.P3D_ERR_INVALID
    assert lib.p3d_patch_plan_destroy(None) == 0
