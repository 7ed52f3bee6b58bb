"""3-D FFT POCS in double precision (``pocs_volume64`` / ``p3d_vol64_*``), everything that needs no GPU: the signature, the refusals (all raised before
anything reaches the device), the C prototypes, ``volume: reference`` in the step-13 driver, and the reason why tests/test_gpu_volume64.py sets no case
aside -- two independent double-precision FFTs agree on every case it runs."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import yaml

from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import POCS as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import volume_cases as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"p3d_vol64_shape_supported", "p3d_vol64_plan_create", "p3d_vol64_plan_destroy", "p3d_vol64_fft3_c128", "p3d_vol64_fft3_c128_dev",
           "p3d_vol64_shrink_c128", "p3d_vol64_stats", "p3d_vol64_stats_dev", "p3d_vol64_run", "p3d_vol64_run_dev", "p3d_vol64_last_profile"}
TWO_FFTS_BAR = 1e-12   # two independent double-precision FFTs (NumPy's and SciPy's) through the whole loop: a case above it would be set aside


@pytest.fixture
def no_upload(monkeypatch):
    """Every way onto the device raises: the errors below are raised before anything is uploaded."""
    def boom(*a, **k):
        raise AssertionError("reached the device")
    for name in ("Plan", "Plan64", "VolumePlan", "VolumePlan64", "DeviceArray", "DeviceBuffer", "lib", "vol64_shape_supported", "shape_supported",
                 "device_mem_info"):
        monkeypatch.setattr(_ffi, name, boom)


def _job(dtype=np.complex128, shape=(6, 8, 10)):
    return np.ones(shape, dtype), np.ones(shape[1:], np.float64)


# ------------------------------------------------------------------------------------------------
# the entry point and its refusals
# ------------------------------------------------------------------------------------------------
def test_signature_equals_pocs_volume():
    a, b = inspect.signature(P.pocs_volume64), inspect.signature(P.pocs_volume)
    assert [(k, v.default, v.kind) for k, v in a.parameters.items()] == [(k, v.default, v.kind) for k, v in b.parameters.items()]
    assert list(a.parameters)[:2] == ["x", "mask"]


@pytest.mark.parametrize("op", ["hard-percentile", "soft-percentile", "garrote-percentile", "garotte-percentile"])
def test_percentile_operators_are_refused(no_upload, op):
    x, m = _job()
    with pytest.raises(NotImplementedError, match=r"pocs_volume64.*percentile"):
        P.pocs_volume64(x, m, thresh_op=op)


def test_data_driven_is_refused(no_upload):
    x, m = _job()
    with pytest.raises(NotImplementedError, match=r"pocs_volume64.*data-driven"):
        P.pocs_volume64(x, m, thresh_model="data-driven")


@pytest.mark.parametrize("n0,near", [(11, "10 (below) and 12 (above)"), (13, "12 (below) and 14 (above)"), (1023, "1008 (below) and 1024 (above)"),
                                     (1025, "1024 (below)"), (2048, "1024 (below)")])
def test_unsupported_first_axis_lists_its_neighbours(no_upload, n0, near):
    x, m = _job(shape=(n0, 2, 3))
    with pytest.raises(ValueError, match=r"pocs_volume64: n0 = %d .*nearest supported: %s$" % (n0, re.escape(near))):
        P.pocs_volume64(x, m)


def test_argument_errors(no_upload):
    x, m = _job()
    with pytest.raises(ValueError, match="pocs_volume64"):
        P.pocs_volume64(x[0], m)
    with pytest.raises(ValueError, match="pocs_volume64.*mask shape"):
        P.pocs_volume64(x, m[:-1])
    with pytest.raises(ValueError, match="pocs_volume64.*quasi-boolean"):
        P.pocs_volume64(x, 2 * m)
    with pytest.raises(ValueError, match="pocs_volume64.*threshold operator"):
        P.pocs_volume64(x, m, thresh_op="firm")
    with pytest.raises(ValueError, match="pocs_volume64.*version"):
        P.pocs_volume64(x, m, version="faster")
    with pytest.raises(ValueError, match="pocs_volume64.*niter"):
        P.pocs_volume64(x, m, niter=0)
    with pytest.raises(NotImplementedError, match="pocs_volume64.*int16"):
        P.pocs_volume64(x.real.astype(np.int16), m)


@pytest.mark.parametrize("dtype", [np.complex128, np.float64, np.complex64, np.float32])
def test_a_volume_that_does_not_fit_is_refused(monkeypatch, dtype):
    def boom(*a, **k):
        raise AssertionError("reached the device")
    for name in ("Plan", "Plan64", "VolumePlan", "VolumePlan64", "DeviceArray", "DeviceBuffer"):
        monkeypatch.setattr(_ffi, name, boom)
    monkeypatch.setattr(_ffi, "vol64_shape_supported", lambda n0, n1, n2: True)
    monkeypatch.setattr(_ffi, "device_mem_info", lambda device=0: (1000, 2000))
    monkeypatch.setattr(P, "_plans", {})
    x, m = _job(dtype)
    needed = P._vol64_bytes_needed(x.shape, x.itemsize, 8 * m.size)
    assert needed >= 16 * x.size + 2 * x.nbytes + 8 * m.size                                         # 16-B work elements, an 8-B mask
    with pytest.raises(MemoryError, match=rf"pocs_volume64.*needs {needed} bytes.* 1000 are free"):
        P.pocs_volume64(x, m.astype(np.float32))
    assert P._vol_bytes_needed(x.shape, 8, 4 * m.size) == 8 * x.size + 16 * x.size + 4 * m.size + 3 * 6 * 8 * 10 * 8   # the float32 estimate is as it was


@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
def test_an_all_zero_volume_needs_no_device(no_upload, dtype):
    x, m = _job(dtype)
    x[...] = 0
    res = []
    out = P.pocs_volume64(x, m, results=res)
    assert out is not x and out.dtype == dtype and out.shape == x.shape and not out.any()
    assert res == [{"niterations": 0, "runtime": 0, "cost": 0, "costs": [0]}]


def test_pocs_volume_still_refuses_double_input_and_points_here(no_upload):
    x, m = _job()
    with pytest.raises(NotImplementedError, match=r"pocs_volume.*complex128.*pocs_volume64"):
        P.pocs_volume(x, m)


# ------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------
def test_every_vol64_prototype_has_a_ctypes_declaration():
    header = open(os.path.join(ROOT, "include", "p3d.h")).read()
    declared = set(re.findall(r"\b(p3d_vol64_[a-z0-9_]+)\s*\(", header))
    assert declared == ENTRIES
    assert declared == {n for n in _ffi.PROTOTYPES if n.startswith("p3d_vol64_")}
    for name in declared:   # argument counts of the header and of the table agree
        args = re.search(r"\b%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(_ffi.PROTOTYPES[name][1]) == len(args.split(",")), name
    for method in ("fft3", "fft3_dev", "shrink", "stats", "stats_dev", "run", "run_dev", "last_profile"):
        assert callable(getattr(_ffi.VolumePlan64, method))
    assert _ffi.VolumePlan64._MASK_DT is np.float64 and _ffi.VolumePlan._MASK_DT is np.float32


def test_the_library_exports_the_entry_points_and_answers_the_shape_query():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for n0 in range(0, 1100):   # the library and the host agree on the axis-0 lengths (no GPU needed)
        assert bool(lib.p3d_vol64_shape_supported(n0, 8, 8)) == P._vol_n0_supported(n0), n0
    assert lib.p3d_vol64_shape_supported(8, 0, 8) == 0 and lib.p3d_vol64_shape_supported(8, 8, 5121) == 0
    assert lib.p3d_vol64_shape_supported(8, 5120, 33) == 1


# ------------------------------------------------------------------------------------------------
# step 13
# ------------------------------------------------------------------------------------------------
def _step13(tmp_path, monkeypatch, extra, mask_var=None, dtype=np.float32):
    """The pattern of tests/test_volume_host.py::_step13 with all three job functions replaced."""
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, save_cube
    n, nil, nxl = 5, 6, 8
    data = {"env": np.arange(nil * nxl * n, dtype=dtype).reshape(nil, nxl, n), "fold": np.full((nil, nxl), 3, np.int32)}
    dims = {"env": ("iline", "xline", "twt"), "fold": ("iline", "xline")}
    if mask_var == "w3":
        data["w3"], dims["w3"] = np.full((nil, nxl, n), 0.5, np.float32), ("iline", "xline", "twt")
    elif mask_var == "w2":
        data["w2"], dims["w2"] = np.full((nil, nxl), 0.25, np.float32), ("iline", "xline")
    ds = Cube(data, dims, {"twt": np.arange(n) * 1.0, "iline": np.arange(nil), "xline": np.arange(nxl)}, {"history": "", "text": ""}, {}, {})
    path = save_cube(ds, str(tmp_path / "cube.npz"))
    meta = dict(transform_kind="fft", niter=4, eps=0, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=0.1)
    meta.update(extra)
    cfg = dict(dim="twt", var="env", batch_chunk=2, output_runtime_results=True, metadata=meta)
    if mask_var:
        cfg["mask_var"] = mask_var
    yml = tmp_path / "pocs.yml"
    yml.write_text(yaml.safe_dump(cfg))
    calls = []

    def fake_cube(cube, mask, results=None, out=None, **kw):
        calls.append(("cube", cube.shape, np.asarray(mask), kw, cube.dtype))
        out[...] = cube
        return out

    def fake(name):
        def run(x, mask, results=None, **kw):
            calls.append((name, x.shape, np.asarray(mask), kw, x.dtype))
            if results is not None:
                results.append({"niterations": 4, "runtime": 0.5, "cost": 0.0, "costs": [0.0] * 4})
            return x + 1
        return run
    monkeypatch.setattr(step13, "pocs_cube", fake_cube)
    monkeypatch.setattr(step13, "pocs_volume", fake("volume"))
    monkeypatch.setattr(step13, "pocs_volume64", fake("volume64"))
    full = step13.main(["13", path, "--path_pocs_parameter", str(yml), "--path_output_dir", str(tmp_path / "out")], return_dataset=True)
    return calls, sorted(os.listdir(tmp_path / "out")), full, tmp_path / "out"


@pytest.mark.parametrize("mask_var,mask_shape,value", [(None, (6, 8), 1), ("w2", (6, 8), 0.25), ("w3", (5, 6, 8), 0.5)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_step13_volume_reference_is_one_double_job(tmp_path, monkeypatch, no_upload, mask_var, mask_shape, value, dtype):
    calls, names, full, out = _step13(tmp_path, monkeypatch, dict(volume="reference", alpha=0.9, device=0), mask_var, dtype)
    assert len(calls) == 1 and calls[0][0] == "volume64" and calls[0][1] == (5, 6, 8) and calls[0][4] == dtype    # the variable as it is, ONE job
    assert calls[0][2].shape == mask_shape and np.all(calls[0][2] == value)
    assert calls[0][3] == dict(niter=4, eps=0, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=0.1, alpha=0.9, device=0)
    prefix = "cube_FFT_soft_niter-4_vol64"
    assert f"runtimes_{prefix}.txt" in names and "parameter_cube_FFT_soft_niter-4.yml" in names
    batch = [n for n in names if n.endswith(".npz")]
    assert len(batch) == 3 and all(n.startswith(prefix + "_") for n in batch)
    assert (out / f"runtimes_{prefix}.txt").read_text() == "4;0.5;0.0;0.0;0.0;0.0\n"                # one line for the volume
    assert yaml.safe_load((out / "parameter_cube_FFT_soft_niter-4.yml").read_text())["volume"] == "reference"
    keys, vals = full.attrs["interp_params_keys"].split(";"), full.attrs["interp_params_vals"].split(";")
    assert vals[keys.index("volume")] == "reference"
    want = np.moveaxis(np.arange(6 * 8 * 5, dtype=dtype).reshape(6, 8, 5), 2, 0) + 1
    assert full.dims["env_interp"] == ("twt", "iline", "xline") and np.array_equal(full.data_vars["env_interp"], want)
    assert full.data_vars["env_interp"].dtype == dtype


def test_step13_volume_true_still_runs_the_float32_job(tmp_path, monkeypatch, no_upload):
    calls, names, _, _ = _step13(tmp_path, monkeypatch, dict(volume=True))
    assert [c[0] for c in calls] == ["volume"] and "runtimes_cube_FFT_soft_niter-4_vol.txt" in names and not any("_vol64" in n for n in names)


@pytest.mark.parametrize("extra,word", [(dict(patch_shape=32), "patch_shape"), (dict(transform_kind="dct"), "FFT"), (dict(transform_kind="wavelet"), "FFT"),
                                        (dict(transform_kind="shearlet"), "FFT")])
def test_step13_volume_reference_refusals_name_the_key(tmp_path, monkeypatch, no_upload, extra, word):
    with pytest.raises(NotImplementedError, match=rf"volume: reference.*{word}"):
        _step13(tmp_path, monkeypatch, dict(volume="reference", **extra))
    assert not (tmp_path / "out").exists()                                                          # refused before anything is created


@pytest.mark.parametrize("value", ["double", "true64", 1, 2.0, "Reference"])
def test_step13_any_other_value_is_a_value_error(tmp_path, monkeypatch, no_upload, value):
    with pytest.raises(ValueError, match="volume must be"):
        _step13(tmp_path, monkeypatch, dict(volume=value))
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------
# the case list: why no case is set aside
# ------------------------------------------------------------------------------------------------
def test_two_double_ffts_agree_on_every_loop_case():
    """tests/test_gpu_volume64.py holds the device to 1e-10 on 9 shapes x 54 combinations x {default schedule exponential, default schedule linear, real
    thresholds} and sets none aside.  That is legitimate only if the float64 trajectory itself is stable on every one of them: the oracle run with SciPy's
    fftn / ifftn must agree with the oracle run with NumPy's (two independent double-precision FFTs) to 1e-12.  Measured: 1458 runs, worst 1.3e-14."""
    import scipy.fft

    from oracle import pocs_oracle as orc
    worst, above, runs = 0.0, 0, 0
    for i in range(len(vc.SHAPES)):
        for op, version, kind, real in vc.grid():
            x, mask = vc.volume(i, real, kind)
            wide = x.astype(np.float64 if real else np.complex128)
            cases = [vc.default_case(i, op, version, kind, real, "exponential"), vc.default_case(i, op, version, kind, real, "linear"),
                     vc.real_tau_case(i, op, version, kind, real)]
            for kw, want, _ in cases:
                got = np.asarray(orc.pocs_slice(wide, mask, fwd=scipy.fft.fftn, inv=scipy.fft.ifftn, **kw))
                err = vc.rel_l2(got, want)
                worst, above, runs = max(worst, err), above + (not err <= TWO_FFTS_BAR), runs + 1
    print(f"two double FFTs through the loop: {runs} runs, worst {worst:.2e}, {above} above {TWO_FFTS_BAR:g}")
    assert runs == 9 * 54 * 3 and above == 0, (worst, above)
