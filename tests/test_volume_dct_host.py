"""3-D DCT POCS (``pocs_volume_dct``), everything that needs no GPU: the signature, the refusals (all raised before anything is uploaded), the C prototypes,
``volume: dct`` of the step-13 driver, and the seeded case list of tests/test_gpu_volume_dct.py held to what that file assumes of it -- from the oracle and
the reference's single-precision run alone."""
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
import volume_dct_cases as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"p3d_voldct_shape_supported", "p3d_voldct_plan_create", "p3d_voldct_plan_destroy", "p3d_voldct_dct3_c64", "p3d_voldct_dct3_c64_dev",
           "p3d_voldct_shrink_c64", "p3d_voldct_stats", "p3d_voldct_stats_dev", "p3d_voldct_run", "p3d_voldct_run_dev", "p3d_voldct_last_profile"}


@pytest.fixture
def no_upload(monkeypatch):
    """Every way onto the device raises: the errors below are raised before anything is uploaded."""
    def boom(*a, **k):
        raise AssertionError("reached the device")
    for name in ("Plan", "VolumePlan", "VolumePlanDct", "DeviceArray", "DeviceBuffer", "lib"):
        monkeypatch.setattr(_ffi, name, boom)


def _job(dtype=np.complex64, shape=(6, 8, 10)):
    return np.ones(shape, dtype), np.ones(shape[1:], np.float32)


# ------------------------------------------------------------------------------------------------
# signature and refusals
# ------------------------------------------------------------------------------------------------
def test_signature_is_pocs_volumes_plus_dct_norm():
    base = [(k, v.default) for k, v in inspect.signature(P.pocs_volume).parameters.items()]
    mine = [(k, v.default) for k, v in inspect.signature(P.pocs_volume_dct).parameters.items()]
    assert mine == base + [("dct_norm", None)]
    assert [(k, v.default) for k, v in inspect.signature(P.pocs_volume64).parameters.items()] == base


@pytest.mark.parametrize("op", ["hard-percentile", "soft-percentile", "garrote-percentile", "garotte-percentile"])
def test_percentile_operators_are_refused(no_upload, op):
    x, m = _job()
    with pytest.raises(NotImplementedError, match=r"pocs_volume_dct.*percentile"):
        P.pocs_volume_dct(x, m, thresh_op=op)


def test_data_driven_is_refused(no_upload):
    x, m = _job()
    with pytest.raises(NotImplementedError, match=r"pocs_volume_dct.*data-driven"):
        P.pocs_volume_dct(x, m, thresh_model="data-driven")


@pytest.mark.parametrize("dtype", [np.complex128, np.float64, np.int32])
def test_other_dtypes_are_refused_not_narrowed(no_upload, dtype):
    x, m = _job(dtype)
    with pytest.raises(NotImplementedError, match=rf"pocs_volume_dct.*{np.dtype(dtype).name}"):
        P.pocs_volume_dct(x, m)


@pytest.mark.parametrize("norm", ["forward", "Ortho", 1])
def test_unknown_norm_is_refused(no_upload, norm):
    x, m = _job()
    with pytest.raises(NotImplementedError, match="dct_norm"):
        P.pocs_volume_dct(x, m, dct_norm=norm)


@pytest.mark.parametrize("n0,near", [(11, "10 (below) and 12 (above)"), (1025, "1024 (below)")])
def test_unsupported_first_axis_lists_its_neighbours(no_upload, n0, near):
    x, m = _job(shape=(n0, 2, 3))
    with pytest.raises(ValueError, match=r"pocs_volume_dct: n0 = %d .*nearest supported: %s$" % (n0, re.escape(near))):
        P.pocs_volume_dct(x, m)


def test_argument_errors(no_upload):
    x, m = _job()
    with pytest.raises(ValueError, match="pocs_volume_dct"):
        P.pocs_volume_dct(x[0], m)
    with pytest.raises(ValueError, match="pocs_volume_dct.*mask shape"):
        P.pocs_volume_dct(x, m[:-1])
    with pytest.raises(ValueError, match="pocs_volume_dct.*quasi-boolean"):
        P.pocs_volume_dct(x, 2 * m)
    with pytest.raises(ValueError, match="pocs_volume_dct.*threshold operator"):
        P.pocs_volume_dct(x, m, thresh_op="firm")
    with pytest.raises(ValueError, match="pocs_volume_dct.*version"):
        P.pocs_volume_dct(x, m, version="faster")
    with pytest.raises(ValueError, match="pocs_volume_dct.*niter"):
        P.pocs_volume_dct(x, m, niter=0)


def test_a_volume_that_does_not_fit_is_refused(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_ffi, "VolumePlanDct", boom)
    monkeypatch.setattr(_ffi, "DeviceBuffer", boom)
    monkeypatch.setattr(_ffi, "shape_supported", lambda nil, nxl: True)
    monkeypatch.setattr(_ffi, "device_mem_info", lambda device=0: (1000, 2000))
    monkeypatch.setattr(P, "_plans", {})
    x, m = _job()
    needed = P._vol_bytes_needed(x.shape, 8, m.nbytes)
    with pytest.raises(MemoryError, match=rf"pocs_volume_dct.*needs {needed} bytes.* 1000 are free"):
        P.pocs_volume_dct(x, m)


@pytest.mark.parametrize("dtype", [np.complex64, np.float32])
def test_an_all_zero_volume_needs_no_device(no_upload, dtype):
    x, m = _job(dtype)
    x[...] = 0
    res = []
    out = P.pocs_volume_dct(x, m, results=res, dct_norm="ortho")
    assert out is not x and out.dtype == dtype and out.shape == x.shape and not out.any()
    assert res == [{"niterations": 0, "runtime": 0, "cost": 0, "costs": [0]}]


# ------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------
def test_every_voldct_prototype_has_a_ctypes_declaration():
    header = open(os.path.join(ROOT, "include", "p3d.h")).read()
    declared = set(re.findall(r"\b(p3d_voldct_[a-z0-9_]+)\s*\(", header))
    assert declared == ENTRIES
    assert declared == {n for n in _ffi.PROTOTYPES if n.startswith("p3d_voldct_")}
    for name in declared:   # argument counts of the header and of the table agree
        args = re.search(r"\b%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(_ffi.PROTOTYPES[name][1]) == len(args.split(",")), name
    for method in ("dct3", "dct3_dev", "shrink", "stats", "stats_dev", "run", "run_dev", "last_profile"):
        assert callable(getattr(_ffi.VolumePlanDct, method))
    assert not any(n.startswith(("p3d_vol_", "p3d_vol64_")) for n in ENTRIES)
    for hook in (_ffi.VolumePlanDct.fft3, _ffi.VolumePlanDct.fft3_dev):   # inherited names without an entry behind them say so
        with pytest.raises(_ffi.UnsupportedError, match="dct3"):
            hook(None)


def test_the_library_exports_the_entry_points_and_answers_the_shape_query():
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for n0 in range(0, 1100):   # the library and the host agree on the axis-0 lengths (no GPU needed)
        assert bool(lib.p3d_voldct_shape_supported(n0, 8, 8)) == P._vol_n0_supported(n0), n0
    assert lib.p3d_voldct_shape_supported(8, 0, 8) == 0


# ------------------------------------------------------------------------------------------------
# step 13
# ------------------------------------------------------------------------------------------------
def _step13(tmp_path, monkeypatch, extra, mask_var=None):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, save_cube
    n, nil, nxl = 5, 6, 8
    data = {"env": np.arange(nil * nxl * n, dtype=np.float32).reshape(nil, nxl, n), "fold": np.full((nil, nxl), 3, np.int32)}
    dims = {"env": ("iline", "xline", "twt"), "fold": ("iline", "xline")}
    if mask_var == "w3":
        data["w3"], dims["w3"] = np.full((nil, nxl, n), 0.5, np.float32), ("iline", "xline", "twt")
    ds = Cube(data, dims, {"twt": np.arange(n) * 1.0, "iline": np.arange(nil), "xline": np.arange(nxl)}, {"history": "", "text": ""}, {}, {})
    path = save_cube(ds, str(tmp_path / "cube.npz"))
    meta = dict(transform_kind="dct", niter=4, eps=0, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=0.1)
    meta.update(extra)
    cfg = dict(dim="twt", var="env", batch_chunk=2, output_runtime_results=True, metadata=meta)
    if mask_var:
        cfg["mask_var"] = mask_var
    yml = tmp_path / "pocs.yml"
    yml.write_text(yaml.safe_dump(cfg))
    calls = []

    def fake(tag):
        def run(x, mask, results=None, out=None, **kw):
            calls.append((tag, x.shape, np.asarray(mask), kw))
            if results is not None:
                results.extend({"niterations": 4, "runtime": 0.5, "cost": 0.0, "costs": [0.0] * 4} for _ in range(1 if tag != "cube" else x.shape[0]))
            if out is not None:
                out[...] = x
                return out
            return x + 1
        return run
    for tag, name in (("cube", "pocs_cube"), ("volume", "pocs_volume"), ("volume64", "pocs_volume64"), ("volume_dct", "pocs_volume_dct")):
        monkeypatch.setattr(step13, name, fake(tag))
    full = step13.main(["13", path, "--path_pocs_parameter", str(yml), "--path_output_dir", str(tmp_path / "out")], return_dataset=True)
    return calls, sorted(os.listdir(tmp_path / "out")), full, tmp_path / "out"


@pytest.mark.parametrize("norm_key,norm", [({}, "ortho"), (dict(dct_norm="backward"), "backward"), (dict(dct_norm="ortho"), "ortho")])
@pytest.mark.parametrize("mask_var,mask_shape,value", [(None, (6, 8), 1), ("w3", (5, 6, 8), 0.5)])
def test_step13_volume_dct_is_one_job(tmp_path, monkeypatch, no_upload, norm_key, norm, mask_var, mask_shape, value):
    calls, names, full, out = _step13(tmp_path, monkeypatch, dict(volume="dct", alpha=0.9, device=0, **norm_key), mask_var)
    assert len(calls) == 1 and calls[0][0] == "volume_dct" and calls[0][1] == (5, 6, 8)             # `dim` first, ONE job
    assert calls[0][2].shape == mask_shape and np.all(calls[0][2] == value)
    assert calls[0][3] == dict(niter=4, eps=0, thresh_op="soft", thresh_model="linear", p_max=0.9, p_min=0.1, alpha=0.9, device=0, dct_norm=norm)
    prefix = f"cube_DCT_soft_niter-4_{norm}_vol"
    assert f"runtimes_{prefix}.txt" in names and "parameter_cube_DCT_soft_niter-4.yml" in names
    batch = [n for n in names if n.endswith(".npz")]
    assert len(batch) == 3 and all(n.startswith(prefix + "_") for n in batch)
    assert (out / f"runtimes_{prefix}.txt").read_text() == "4;0.5;0.0;0.0;0.0;0.0\n"                # one line for the volume
    assert yaml.safe_load((out / "parameter_cube_DCT_soft_niter-4.yml").read_text())["volume"] == "dct"
    keys, vals = full.attrs["interp_params_keys"].split(";"), full.attrs["interp_params_vals"].split(";")
    assert vals[keys.index("volume")] == "dct" and vals[keys.index("dct_norm")] == norm
    want = np.moveaxis(np.arange(6 * 8 * 5, dtype=np.float32).reshape(6, 8, 5), 2, 0) + 1
    assert full.dims["env_interp"] == ("twt", "iline", "xline") and np.array_equal(full.data_vars["env_interp"], want)


def test_step13_dct_without_the_key_is_the_slice_loop(tmp_path, monkeypatch, no_upload):
    calls, names, _, _ = _step13(tmp_path, monkeypatch, {})
    assert calls and all(c[0] == "cube" for c in calls) and not any("_vol" in n for n in names)


@pytest.mark.parametrize("extra,word", [(dict(transform_kind="fft"), "DCT"), (dict(transform_kind="wavelet"), "DCT"), (dict(patch_shape=32), "patch_shape"),
                                        (dict(precision="reference"), "precision")])
def test_step13_volume_dct_refusals_name_the_key(tmp_path, monkeypatch, no_upload, extra, word):
    with pytest.raises(NotImplementedError, match=rf"volume: dct.*{word}"):
        _step13(tmp_path, monkeypatch, dict(volume="dct", **extra))
    assert not (tmp_path / "out").exists()                                                          # refused before anything is created


@pytest.mark.parametrize("volume", [True, "reference"])
def test_step13_the_fft_volume_keys_still_refuse_dct(tmp_path, monkeypatch, no_upload, volume):
    with pytest.raises(NotImplementedError, match=r"volume.*FFT"):
        _step13(tmp_path, monkeypatch, dict(volume=volume))
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("value", ["DCT", "cosine", "dctn", 3])
def test_step13_any_other_value_is_a_value_error(tmp_path, monkeypatch, no_upload, value):
    with pytest.raises(ValueError, match="^volume must be"):
        _step13(tmp_path, monkeypatch, dict(volume=value))
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------
# the seeded cases: which may be set aside
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched,norm", dc.BLOCKS)
def test_the_set_aside_list_stays_under_its_cap(sched, norm):
    """A case is set aside only when the reference's own single-precision run leaves the float64 oracle by more than 2.5e-6: never on a real (float32) volume,
    never on a complex volume with real thresholds and norm 'backward', and on at most one case in sixteen of each block."""
    spreads = {(i, g): dc.case(i, sched, norm, *g)[2] for i in range(len(dc.SHAPES)) for g in dc.grid()}
    assert len(spreads) == 486
    aside = [key for key in spreads if dc.set_aside(key[0], sched, norm, *key[1])]
    worst_real = max(s for (i, g), s in spreads.items() if g[3])
    worst_kept = max(s for key, s in spreads.items() if key not in aside)
    print(f"{sched} {norm}: {len(aside)} of 486 set aside, worst spread {max(spreads.values()):.2e}, real volumes {worst_real:.2e}, kept {worst_kept:.2e}")
    assert not any(g[3] for _, g in aside), [k for k in aside if k[1][3]]                            # real volumes: none
    assert worst_real <= dc.SET_ASIDE_BAR
    if (sched, norm) in dc.NONE_ASIDE:
        assert not aside, aside
    assert len(aside) * dc.SET_ASIDE_CAP <= len(spreads), len(aside)
