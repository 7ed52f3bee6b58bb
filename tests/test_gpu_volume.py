"""3-D FFT POCS on the GPU (``pocs_volume`` / ``p3d_vol_*``, csrc/p3d_vol.hip) against NumPy's fftn and the float64 oracle
``pocs_slice(x, mask, fwd=np.fft.fftn, inv=np.fft.ifftn, ...)`` on the seeded volumes of tests/helpers/volume_cases.py."""
import os
import sys

import numpy as np
import pytest
import yaml

from conftest import rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import volume_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

TRANSFORM_TOL = 2e-6   # test_gpu_dct.py
STEP_TOL = 2e-6
NSHAPES = len(vc.SHAPES)


@pytest.fixture(scope="module")
def ffi():
    from pseudo_3d_interpolation_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def P():
    from pseudo_3d_interpolation_amd.functions import POCS
    yield POCS
    POCS.release_plans()


@pytest.fixture(scope="module")
def orc():
    from oracle import pocs_oracle
    return pocs_oracle


def _bound(measured, single, want):
    """TRANSFORM_TOL, or -- only where the device measures above it -- twice SciPy's own single-precision error (the rule of test_gpu_dct.py)."""
    if measured < TRANSFORM_TOL:
        return TRANSFORM_TOL
    return 2 * rel_l2(single(), want)


# ------------------------------------------------------------------------------------------------
# 1. transform hook
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vc.SHAPES + vc.FFT3_EXTRA_SHAPES)
def test_fft3_matches_numpy(ffi, shape):
    import scipy.fft
    rng = np.random.default_rng([vc.SEED, *shape])
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    fwd = np.fft.fftn(x.astype(np.complex128))
    spec = fwd.astype(np.complex64)
    inv = np.fft.ifftn(spec.astype(np.complex128))
    with ffi.VolumePlan(*shape) as plan:
        got_f, got_i = plan.fft3(x), plan.fft3(spec, inverse=True)
    ef, ei = rel_l2(got_f, fwd), rel_l2(got_i, inv)
    print(f"fft3 {shape}: forward {ef:.2e}, inverse {ei:.2e}")
    assert got_f.dtype == np.complex64 and got_f.shape == shape
    assert ef < _bound(ef, lambda: scipy.fft.fftn(x), fwd), ef
    assert ei < _bound(ei, lambda: scipy.fft.ifftn(spec), inv), ei


def test_fft3_on_device_buffers_in_place(ffi):
    shape = vc.SHAPES[4]
    x = vc.volume(4, False, "2d")[0]
    with ffi.VolumePlan(*shape) as plan:
        d = ffi.DeviceArray(shape, np.complex64).upload(x)
        plan.fft3_dev(d.ptr, d.ptr)
        spec = d.download()
        plan.fft3_dev(d.ptr, d.ptr, inverse=True)
        back = d.download()
        assert np.array_equal(spec, plan.fft3(x))
        d.free()
    assert rel_l2(back, x) < TRANSFORM_TOL


def test_unsupported_first_axis_is_refused(ffi):
    assert ffi.vol_shape_supported(1024, 4, 8) and ffi.vol_shape_supported(1, 16, 16) and ffi.vol_shape_supported(945, 2, 2)
    for n0 in (0, 11, 13, 121, 1025, 2048):
        assert not ffi.vol_shape_supported(n0, 8, 8)
    with pytest.raises(ffi.UnsupportedError, match="n0 = 11"):
        ffi.VolumePlan(11, 8, 8)


# ------------------------------------------------------------------------------------------------
# 2. statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NSHAPES))
@pytest.mark.parametrize("real", [False, True])
def test_stats_match_numpy(ffi, i, real):
    """The tolerances test_gpu_parity.py::test_stats_match_numpy holds p3d_pocs_stats to."""
    x = vc.volume(i, real, "3d")[0]
    X = np.fft.fftn(x.astype(np.float64 if real else np.complex128))
    with ffi.VolumePlan(*x.shape) as plan:
        st = plan.stats(x)
    assert st.shape == (1, 6)
    st, pk = st[0], X.max()
    if real:
        # the spectrum of a real volume is Hermitian: a coefficient and its mirror image share their real part up to rounding, so the sign of the
        # imaginary part of the lexicographic maximum is rounding -- in NumPy as much as here (test_gpu_parity.py:614)
        assert abs(abs(st[1]) - abs(pk.imag)) < 1e-4 * abs(pk)
    else:
        assert abs(st[1] - pk.imag) < 1e-4 * abs(pk)
    assert abs(st[0] - pk.real) < 1e-4 * abs(pk)
    assert abs(st[2] - np.abs(X).max()) < 1e-5 * np.abs(X).max()
    assert abs(st[3] - np.abs(X).min()) < 1e-3 * np.abs(X).mean()
    assert abs(st[4] - np.linalg.norm(X) ** 2) < 1e-5 * np.linalg.norm(X) ** 2
    assert st[5] == 0


# ------------------------------------------------------------------------------------------------
# 3. one iteration: decisions and replay
# ------------------------------------------------------------------------------------------------
def _tie_band(spec, tau_re, scale=2e-6):
    """test_gpu_parity.py: coefficients whose modulus float32 arithmetic cannot place relative to Re(tau)."""
    return np.abs(np.abs(spec) - tau_re) <= scale * np.abs(spec).max()


@pytest.mark.parametrize("i", range(NSHAPES))
@pytest.mark.parametrize("op", vc.OPERATORS)
def test_step_decisions_and_result(ffi, orc, i, op):
    """One iteration with the complex tau of the real schedule: the device's keep / zero map may leave the oracle's only inside the float32 tie band,
    and the oracle step replayed with the device's map matches the device's step."""
    kind = vc.MASK_KINDS[i % 3]
    x32, mask = vc.volume(i, False, kind)
    x = x32.astype(np.complex128)
    tau = orc.threshold_schedule("exponential", vc.NITER, "FFT", 0.99, 1e-2, np.fft.fftn(x), "values")
    t = tau[vc.NITER // 2]
    assert t.imag != 0
    with ffi.VolumePlan(*x.shape) as plan:
        shr_gpu = plan.shrink(x32, t, op)
        out_gpu, done, sums, _ = plan.run(x32, mask, np.array([t]), 1, thresh_op=op)
    _, spec, shr = orc.pocs_step(x, x, mask, t, op, fwd=np.fft.fftn, inv=np.fft.ifftn)
    band = _tie_band(spec, t.real)
    kept_gpu, kept_ref = shr_gpu != 0, shr != 0
    assert kept_ref.any()
    assert np.array_equal(kept_gpu[~band], kept_ref[~band]), int(np.count_nonzero(kept_gpu[~band] != kept_ref[~band]))
    want, _, shr_replay = orc.pocs_step(x, x, mask, t, op, keep=kept_gpu, fwd=np.fft.fftn, inv=np.fft.ifftn)
    assert np.abs(shr_gpu - shr_replay).max() < 4e-6 * np.abs(spec).max()
    err = rel_l2(out_gpu, want)
    print(f"step {x.shape} {op} {kind}: {err:.2e}, {int(np.count_nonzero(kept_gpu != kept_ref))} decisions differ, band {int(band.sum())}")
    assert done == 1 and err < STEP_TOL, err
    assert abs(sums[1] - np.abs(want).sum()) < 1e-5 * np.abs(want).sum()
    assert abs(sums[0] - np.abs(x).sum()) < 1e-5 * np.abs(x).sum()


# ------------------------------------------------------------------------------------------------
# 4. / 5. whole loops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NSHAPES))
def test_loop_with_real_thresholds(P, i):
    """Real thresholds (0.5 ... 0.01 max|X0| as factors, 8 iterations) are continuous in the reference: every operator x version x mask kind x dtype is held
    to 1e-5 against the float64 oracle, none set aside."""
    worst = 0.0
    for op, version, kind, real in vc.grid():
        x, mask = vc.volume(i, real, kind)
        kw, want, _ = vc.real_tau_case(i, op, version, kind, real)
        res = []
        got = P.pocs_volume(x, mask, results=res, **kw)
        err = rel_l2(got, want)
        worst = max(worst, err)
        assert got.dtype == x.dtype and got.shape == x.shape and res[0]["niterations"] == vc.NITER
        assert err <= vc.BAR, (op, version, kind, real, err)
    print(f"real thresholds {vc.SHAPES[i]}: worst of {len(vc.grid())} cases {worst:.2e}")


@pytest.mark.parametrize("i", range(NSHAPES))
def test_loop_with_the_default_schedule(P, i):
    """The default schedule (complex thresholds p X0.max(), exponential and linear, p_min = 1e-2).  A case is set aside only when the reference's own
    single-precision run leaves the float64 oracle by more than 2.5e-6 -- computed from the reference alone --, at most one case in eight."""
    worst, aside, ncase = 0.0, 0, 0
    for model in ("exponential", "linear"):
        for op, version, kind, real in vc.grid():
            x, mask = vc.volume(i, real, kind)
            kw, want, spread = vc.default_case(i, op, version, kind, real, model)
            ncase += 1
            if not spread <= vc.SET_ASIDE_BAR:
                aside += 1
                continue
            err = rel_l2(P.pocs_volume(x, mask, **kw), want)
            worst = max(worst, err)
            assert err <= vc.BAR, (model, op, version, kind, real, err, spread)
    print(f"default schedule {vc.SHAPES[i]}: worst of {ncase - aside} cases {worst:.2e}, {aside} set aside")
    assert aside * vc.SET_ASIDE_CAP <= ncase


# ------------------------------------------------------------------------------------------------
# 6. early exit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,op,version,real", [(3, "hard", "regular", False), (4, "garrote", "adaptive", True), (5, "garrote", "fast", False), (7, "soft", "regular", True),
                                                (8, "soft", "adaptive", True)])
def test_early_exit_follows_the_oracle(P, i, op, version, real):
    from loop_cases import _eps_between_costs
    x, mask = vc.volume(i, real, "2d")
    kw = dict(vc.real_tau_kwargs(x, op, version), niter=14)
    info = {}
    vc.oracle(x, mask, info=info, **kw)
    eps = _eps_between_costs([info])
    assert eps > 0
    info = {}
    want = vc.oracle(x, mask, info=info, **dict(kw, eps=eps))
    assert 3 < info["niterations"] < 14, info["niterations"]
    res = []
    got = P.pocs_volume(x, mask, results=res, **dict(kw, eps=eps))
    assert len(res) == 1 and res[0]["niterations"] == info["niterations"]
    assert len(res[0]["costs"]) == len(info["costs"])
    assert np.allclose(res[0]["costs"], info["costs"], rtol=1e-4, atol=0)
    assert np.isclose(res[0]["cost"], info["costs"][-1], rtol=1e-4, atol=0)
    assert rel_l2(got, want) <= vc.BAR


# ------------------------------------------------------------------------------------------------
# 7. equivalences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (33, 20)])
def test_a_volume_of_one_slice_is_the_slice_job(P, orc, shape):
    _, mask, obs = orc.synthetic_cube(shape[0], shape[1], 1, 0.5)
    kw = dict(niter=8, thresh_op="soft", thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    a, b = P.pocs_volume(obs, mask, **kw), P.pocs_cube(obs, mask, **kw)
    assert rel_l2(a, b) <= 2e-6, rel_l2(a, b)


@pytest.mark.parametrize("dtype", [np.complex64, np.float32])
def test_an_all_zero_volume_comes_back_untouched(P, ffi, dtype):
    x, mask = np.zeros((8, 16, 32), dtype), vc.masks(3, False)["2d"]
    res = []
    out = P.pocs_volume(x, mask, niter=5, results=res)
    assert out.dtype == dtype and not out.any() and res == [{"niterations": 0, "runtime": 0, "cost": 0, "costs": [0]}]
    with ffi.VolumePlan(8, 16, 32) as plan:   # ... and through the C entry, which counts the non-zero samples itself
        out, done, sums, _ = plan.run(x, mask, np.ones(5), 5)
    assert done == 0 and not out.any() and not sums.any()


def test_in_place_on_the_device_equals_out_of_place(ffi, P):
    """A device `out` that IS `x` goes through the staging volume (every iteration reads x); with eps > 0 the result is written in every iteration."""
    x, mask = vc.volume(4, False, "weights")
    n = 10
    with ffi.VolumePlan(*x.shape) as plan:
        tau = P._schedule_from_stats(plan.stats(x), x.size, "exponential", n, 0.99, 1e-2, "values")[0]
        xd, od = ffi.DeviceArray(x.shape, x.dtype).upload(x), ffi.DeviceArray(x.shape, x.dtype)
        md = ffi.DeviceArray(mask.shape, np.float32).upload(mask.astype(np.float32))
        a = plan.run_dev(xd.ptr, ffi.P3D_C64, md.ptr, tau, n, od.ptr, thresh_op="soft", eps=1e-12)
        out = od.download()
        b = plan.run_dev(xd.ptr, ffi.P3D_C64, md.ptr, tau, n, xd.ptr, thresh_op="soft", eps=1e-12)
        inplace = xd.download()
        host = plan.run(x, mask, tau, n, thresh_op="soft", eps=1e-12)
        for d in (xd, od, md):
            d.free()
    assert a[0] == b[0] == host[1] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], host[2])
    assert np.array_equal(out, inplace) and np.array_equal(out, host[0])
    assert out.any() and not np.array_equal(out, x)


@pytest.mark.parametrize("real", [False, True])
def test_two_calls_are_bit_identical(P, real):
    """The cost sums are block sums folded in a fixed order: results, costs and the stopping iteration do not depend on atomic ordering."""
    x, mask = vc.volume(5, real, "3d")
    kw = dict(niter=12, thresh_op="hard", thresh_model="linear", eps=1e-7, p_max=0.99, p_min=1e-2, version="adaptive", alpha=0.8)
    ra, rb = [], []
    a, b = P.pocs_volume(x, mask, results=ra, **kw), P.pocs_volume(x, mask, results=rb, **kw)
    assert np.array_equal(a, b)
    assert ra[0]["niterations"] == rb[0]["niterations"] and ra[0]["costs"] == rb[0]["costs"]


# ------------------------------------------------------------------------------------------------
# 8. step 13
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["2d", "3d"])
def test_step13_volume_run(P, tmp_path, mask_kind):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, open_cube, save_cube
    n0, n1, n2 = vc.SHAPES[4]
    x, mask = vc.volume(4, True, mask_kind)
    fold = (vc.masks(4, True)["2d"] * 2).astype(np.uint8)          # fold counts: the mask rule clips them to 1
    data = {"env": np.ascontiguousarray(np.moveaxis(x, 0, 2)), "fold": fold}     # stored (iline, xline, twt): the driver moves `dim` first
    dims = {"env": ("iline", "xline", "twt"), "fold": ("iline", "xline")}
    if mask_kind == "3d":
        data["weights"], dims["weights"] = np.ascontiguousarray(np.moveaxis(mask, 0, 2)), ("iline", "xline", "twt")
    cube = Cube(data, dims, {"twt": 0.05 * np.arange(n0), "iline": np.arange(n1), "xline": np.arange(n2)}, {"history": "made;", "text": ""}, {}, {})
    path = save_cube(cube, str(tmp_path / "cube_twt.npz"))
    metadata = dict(transform_kind="fft", niter=6, eps=0, thresh_op="soft", thresh_model="exponential", decay_kind="values", p_max=0.99, p_min=0.05, alpha=1.0,
                    sqrt_decay=False, version="regular", verbose=False, volume=True)
    cfg = dict(dim="twt", var="env", batch_chunk=5, output_runtime_results=True, metadata=metadata)
    if mask_kind == "3d":
        cfg["mask_var"] = "weights"
    (tmp_path / "pocs.yml").write_text(yaml.safe_dump(cfg))
    step13.main(["13_cube_interpolate_POCS", path, "--path_pocs_parameter", str(tmp_path / "pocs.yml")])
    base = "cube_twt_FFT_soft_niter-6"
    out_dir = tmp_path / base
    names = sorted(os.listdir(out_dir))
    assert f"runtimes_{base}_vol.txt" in names and f"parameter_{base}.yml" in names
    batch_files = [f for f in names if f.endswith(".npz")]
    assert len(batch_files) == 3 and all(f.startswith(base + "_vol_") for f in batch_files)
    lines = (out_dir / f"runtimes_{base}_vol.txt").read_text().strip().splitlines()
    assert len(lines) == 1 and len(lines[0].split(";")) == 2 + 6 and lines[0].startswith("6;")
    assert yaml.safe_load((out_dir / f"parameter_{base}.yml").read_text())["volume"] is True
    icube = open_cube(str(tmp_path / f"{base}.npz"))
    assert "volume" in icube.attrs["interp_params_keys"].split(";")
    assert icube.dims["env_interp"] == ("twt", "iline", "xline")
    kw = {k: v for k, v in metadata.items() if k not in ("transform_kind", "verbose", "volume")}
    want = P.pocs_volume(x, np.where(fold <= 1, fold, 1) if mask_kind == "2d" else mask, **kw)
    assert np.array_equal(icube.data_vars["env_interp"], want)
    assert rel_l2(want, vc.oracle(x, mask, **kw)) <= vc.BAR
