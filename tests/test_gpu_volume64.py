"""3-D FFT POCS in double precision on the GPU (``pocs_volume64`` / ``p3d_vol64_*``, csrc/p3d_vol64.hip) against NumPy's fftn in double and the float64 oracle
``pocs_slice(x, mask, fwd=np.fft.fftn, inv=np.fft.ifftn, ...)`` on the seeded volumes of tests/helpers/volume_cases.py, widened to complex128 / float64.
The loops are held to the project's double-precision bar, 1e-10, with no case set aside (tests/test_volume64_host.py shows why none needs to be)."""
import os
import sys

import numpy as np
import pytest
import yaml

from conftest import rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import volume_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

FFT_BAR = 1e-13    # about 50 eps log2(N) for the largest N here (2^15 points)
STAT_BAR = 1e-12   # test_gpu_dct64.py
STEP_BAR = 1e-12
LOOP_BAR = 1e-10   # the double-precision loops against the float64 oracle
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


def _wide(x):
    return x.astype(np.float64 if x.dtype == np.float32 else np.complex128)


# ------------------------------------------------------------------------------------------------
# 1. transform hooks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vc.SHAPES + vc.FFT3_EXTRA_SHAPES)
def test_fft3_matches_numpy(ffi, shape):
    rng = np.random.default_rng([vc.SEED, 64, *shape])
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    fwd = np.fft.fftn(x)
    inv = np.fft.ifftn(fwd)
    with ffi.VolumePlan64(*shape) as plan:
        got_f, got_i = plan.fft3(x), plan.fft3(fwd, inverse=True)
    ef, ei = rel_l2(got_f, fwd), rel_l2(got_i, inv)
    print(f"fft3 in double {shape}: forward {ef:.2e}, inverse {ei:.2e}")
    assert got_f.dtype == np.complex128 and got_f.shape == shape
    assert ef < FFT_BAR and ei < FFT_BAR, (ef, ei)


def test_fft3_on_device_buffers_in_place(ffi):
    shape = vc.SHAPES[4]
    x = _wide(vc.volume(4, False, "2d")[0])
    with ffi.VolumePlan64(*shape) as plan:
        d = ffi.DeviceArray(shape, np.complex128).upload(x)
        plan.fft3_dev(d.ptr, d.ptr)
        spec = d.download()
        plan.fft3_dev(d.ptr, d.ptr, inverse=True)
        back = d.download()
        assert np.array_equal(spec, plan.fft3(x))
        d.free()
    assert rel_l2(spec, np.fft.fftn(x)) < FFT_BAR and rel_l2(back, x) < FFT_BAR


def test_unsupported_first_axis_is_refused(ffi):
    assert ffi.vol64_shape_supported(1024, 4, 8) and ffi.vol64_shape_supported(1, 16, 16) and ffi.vol64_shape_supported(945, 2, 2)
    for n0 in (0, 11, 13, 121, 1025, 2048):
        assert not ffi.vol64_shape_supported(n0, 8, 8)
    with pytest.raises(ffi.UnsupportedError, match="n0 = 11"):   # P3D_ERR_UNSUPPORTED
        ffi.VolumePlan64(11, 8, 8)


# ------------------------------------------------------------------------------------------------
# 2. statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NSHAPES))
@pytest.mark.parametrize("real", [False, True])
def test_stats_match_numpy(ffi, i, real):
    x = _wide(vc.volume(i, real, "3d")[0])
    X = np.fft.fftn(x)
    with ffi.VolumePlan64(*x.shape) as plan:
        st = plan.stats(x)
    assert st.shape == (1, 6)
    st, pk, top = st[0], X.max(), np.abs(X).max()
    if real:
        # the spectrum of a real volume is Hermitian: a coefficient and its mirror image share their real part up to rounding, so the sign of the
        # imaginary part of the lexicographic maximum is rounding -- in NumPy as much as here (test_gpu_volume.py)
        assert abs(abs(st[1]) - abs(pk.imag)) <= STAT_BAR * abs(pk)
    else:
        assert abs(st[1] - pk.imag) <= STAT_BAR * abs(pk)
    assert abs(st[0] - pk.real) <= STAT_BAR * abs(pk)
    assert abs(st[2] - top) <= STAT_BAR * top
    assert abs(st[3] - np.abs(X).min()) <= STAT_BAR * top
    assert abs(st[4] - np.linalg.norm(X) ** 2) <= STAT_BAR * np.linalg.norm(X) ** 2
    assert st[5] == 0


# ------------------------------------------------------------------------------------------------
# 3. one iteration: decisions and result
# ------------------------------------------------------------------------------------------------
def _boundary(op, t):
    """|X| at which the operator's keep / zero decision flips (threshold_operator.py with a complex tau: hard and soft compare |X| with Re tau, garrote
    |X|^2 with Re tau^2)."""
    if op == "garrote":
        return np.sqrt(max((t * t).real, 0.0))
    return t.real


@pytest.mark.parametrize("i", range(NSHAPES))
@pytest.mark.parametrize("op", vc.OPERATORS)
def test_step_decisions_and_result(ffi, orc, i, op):
    kind = vc.MASK_KINDS[i % 3]
    x32, mask = vc.volume(i, False, kind)
    x = _wide(x32)
    tau = orc.threshold_schedule("exponential", vc.NITER, "FFT", 0.99, 1e-2, np.fft.fftn(x), "values")
    t = tau[vc.NITER // 2]
    assert t.imag != 0
    with ffi.VolumePlan64(*x.shape) as plan:
        shr_gpu = plan.shrink(x, t, op)
        out_gpu, done, sums, _ = plan.run(x, mask, np.array([t]), 1, thresh_op=op)
    want, spec, shr = orc.pocs_step(x, x, mask, t, op, fwd=np.fft.fftn, inv=np.fft.ifftn)
    band = np.abs(np.abs(spec) - _boundary(op, t)) <= 1e-12 * abs(t)
    kept_gpu, kept_ref = shr_gpu != 0, shr != 0
    assert kept_ref.any()
    assert np.array_equal(kept_gpu[~band], kept_ref[~band]), int(np.count_nonzero(kept_gpu[~band] != kept_ref[~band]))
    err = rel_l2(out_gpu, want)
    print(f"step in double {x.shape} {op} {kind}: {err:.2e}, {int(np.count_nonzero(kept_gpu != kept_ref))} decisions differ, band {int(band.sum())}")
    assert out_gpu.dtype == np.complex128 and done == 1 and err < STEP_BAR, err
    assert rel_l2(shr_gpu, shr) < STEP_BAR
    assert abs(sums[1] - np.abs(want).sum()) <= STEP_BAR * np.abs(want).sum()
    assert abs(sums[0] - np.abs(x).sum()) <= STEP_BAR * np.abs(x).sum()


# ------------------------------------------------------------------------------------------------
# 4. whole loops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NSHAPES))
def test_loops_against_the_oracle(P, i):
    """8 iterations of every operator x version x mask kind x dtype with the real-threshold schedule and with the default schedule (complex thresholds,
    exponential and linear): 1e-10 against the float64 oracle, the oracle's iteration count, no case set aside.

    Measured on an MI355X over the nine shapes (1458 runs): worst 3.0e-14 (the volume of one slice), 4.0e-15 on the others."""
    worst, runs = 0.0, 0
    for op, version, kind, real in vc.grid():
        x, mask = vc.volume(i, real, kind)
        xw = _wide(x)
        cases = [("real", vc.real_tau_case(i, op, version, kind, real)), ("exponential", vc.default_case(i, op, version, kind, real, "exponential")),
                 ("linear", vc.default_case(i, op, version, kind, real, "linear"))]
        for label, (kw, want, _) in cases:
            res = []
            got = P.pocs_volume64(xw, mask, results=res, **kw)
            err = rel_l2(got, want)
            worst, runs = max(worst, err), runs + 1
            assert got.dtype == xw.dtype and got.shape == x.shape and res[0]["niterations"] == vc.NITER
            assert err <= LOOP_BAR, (label, op, version, kind, real, err)
    print(f"loops in double {vc.SHAPES[i]}: worst of {runs} runs {worst:.2e}")
    assert runs == 3 * 54


@pytest.mark.parametrize("shape", [(256, 3, 5), (160, 2, 4), (1024, 2, 3)])
@pytest.mark.parametrize("op", ["hard", "soft"])
def test_loop_on_the_narrow_tiles(P, shape, op):
    """First axes above 128 points run on tiles of 8 positions (128-byte rows): 256 = 4^4 and 1024 = 4^5 with an even innermost radix, 160 = 4 4 2 5 with an
    odd one; planes of 15, 8 and 6 positions, so a tile is partly or exactly filled.  The seeded volumes stop at n0 = 100."""
    rng = np.random.default_rng([vc.SEED, 65, *shape])
    mask = (rng.random(shape[1:]) >= vc.MISSING).astype(np.float64)
    mask[0, 0] = 1.0
    k = np.arange(shape[0])[:, None, None] / shape[0]
    x = (np.exp(2j * np.pi * 3 * k) + 0.5 * np.exp(-2j * np.pi * 7 * k) + 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))) * mask
    kw = vc.default_kwargs(op, "fast", "exponential")
    info, res = {}, []
    want = vc.oracle(x, mask, info=info, **kw)
    got = P.pocs_volume64(x, mask, results=res, **kw)
    err = rel_l2(got, want)
    print(f"narrow tiles {shape} {op}: {err:.2e}")
    assert res[0]["niterations"] == info["niterations"] == vc.NITER and err <= LOOP_BAR, err
    assert np.allclose(res[0]["costs"], info["costs"], rtol=1e-10, atol=0)


# ------------------------------------------------------------------------------------------------
# 5. early exit
# ------------------------------------------------------------------------------------------------
def _eps_at_an_exit(costs):
    """eps between the oracle's cost at an exit iteration e (0-based, e > 2) and at the one before -- their geometric mean --, e chosen where that gap is
    widest among the iterations that exit there (every earlier cost the exit rule looks at stays above eps).  Returns (eps, e)."""
    best = None
    for e in range(4, len(costs) - 1):
        eps = float(np.sqrt(costs[e] * costs[e - 1]))
        if costs[e] < eps < min(costs[3:e]):
            ratio = costs[e - 1] / costs[e]
            if best is None or ratio > best[0]:
                best = (ratio, eps, e)
    assert best is not None and best[0] >= 1.2 ** 2, costs
    return best[1], best[2]


@pytest.mark.parametrize("i,op,version,real", [(3, "hard", "regular", False), (4, "garrote", "adaptive", True), (5, "garrote", "fast", False), (7, "soft", "regular", True),
                                                (8, "soft", "adaptive", True)])
def test_early_exit_follows_the_oracle(P, i, op, version, real):
    x, mask = vc.volume(i, real, "2d")
    kw = dict(vc.real_tau_kwargs(x, op, version), niter=14)
    info = {}
    vc.oracle(x, mask, info=info, **kw)
    eps, e = _eps_at_an_exit(info["costs"])
    info = {}
    want = vc.oracle(x, mask, info=info, **dict(kw, eps=eps))
    assert info["niterations"] == e + 1 and 3 < info["niterations"] < 14
    res = []
    got = P.pocs_volume64(_wide(x), mask, results=res, **dict(kw, eps=eps))
    assert len(res) == 1 and res[0]["niterations"] == info["niterations"]
    assert len(res[0]["costs"]) == len(info["costs"])
    print(f"early exit in double {x.shape} {op} {version}: {info['niterations']} iterations, costs off by "
          f"{np.max(np.abs(np.array(res[0]['costs']) / np.array(info['costs']) - 1)):.2e}")
    assert np.allclose(res[0]["costs"], info["costs"], rtol=1e-10, atol=0)
    assert np.isclose(res[0]["cost"], info["costs"][-1], rtol=1e-10, atol=0)
    assert rel_l2(got, want) <= LOOP_BAR


# ------------------------------------------------------------------------------------------------
# 6. narrow inputs, equivalences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [False, True])
def test_narrow_volumes_run_in_double_and_keep_their_type(P, real):
    """complex64 / float32 in: computed in double (within 1e-10 of the oracle on the widened volume before the final cast), rounded once on store.  Against the
    oracle's result cast to the narrow type that leaves at most one unit in the last place per component -- a value 1e-10 from a rounding boundary may fall
    on its other side -- and half a unit (2^-24) in rel-L2."""
    x, mask = vc.volume(4, real, "weights")
    kw, want, _ = vc.default_case(4, "soft", "fast", "weights", real, "exponential")
    got = P.pocs_volume64(x, mask, **kw)
    assert got.dtype == x.dtype and got.shape == x.shape
    want32 = want.astype(x.dtype)
    floor = LOOP_BAR * np.abs(want).max()
    for part in ((np.real,) if real else (np.real, np.imag)):
        g, w = part(got).astype(np.float64), part(want32).astype(np.float64)
        assert np.all(np.abs(g - w) <= np.spacing(np.abs(part(want32))).astype(np.float64) + floor)
    err = rel_l2(got, want)
    print(f"narrow volume {x.dtype}: {err:.2e} from the float64 oracle, {np.mean(got != want32):.1e} of the samples differ from its cast")
    assert err <= 2.0 ** -24 + LOOP_BAR


@pytest.mark.parametrize("real", [False, True])
def test_two_calls_are_bit_identical(P, real):
    """The cost sums are workgroup sums folded in a fixed order: results, costs and the stopping iteration do not depend on atomic ordering."""
    x, mask = vc.volume(5, real, "3d")
    kw = dict(niter=12, thresh_op="hard", thresh_model="linear", eps=1e-7, p_max=0.99, p_min=1e-2, version="adaptive", alpha=0.8)
    ra, rb = [], []
    a, b = P.pocs_volume64(_wide(x), mask, results=ra, **kw), P.pocs_volume64(_wide(x), mask, results=rb, **kw)
    assert a.dtype == (np.float64 if real else np.complex128) and np.array_equal(a, b) and a.any()
    assert ra[0]["niterations"] == rb[0]["niterations"] and ra[0]["costs"] == rb[0]["costs"]


def test_in_place_on_the_device_equals_out_of_place(ffi, P):
    """A device `out` that IS `x` goes through the staging volume (every iteration reads x); with eps > 0 the result is written in every iteration."""
    x32, mask = vc.volume(4, False, "weights")
    x, n = _wide(x32), 10
    with ffi.VolumePlan64(*x.shape) as plan:
        tau = P._schedule_from_stats(plan.stats(x), x.size, "exponential", n, 0.99, 1e-2, "values")[0]
        xd, od = ffi.DeviceArray(x.shape, x.dtype).upload(x), ffi.DeviceArray(x.shape, x.dtype)
        md = ffi.DeviceArray(mask.shape, np.float64).upload(mask)
        a = plan.run_dev(xd.ptr, ffi.P3D_C128, md.ptr, tau, n, od.ptr, thresh_op="soft", eps=1e-12)
        out = od.download()
        b = plan.run_dev(xd.ptr, ffi.P3D_C128, md.ptr, tau, n, xd.ptr, thresh_op="soft", eps=1e-12)
        inplace = xd.download()
        host = plan.run(x, mask, tau, n, thresh_op="soft", eps=1e-12)
        for d in (xd, od, md):
            d.free()
    assert a[0] == b[0] == host[1] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], host[2])
    assert np.array_equal(out, inplace) and np.array_equal(out, host[0])
    assert out.any() and not np.array_equal(out, x)


@pytest.mark.parametrize("dtype", [np.complex128, np.float32])
def test_an_all_zero_volume_comes_back_untouched_through_the_c_entry(ffi, dtype):
    x, mask = np.zeros((8, 16, 32), dtype), vc.masks(3, False)["2d"]
    with ffi.VolumePlan64(8, 16, 32) as plan:   # the C entry counts the non-zero samples itself
        out, done, sums, _ = plan.run(x, mask, np.ones(5), 5)
    assert out.dtype == dtype and done == 0 and not out.any() and not sums.any()


@pytest.mark.parametrize("shape", [(64, 64), (33, 20)])
def test_a_volume_of_one_slice_is_the_double_slice_job(P, orc, shape):
    _, mask, obs = orc.synthetic_cube(shape[0], shape[1], 1, 0.5)
    obs = obs.astype(np.complex128)
    kw = dict(niter=8, thresh_op="soft", thresh_model="exponential", eps=0, p_max=0.99, p_min=1e-2)
    a, b = P.pocs_volume64(obs, mask, **kw), P.pocs_cube(obs, mask, precision="reference", **kw)
    assert a.dtype == b.dtype == np.complex128 and rel_l2(a, b) <= 1e-12, rel_l2(a, b)


# ------------------------------------------------------------------------------------------------
# 7. step 13
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["2d", "3d"])
def test_step13_volume_reference_run(P, tmp_path, mask_kind):
    """``volume: reference`` on the cube tests/test_gpu_volume.py::test_step13_volume_run builds: the float32 variable runs in double and is stored as float32."""
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
                    sqrt_decay=False, version="regular", verbose=False, volume="reference")
    cfg = dict(dim="twt", var="env", batch_chunk=5, output_runtime_results=True, metadata=metadata)
    if mask_kind == "3d":
        cfg["mask_var"] = "weights"
    (tmp_path / "pocs.yml").write_text(yaml.safe_dump(cfg))
    step13.main(["13_cube_interpolate_POCS", path, "--path_pocs_parameter", str(tmp_path / "pocs.yml")])
    base = "cube_twt_FFT_soft_niter-6"
    out_dir = tmp_path / base
    names = sorted(os.listdir(out_dir))
    assert f"runtimes_{base}_vol64.txt" in names and f"parameter_{base}.yml" in names
    batch_files = [f for f in names if f.endswith(".npz")]
    assert len(batch_files) == 3 and all(f.startswith(base + "_vol64_") for f in batch_files)
    lines = (out_dir / f"runtimes_{base}_vol64.txt").read_text().strip().splitlines()
    assert len(lines) == 1 and len(lines[0].split(";")) == 2 + 6 and lines[0].startswith("6;")
    assert yaml.safe_load((out_dir / f"parameter_{base}.yml").read_text())["volume"] == "reference"
    icube = open_cube(str(tmp_path / f"{base}.npz"))
    assert "volume" in icube.attrs["interp_params_keys"].split(";")
    assert icube.dims["env_interp"] == ("twt", "iline", "xline") and icube.data_vars["env_interp"].dtype == np.float32
    kw = {k: v for k, v in metadata.items() if k not in ("transform_kind", "verbose", "volume")}
    want = P.pocs_volume64(x, np.where(fold <= 1, fold, 1) if mask_kind == "2d" else mask, **kw)
    assert np.array_equal(icube.data_vars["env_interp"], want)
    assert rel_l2(want, vc.oracle(x, mask, **kw)) <= 2.0 ** -24 + LOOP_BAR
