"""Windowed POCS on the GPU (``pocs_cube(..., patch_shape=...)``): every window of every slice is an independent POCS job, the results are blended by a
tapered overlap-add.  The reference is the oracle composition of tests/helpers/patch_numpy.py (``pocs_slice`` per window and the blend, float64).

Parity cases: three slices of 80 x 72 (slice 1 all zero), windows of 32 x 32 with overlap 16 (4 x 4 windows: the last start of the xline axis, 40, overlaps its
neighbour by 24), rows 0-39 unobserved (the four windows that start at row 0 are inactive), 10 iterations, exponential model, and an ``eps`` under which the
windows stop at different iterations.  ``eps`` is chosen per case from the ORACLE's costs (double precision, CPU) as in test_gpu_mask3d.py: the value that lies
furthest, as a ratio, from every cost the early exit compares with it, over a few seeds of the synthetic slices -- a factor of at least 1.1 in every case
(asserted below, on the CPU; 24 active windows leave less room than the five slices of test_gpu_mask3d.py), five times the 2 % by which float32 costs may
differ.  The synthetic slices are generated in single precision, so the composition's float64 run IS its run on the float32-rounded input: rounding the
input costs the comparison nothing.

Tolerance: 1e-5 rel-L2 per slice, the project's float32 bound (README; ``TOL32`` of test_gpu_mask3d.py), for the continuous operators (soft, garrote) and the
bulk-percentile case; the hard operator is covered by the bit identities, which need no tolerance."""
import functools
import os
import sys
from functools import partial

import numpy as np
import pytest
import yaml

from conftest import rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import patch_numpy as pn  # noqa: E402

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
SHAPE = (3, 80, 72)
W, O = 32, 16
BASE = dict(niter=10, thresh_op="soft", thresh_model="exponential", p_max=0.99, p_min=1e-2)
PCT = dict(niter=8, thresh_op="hard-percentile", thresh_model="linear", decay_kind="factors", eps=0, p_max=97.0, p_min=60.0)   # test_gpu_mask3d.py:161


@pytest.fixture(scope="module")
def P():
    from pseudo_3d_interpolation_amd import _ffi
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    assert _ffi.device_count() >= 1, "no GPU visible"
    yield mod
    _ffi.PatchPlan.test_hook = None
    mod.release_plans()


@functools.lru_cache(maxsize=None)
def _input(kind, seed):
    from oracle import pocs_oracle as orc
    variant = kind
    n, nil, nxl = SHAPE
    real = variant == "real"
    full = np.stack([orc.synthetic_slice(nil, nxl, seed + s, real=real) for s in range(n)])
    fr = (0.4, 0.5, 0.6) if variant == "mask3d" else (0.5,) * n
    masks = np.stack([(np.random.default_rng(7 + int(100 * f) + (s if variant == "mask3d" else 0)).random((nil, nxl)) >= f) for s, f in enumerate(fr)]).astype(np.float32)
    masks[:, :40] = 0                      # rows 0-39 unobserved
    cube = (full * masks).astype(np.float32 if real else np.complex64)
    cube[1] = 0                            # an all-zero slice
    mask = masks if variant == "mask3d" else masks[0]
    if variant == "weights":               # every third observed trace at half weight (the data are the observed samples, as before)
        mask = mask.copy()
        obs = np.flatnonzero(mask.ravel())
        mask.ravel()[obs[::3]] = 0.5
    cube.setflags(write=False)
    mask.setflags(write=False)
    return cube, mask


# variant -> (arguments beyond BASE, eps, seed of the synthetic slices); eps and seed from the oracle composition's costs on the CPU (see the module docstring)
CASES = {
    "soft": (dict(), 1.01e-5, 310),
    "garrote": (dict(thresh_op="garrote"), 2.59e-7, 300),
    "real": (dict(), 3.45e-6, 300),
    "mask3d": (dict(), 1.82e-5, 350),
    "dct-ortho": (dict(transform_kind="DCT", dct_norm="ortho"), 9.53e-6, 310),
    "apocs": (dict(version="adaptive", alpha=0.8), 4.73e-5, 310),
    "weights": (dict(), 2.16e-2, 300),
    "hard-percentile": (dict(PCT), 0, 310),
}


def job_input(variant):
    """(cube, mask) of a parity case, read-only: complex64 (float32 for 'real'); mask (80, 72) float32 -- (3, 80, 72) for 'mask3d', weights 0 / 0.5 / 1 for
    'weights'."""
    return _input(variant if variant in ("real", "mask3d", "weights") else "soft", CASES[variant][2])


def case_kw(variant):
    more, eps, _ = CASES[variant]
    return dict(BASE, eps=eps, **more) if variant != "hard-percentile" else dict(more)


@functools.lru_cache(maxsize=None)
def reference(variant):
    """(blended cube, per-slice lists of window infos, un-blended window results) of the oracle composition; computed once per case and shared."""
    cube, mask = job_input(variant)
    kw = case_kw(variant)
    fn = None
    if kw.get("transform_kind") == "DCT":
        from scipy.fft import dctn, idctn
        from oracle import pocs_oracle as orc
        norm = kw.pop("dct_norm")
        fn = partial(orc.pocs_slice, fwd=partial(dctn, norm=norm), inv=partial(idctn, norm=norm))
    return pn.pocs_windowed(cube, mask, W, O, "hann", slice_fn=fn, **kw)


def eps_margin(infos, eps):
    """The smallest ratio between eps and a cost the early exit compares with it (iterations 4 ... of every active window, as far as it ran)."""
    r = [max(c / eps, eps / c) for row in infos for i in row if i["niterations"] for c in i["costs"][3:]]
    return min(r)


def run(P, variant, results=None, **more):
    cube, mask = job_input(variant)
    return P.pocs_cube(np.array(cube), np.array(mask), results=results, patch_shape=W, patch_overlap=O, **dict(case_kw(variant), **more))


def check_parity(P, variant, **more):
    want, infos, _ = reference(variant)
    eps = CASES[variant][1]
    res = []
    got = run(P, variant, results=res, **more)
    assert got.dtype == job_input(variant)[0].dtype and got.shape == SHAPE
    assert not got[1].any() and res[1]["niterations"] == 0 and res[1]["patches"] == [(0, 0)] * 16
    ref_rows = pn.slice_results(infos)
    its = set()
    for s in (0, 2):
        err = rel_l2(got[s], want[s])
        got_its, want_its = [p[0] for p in res[s]["patches"]], [i["niterations"] for i in infos[s]]
        print(f"{variant} slice {s}: rel-L2 {err:.3e}; window iterations {got_its} (oracle {want_its})")
        assert not got[s][:16].any()                   # only inactive windows cover rows 0-15
        assert want_its[:4] == [0] * 4 and all(want_its[4:])
        assert got_its == want_its
        assert err <= TOL32, (s, err)
        assert res[s]["niterations"] == ref_rows[s]["niterations"]
        np.testing.assert_allclose(res[s]["costs"], ref_rows[s]["costs"], rtol=2e-2, atol=1e-12)     # (float32 costs: test_gpu_wavelet.py:111)
        np.testing.assert_allclose(res[s]["cost"], ref_rows[s]["cost"], rtol=2e-2, atol=1e-12)
        its |= set(want_its[4:])
    if eps:
        assert eps_margin(infos, eps) >= 1.1, eps_margin(infos, eps)
        assert len(its) > 1, its                       # the windows stop at different iterations


# ---- 1. parity with the oracle composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(CASES))
def test_windowed_job_is_the_oracle_composition(P, variant):
    check_parity(P, variant)


def test_the_argument_is_not_ignored(P):
    """(what the parent commit did: ``patch_shape`` fell into ``**ignored`` and the whole slice was one job)"""
    whole = P.pocs_cube(np.array(job_input("soft")[0]), np.array(job_input("soft")[1]), **case_kw("soft"))
    assert rel_l2(run(P, "soft")[2], whole[2]) > 1e-3


# ---- 2. the single-kernel loop with one mask per window gives the bits of the shared-mask resident path -----------------------------------------
@pytest.mark.parametrize("win", [(32, 32), (64, 32), (64, 128)], ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("op", ["hard", "soft", "garrote"])
def test_window_results_are_the_bits_of_the_resident_path(P, win, op):
    from oracle import pocs_oracle as orc
    from pseudo_3d_interpolation_amd import _ffi
    n, nil, nxl = 3, win[0] + 24, win[1] + 40
    o = (win[0] - 24, win[1] - 20)                      # two windows along iline, three along xline
    full = np.stack([orc.synthetic_slice(nil, nxl, 310 + s) for s in range(n)])
    mask = (np.random.default_rng(11).random((nil, nxl)) >= 0.5).astype(np.float32)
    cube = (full * mask).astype(np.complex64)
    kw = dict(BASE, thresh_op=op, eps=1e-3)
    seen = []
    _ffi.PatchPlan.test_hook = lambda windows, done, active: seen.append((windows, done, active))
    try:
        P.pocs_cube(cube, mask, patch_shape=win, patch_overlap=o, **kw)
    finally:
        _ffi.PatchPlan.test_hook = None
    (windows, done, active), = seen
    wins = pn.windows((nil, nxl), win, o)
    npatch = len(wins)
    assert npatch == 6 and windows.shape == (n * npatch,) + win and active.all()
    patches = pn.patch_cube(cube, win, o)
    for p, (a, b) in enumerate(wins):
        res = []
        want = P.pocs_cube(np.ascontiguousarray(patches[p::npatch]), np.ascontiguousarray(mask[a:a + win[0], b:b + win[1]]), results=res, **kw)
        assert np.array_equal(windows[p::npatch], want), (p, rel_l2(windows[p::npatch], want))
        assert list(done[p::npatch]) == [r["niterations"] for r in res]


# ---- 3. one window that is the whole slice ----------------------------------------------------------------------------------------------------
def test_a_window_of_the_whole_slice_is_the_plain_call(P):
    from oracle import pocs_oracle as orc
    _, mask, obs = orc.synthetic_cube(64, 64, 3, 0.5)
    kw = dict(BASE, thresh_op="hard", eps=1e-3)
    r0, r1 = [], []
    plain = P.pocs_cube(obs, mask, results=r0, **kw)
    got = P.pocs_cube(obs, mask, results=r1, patch_shape=64, patch_taper="boxcar", **kw)
    assert np.array_equal(got, plain)
    assert [r["niterations"] for r in r1] == [r["niterations"] for r in r0]


# ---- 4. gather and blend alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", ["hann", "boxcar"])
@pytest.mark.parametrize("overlap", [8, 24])
@pytest.mark.parametrize("real", [False, True], ids=["cplx", "real"])
def test_gather_and_blend_return_the_input(P, taper, overlap, real):
    """mask = 1 and alpha = 1: every window returns its input exactly, so the output is the blend of up to 4 x 4 copies of x: at most 16 float32
    multiply-adds and one divide, 1e-6 is about 8 ulp over them."""
    from oracle import pocs_oracle as orc
    x = np.stack([orc.synthetic_slice(45, 70, 320 + s, real=real) for s in range(2)])
    got = P.pocs_cube(x, np.ones((45, 70), np.float32), patch_shape=32, patch_overlap=overlap, patch_taper=taper, niter=3, thresh_op="hard", eps=0, alpha=1.0,
                      p_max=0.99, p_min=1e-2)
    err = float(np.max(np.abs(got - x)) / np.max(np.abs(x)))
    print(f"{taper} overlap {overlap} {'real' if real else 'complex'}: max |out - x| / max |x| = {err:.3e}")
    assert got.dtype == x.dtype and err <= 1e-6, err


# ---- 5. the two routes ------------------------------------------------------------------------------------------------------------------------
def test_generic_route_agrees_with_the_single_kernel_route(P, monkeypatch):
    r0, r1 = [], []
    one = run(P, "soft", results=r0)
    monkeypatch.setenv("P3D_NO_PATCH_RESIDENT", "1")
    gen = run(P, "soft", results=r1)
    monkeypatch.delenv("P3D_NO_PATCH_RESIDENT")
    for s in range(SHAPE[0]):
        assert rel_l2(gen[s], one[s]) <= TOL32, (s, rel_l2(gen[s], one[s]))
        assert [p[0] for p in r1[s]["patches"]] == [p[0] for p in r0[s]["patches"]]


def test_the_switch_really_changes_the_route(P, monkeypatch):
    from pseudo_3d_interpolation_amd import _ffi
    with _ffi.Plan(32, 32, 4) as plan, _ffi.PatchPlan(plan, 40, 40, [0, 8], [0, 8], np.ones(32), np.ones(32), 1) as pp:
        md = plan.alloc(40 * 40 * 4).upload(np.ones((40, 40), np.float32))
        assert pp.resident_shape and not pp.mask_dev(md.ptr, 1, 1)
        assert pp.route("soft") and not pp.route("soft", "adaptive") and not pp.route("hard-percentile")
        monkeypatch.setenv("P3D_NO_PATCH_RESIDENT", "1")
        assert not pp.route("soft")
        monkeypatch.delenv("P3D_NO_PATCH_RESIDENT")
        md.upload(np.full((40, 40), 0.5, np.float32))
        assert pp.mask_dev(md.ptr, 1, 1) and not pp.route("soft")
        md.free()


# ---- 6. batching ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["soft", "mask3d"])
def test_batches_of_one_slice_give_the_same_bits(P, variant):
    r0, r1 = [], []
    assert np.array_equal(run(P, variant, results=r1, batch_slices=1), run(P, variant, results=r0))
    assert [r["patches"] for r in r1] == [r["patches"] for r in r0]


# ---- 7. the step-13 driver ----------------------------------------------------------------------------------------------------------------------
def test_step13_passes_the_yaml_keys_on(P, tmp_path):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, save_cube
    cube, mask = job_input("soft")
    n, nil, nxl = cube.shape
    ds = Cube({"freq_env": np.array(cube), "fold": np.array(mask).astype(np.int32)}, {"freq_env": ("freq_twt", "iline", "xline"), "fold": ("iline", "xline")},
              {"freq_twt": np.arange(n) * 10.0, "iline": np.arange(nil), "xline": np.arange(nxl)},
              {"long_name": "test cube", "description": "synthetic", "history": "made;", "text": ""}, {}, {})
    path = save_cube(ds, str(tmp_path / "cube.npz"))
    kw = case_kw("soft")
    cfg = dict(dim="freq_twt", var="freq_env", batch_chunk=2, output_runtime_results=False,
               metadata=dict(transform_kind="fft", patch_shape=[W, W], patch_overlap=O, patch_taper="hann", **kw))
    yml = str(tmp_path / "pocs.yml")
    with open(yml, "w") as fh:
        yaml.safe_dump(cfg, fh)
    full = step13.main(["x", path, "--path_pocs_parameter", yml, "--path_output_dir", str(tmp_path / "out")], return_dataset=True)
    got = full.data_vars["freq_env_interp.real"] + 1j * full.data_vars["freq_env_interp.imag"]
    assert np.array_equal(got.astype(np.complex64), run(P, "soft"))
    names = os.listdir(tmp_path / "out")
    assert any(f"_patch-{W}x{W}_" in f for f in names), names
    with open(tmp_path / "out" / "parameter_cube_FFT_soft_niter-10.yml") as fh:
        assert yaml.safe_load(fh)["patch_shape"] == [W, W]
