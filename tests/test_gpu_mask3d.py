"""Per-slice masks on the GPU: ``mask`` of shape (nslices, nil, nxl) in every batched POCS loop.

Parity: slice ``s`` of the result -- the iterate, ``niterations`` and ``costs`` -- is the oracle's single-slice result for ``(cube[s], mask[s])``.
Every case has 5 slices with five different masks (``synthetic_mask`` at missing fractions 0.3 ... 0.7), slice 2 all zero, ``batch_slices=2`` (batches
start at mask offsets 0, 2 and 4), the soft operator (continuous: no keep / zero flips), the exponential model, 10 iterations and an ``eps`` under which
the slices stop at different iterations.  ``eps`` is chosen per case from the ORACLE's costs (double precision, CPU): the value that lies furthest, as a
ratio, from every cost the early exit compares with it -- at least a factor 1.2 in every case, against the 2 % by which float32 costs may differ
(test_gpu_wavelet.py:111) -- so that the stopping iteration is not a coin toss between float32 and double.

Tolerances are the constants of the existing parity tests for the same operator and oracle: 1e-5 rel-L2 for the float32 loops (test_gpu_parity.py:13
``TOL``; test_gpu_wavelet.py:104; test_gpu_shearlet.py:109; test_gpu_dct.py:159), 1e-10 for the double-precision loops (test_gpu_parity.py:850;
test_gpu_wavelet.py:492; test_gpu_shearlet.py:398); costs to rtol 2e-2 / atol 1e-12 in float32 (test_gpu_wavelet.py:111) and rtol 1e-6 / atol 1e-18 in
double (test_gpu_parity.py:853)."""
import ctypes as C
import functools
import os
from functools import partial

import numpy as np
import pytest
import yaml

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 1e-5, 1e-10
FRACTIONS = (0.3, 0.4, 0.5, 0.6, 0.7)
SEED = 100
BASE = dict(niter=10, thresh_op="soft", thresh_model="exponential", p_max=0.99, p_min=1e-2)


@pytest.fixture(scope="module")
def P():
    from pseudo_3d_interpolation_amd import _ffi
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    assert _ffi.device_count() >= 1, "no GPU visible"
    yield mod
    mod.release_plans()


@functools.lru_cache(maxsize=None)
def _masks(nil, nxl):
    from oracle import pocs_oracle as orc
    m = np.stack([orc.synthetic_mask(nil, nxl, f) for f in FRACTIONS])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _cube(nil, nxl, real):
    """Five observed slices under their own masks, slice 2 all zero; complex128 / float64 (the tests narrow it)."""
    from oracle import pocs_oracle as orc
    full = np.stack([orc.synthetic_slice(nil, nxl, SEED + s, real=real) for s in range(len(FRACTIONS))])
    cube = (full * _masks(nil, nxl)).astype(np.float64 if real else np.complex128)
    cube[2] = 0
    cube.setflags(write=False)
    return cube


def _psi(shape):
    from pseudo_3d_interpolation_amd.functions import shearlets
    return shearlets.scalesShearsAndSpectra(shape)


def _oracle_slice(kind, shape, extra):
    """The oracle's single-slice function for a loop: f(x, mask, info=..., **kw)."""
    from oracle import pocs_oracle as orc
    from oracle import shearlet_oracle as so
    from oracle import wavelet_oracle as wo
    if kind == "FFT":
        return orc.pocs_slice
    if kind == "DCT":
        from scipy.fft import dctn, idctn
        norm = extra["dct_norm"]
        return partial(orc.pocs_slice, transform_kind="DCT", fwd=partial(dctn, norm=norm), inv=partial(idctn, norm=norm))
    if kind == "WAVELET":
        return partial(wo.pocs_slice_wavelet, wavelet=extra["wavelet"])
    psi = _psi(shape)
    return lambda x, m, info=None, **kw: so.pocs_slice_shearlet(x, m, psi, info=info, **kw)


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, real, extra_items, kw_items):
    """(results, infos) of the oracle, slice by slice with that slice's mask; computed once per case and shared."""
    extra, kw = dict(extra_items), dict(kw_items)
    cube, masks = _cube(*shape, real), _masks(*shape)
    fn = _oracle_slice(kind, shape, extra)
    outs, infos = [], []
    for s in range(cube.shape[0]):
        info = {}
        outs.append(np.array(fn(cube[s].copy(), masks[s], info=info, **kw)))
        infos.append(info)
    return outs, infos


def _run(P, kind, shape, real, double, extra, kw, masks=None, batch_slices=2):
    cube = _cube(*shape, real)
    if not double:
        cube = cube.astype(np.float32 if real else np.complex64)
    call = dict(extra)
    if kind == "SHEARLET":
        call["auxiliary_data"] = _psi(shape)
    res = []
    got = P.pocs_cube(np.array(cube), _masks(*shape) if masks is None else masks, transform_kind=kind, results=res, batch_slices=batch_slices, **call, **kw)
    return got, res


def _check_parity(P, kind, shape, real, double, extra, kw):
    got, res = _run(P, kind, shape, real, double, extra, kw)
    want, infos = _reference(kind, shape, real, tuple(sorted(extra.items())), tuple(sorted(kw.items())))
    tol = TOL64 if double else TOL32
    assert not got[2].any() and res[2]["niterations"] == 0
    its = []
    for s in (0, 1, 3, 4):
        err = rel_l2(got[s], want[s])
        print(f"{kind} {shape} {'double' if double else 'float32'} slice {s}: rel-L2 {err:.3e}, niterations {res[s]['niterations']} (oracle {infos[s]['niterations']})")
        assert err <= tol, (s, err)
        assert res[s]["niterations"] == infos[s]["niterations"], (s, res[s]["niterations"], infos[s]["niterations"])
        if double:
            np.testing.assert_allclose(res[s]["costs"], infos[s]["costs"], rtol=1e-6, atol=1e-18)
        else:
            np.testing.assert_allclose(res[s]["costs"], infos[s]["costs"], rtol=2e-2, atol=1e-12)
        its.append(res[s]["niterations"])
    if kw.get("eps", 0) > 0:
        assert len(set(its)) > 1, its      # the slices of a batch stop at different iterations


# (kind, shape, real cube, double-precision loop, transform options, eps, what else differs from BASE)
PARITY = [
    # FFT float32: the resident path's territory (which a per-slice job must not take), a shape that is no power of two, a tuned plan
    ("FFT", (64, 32), False, False, {}, 3.89e-4, {}),
    ("FFT", (24, 40), False, False, {}, 3.8e-3, {}),
    ("FFT", (256, 256), False, False, {}, 1.0e-3, {}),
    # more than 65536 points per slice: the update kernel has at most 256 blocks of 256 threads per slice, so its grid-stride loop makes a second pass
    # and reads mask[s * stride + i] with i beyond the first one (at 256 x 256 every thread makes exactly one pass)
    ("FFT", (320, 256), False, False, {}, 2.0e-5, {}),
    ("FFT", (24, 40), False, False, {}, 5.13e-3, dict(version="adaptive", alpha=0.8)),        # APOCS: the adaptive mix uses m
    ("FFT", (24, 40), True, False, {}, 6.61e-3, {}),                                           # a real cube (not the half-spectrum path)
    ("DCT", (24, 40), False, False, dict(dct_norm="backward"), 9.55e-3, {}),
    ("DCT", (24, 40), False, False, dict(dct_norm="ortho"), 8.51e-3, {}),
    ("WAVELET", (64, 80), True, False, dict(wavelet="coif5"), 2.24e-4, {}),                    # test_wavelet_pocs_vs_oracle's shape and wavelet
    ("SHEARLET", (48, 64), True, False, {}, 2.24e-3, {}),                                      # test_shearlet_pocs_vs_oracle's shape
    ("SHEARLET", (33, 31), True, True, {}, 1.05e-4, {}),                                       # the smallest of test_shearlet_loop_in_the_reference_precision
    ("FFT", (24, 40), False, True, {}, 3.8e-3, {}),
    ("FFT", (64, 32), False, True, {}, 3.89e-4, {}),
    ("WAVELET", (33, 70), True, True, dict(wavelet="db2"), 2.88e-4, {}),                       # the smallest of test_wavelet_loop_in_the_reference_precision
]


@pytest.mark.parametrize("kind,shape,real,double,extra,eps,more", PARITY,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-{'real' if c[2] else 'cplx'}-{'f64' if c[3] else 'f32'}" + "".join(f"-{v}" for v in list(c[4].values()) + list(c[6].values()))
                              for c in PARITY])
def test_every_slice_is_the_oracles_result_for_its_own_mask(P, kind, shape, real, double, extra, eps, more):
    _check_parity(P, kind, shape, real, double, extra, dict(BASE, eps=eps, **more))


def test_hard_percentile_with_one_mask_per_slice(P):
    """The -percentile operators rank the whole spectrum; a per-slice job takes the unfused passes for them as for everything else.  Percentages inside the
    bulk of the distribution, as test_percentile_operators_vs_oracle (test_gpu_parity.py:680) has them; its tolerance (line 684)."""
    kw = dict(niter=8, thresh_op="hard-percentile", thresh_model="linear", decay_kind="factors", eps=0, p_max=97.0, p_min=60.0)
    got, res = _run(P, "FFT", (24, 40), False, False, {}, kw)
    want, infos = _reference("FFT", (24, 40), False, (), tuple(sorted(kw.items())))
    assert not got[2].any()
    for s in (0, 1, 3, 4):
        assert rel_l2(got[s], want[s]) < TOL32, (s, rel_l2(got[s], want[s]))
        assert res[s]["niterations"] == infos[s]["niterations"] == 8


# ---- consistency with the shared-mask call --------------------------------------------------------------------------------------------------
SAME_BITS = [
    ("DCT", (24, 40), False, False, dict(dct_norm="ortho")),
    ("WAVELET", (64, 80), True, False, dict(wavelet="coif5")),
    ("WAVELET", (64, 80), False, False, dict(wavelet="db4")),      # (db4: the fused level-1 kernel, which reads a shared 0 / 1 mask as bits)
    ("SHEARLET", (48, 64), True, False, {}),
    ("FFT", (24, 40), False, True, {}),
    ("FFT", (64, 32), False, True, {}),
    ("WAVELET", (33, 70), True, True, dict(wavelet="db2")),
    ("SHEARLET", (33, 31), True, True, {}),
    ("SHEARLET", (64, 128), True, True, {}),                       # (both extents on the register engine: the three fused passes)
]


@pytest.mark.parametrize("kind,shape,real,double,extra", SAME_BITS,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-{'real' if c[2] else 'cplx'}-{'f64' if c[3] else 'f32'}" for c in SAME_BITS])
def test_identical_mask_slices_give_the_bits_of_the_shared_mask(P, kind, shape, real, double, extra):
    """The same kernels, the same arithmetic: a per-slice mask whose slices are all ONE mask is the shared-mask call, bit for bit -- and a shared-mask call
    on the same cached plan gives the same bits before and after a per-slice call (no per-slice state is left behind)."""
    kw = dict(BASE, eps=1e-3)
    one = np.array(_masks(*shape)[2])
    before, res_b = _run(P, kind, shape, real, double, extra, kw, masks=one)
    stacked, res_s = _run(P, kind, shape, real, double, extra, kw, masks=np.broadcast_to(one, (len(FRACTIONS),) + one.shape))
    own, _ = _run(P, kind, shape, real, double, extra, kw)                               # five different masks in between
    after, res_a = _run(P, kind, shape, real, double, extra, kw, masks=one)
    assert np.array_equal(stacked, before)
    assert np.array_equal(after, before)
    for other in (res_s, res_a):
        assert [r["niterations"] for r in other] == [r["niterations"] for r in res_b]
        for a, b in zip(other, res_b):   # (the float32 loops add their block sums atomically: the last bits of a cost depend on the order, test_gpu_dct.py:255)
            assert np.allclose(a["costs"], b["costs"], rtol=1e-9, atol=0.0)
    assert not np.array_equal(own, before)


@pytest.mark.parametrize("shape", [(64, 32), (256, 256)])
def test_fft_float32_identical_mask_slices_against_the_fused_paths(P, shape):
    """FFT float32: the shared-mask call takes the resident / fused passes, the per-slice one the unfused passes on the generic twin -- two paths, held
    to the tolerance test_gpu_parity.py:688 puts between a fused run and its unfused (generic twin) run: rel-L2 < TOL = 1e-5 against each other (and each
    within 1e-5 of the oracle).  A shared-mask call after the per-slice one returns the bits of the one before it."""
    from oracle import pocs_oracle as orc
    kw = dict(BASE, eps=0.0)
    one = np.array(_masks(*shape)[2])
    cube = np.array(_cube(*shape, False))
    want = orc.pocs_cube(cube, one, **kw)
    before, _ = _run(P, "FFT", shape, False, False, {}, kw, masks=one)
    stacked, _ = _run(P, "FFT", shape, False, False, {}, kw, masks=np.broadcast_to(one, (len(FRACTIONS),) + one.shape))
    after, _ = _run(P, "FFT", shape, False, False, {}, kw, masks=one)
    for s in (0, 1, 3, 4):
        assert rel_l2(before[s], want[s]) <= TOL32 and rel_l2(stacked[s], want[s]) <= TOL32, (s, rel_l2(before[s], want[s]), rel_l2(stacked[s], want[s]))
        print(f"FFT {shape} slice {s}: per-slice against shared-mask path rel-L2 {rel_l2(stacked[s], before[s]):.3e}")
        assert rel_l2(stacked[s], before[s]) < TOL32, (s, rel_l2(stacked[s], before[s]))
    assert np.array_equal(after, before)


def test_unbatched_call_and_non_binary_weights(P):
    """One batch for the whole cube (the chunk workers' default) and a per-slice mask of weights in [0, 1] (accepted like a 2-D one)."""
    from oracle import pocs_oracle as orc
    shape = (24, 40)
    kw = dict(BASE, eps=0.0, alpha=0.9)
    weights = _masks(*shape) * np.linspace(0.5, 1.0, shape[1])[None, None, :]
    cube = np.array(_cube(*shape, False)).astype(np.complex64)
    got = P.pocs_cube(cube, weights, **kw)
    for s in (0, 1, 3, 4):
        want = orc.pocs_slice(cube[s].astype(np.complex128), weights[s], **kw)
        assert rel_l2(got[s], want) <= TOL32, (s, rel_l2(got[s], want))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_p3d_pocs_run_with_the_flag_and_a_host_mask(P):
    """p3d_pocs_run through ctypes with P3D_FLAG_MASK_PER_SLICE and a HOST mask [3][24][40]: the plan stages the larger mask; the result is the Python
    path's (the same plan class, the same schedule)."""
    from pseudo_3d_interpolation_amd import _ffi
    nil, nxl, n, niter = 24, 40, 3, 6
    masks = np.ascontiguousarray(_masks(nil, nxl)[[0, 3, 4]], dtype=np.float32)
    cube = np.ascontiguousarray(np.array(_cube(nil, nxl, False))[[0, 3, 4]], dtype=np.complex64)
    kw = dict(niter=niter, thresh_op="soft", thresh_model="exponential", eps=0.0, p_max=0.99, p_min=1e-2)
    want = P.pocs_cube(cube, masks, **kw)
    assert _ffi.P3D_FLAG_MASK_PER_SLICE == 4
    lib = _ffi.lib()
    h = C.c_void_p()
    _ffi.check(lib.p3d_plan_create(C.byref(h), 0, nil, nxl, n))
    try:
        st = np.empty((n, _ffi.STATS_PER_SLICE), np.float64)
        _ffi.check(lib.p3d_pocs_stats(h, _ffi._ptr(cube), _ffi.P3D_C64, n, _ffi._ptr(st)))
        tau = _ffi._tau_table(P._schedule_from_stats(st, nil * nxl, "exponential", niter, 0.99, 1e-2, "values"), (n, niter))
        prm = _ffi.PocsParams(niter, _ffi.P3D_OP["soft"], _ffi.P3D_VER["regular"], 4, 0.0, 1.0)
        out = np.empty_like(cube)
        done = np.zeros(n, np.int32)
        for _ in range(2):   # (the second call finds the grown staging buffer)
            _ffi.check(lib.p3d_pocs_run(h, _ffi._ptr(cube), _ffi.P3D_C64, _ffi._ptr(masks), _ffi._ptr(tau), None, C.byref(prm), _ffi._ptr(out), n, _ffi._ptr(done),
                                        None, None))
            assert np.array_equal(out, want) and list(done) == [niter] * n
        # the same plan with a shared mask afterwards: the first slice's mask for all three
        prm.flags = 0
        _ffi.check(lib.p3d_pocs_run(h, _ffi._ptr(cube), _ffi.P3D_C64, _ffi._ptr(masks), _ffi._ptr(tau), None, C.byref(prm), _ffi._ptr(out), n, _ffi._ptr(done),
                                    None, None))
        # (the shared-mask call may take another path than the per-slice one: the 1e-5 of test_gpu_parity.py:688 between a fused and an unfused run;
        # slice 1 under slice 0's mask is another problem)
        assert rel_l2(out[0], want[0]) < TOL32 and rel_l2(out[1], want[1]) > 1e-3, (rel_l2(out[0], want[0]), rel_l2(out[1], want[1]))
    finally:
        lib.p3d_plan_destroy(h)


def test_several_devices_entry_point_hands_every_chunk_its_own_masks(P):
    """p3d_multi_run with the flag: every device's block, and every chunk of it, takes its own part of the mask -- the result of ONE plan over the whole
    cube, bit for bit (the pattern of test_one_process_several_devices_entry_point, test_gpu_parity.py:1371)."""
    from pseudo_3d_interpolation_amd import _ffi
    nil, nxl, niter = 24, 40, 6
    masks = np.ascontiguousarray(_masks(nil, nxl), dtype=np.float32)
    cube = np.ascontiguousarray(np.array(_cube(nil, nxl, False)), dtype=np.complex64)
    n = cube.shape[0]
    with _ffi.Plan(nil, nxl, n) as plan:
        st = plan.stats(cube)
        active = st[:, 2] > 0
        st[~active] = 1.0
        tau = P._schedule_from_stats(st, nil * nxl, "exponential", niter, 0.99, 1e-2, "values")
        want, done, sums, _ = plan.run(cube, masks, tau, niter, thresh_op="soft", eps=1e-7, active=active)
        shared, _, _, _ = plan.run(cube, masks[0], tau, niter, thresh_op="soft", eps=1e-7, active=active)
    assert not np.array_equal(want, shared)
    for devices in ([0], [0, 0], [0, 0, 0]):
        got, d2, s2 = _ffi.multi_run(cube, masks, tau, niter, devices, thresh_op="soft", eps=1e-7, active=active)
        assert np.array_equal(got, want) and np.array_equal(d2, done) and np.allclose(s2, sums, rtol=1e-12)
    with pytest.raises(ValueError):
        _ffi.multi_run(cube, masks[:-1], tau, niter, [0])


# ---- sharded entry point: the result stays on the device ----------------------------------------------------------------------------------------
BLOCK_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["P3D_ROOT"])
import torch                      # (first: torch.cuda sees the GPU only when its own HIP runtime is the one the process binds)
import numpy as np
from oracle import pocs_oracle as orc
from pseudo_3d_interpolation_amd.functions import POCS as P
from pseudo_3d_interpolation_amd.functions import shearlets
from pseudo_3d_interpolation_amd.sharding import pocs_block_on_device
base = dict(niter=6, thresh_op="soft", thresh_model="exponential", eps=0.0, p_max=0.99, p_min=1e-2)
for kind, shape, real, extra in (("FFT", (24, 40), False, {}), ("FFT", (64, 32), True, {}), ("WAVELET", (64, 80), True, dict(wavelet="coif5")),
                                 ("SHEARLET", (48, 64), True, dict(auxiliary_data=shearlets.scalesShearsAndSpectra((48, 64))))):
    masks = np.stack([orc.synthetic_mask(shape[0], shape[1], f) for f in (0.3, 0.4, 0.5, 0.6, 0.7)])
    cube = np.stack([orc.synthetic_slice(shape[0], shape[1], 100 + s, real=real) for s in range(5)]) * masks
    cube = cube.astype(np.float32 if real else np.complex64)
    cube[2] = 0
    kw = dict(base, transform_kind=kind, **extra)
    want = P.pocs_cube(cube, masks, **kw)
    got = pocs_block_on_device(cube, masks, device=0, **kw)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), (kind, shape)
    assert not np.array_equal(want, P.pocs_cube(cube, masks[0], **kw)), (kind, shape)
print("block ok")
'''


def test_block_on_device_with_one_mask_per_slice(tmp_path):
    """sharding.pocs_block_on_device with a (n, nil, nxl) mask equals pocs_cube, bit for bit (FFT: plain statistics instead of the primed first pass;
    WAVELET / SHEARLET: the batch's own part of the mask).  In a child process, as test_gpu_sharding.py runs it: torch has to bind its HIP runtime first."""
    import subprocess
    import sys

    from conftest import ROOT
    script = tmp_path / "block_worker.py"
    script.write_text(BLOCK_WORKER)
    res = subprocess.run([sys.executable, str(script)], env=dict(os.environ, P3D_ROOT=ROOT), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "block ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


# ---- step-13 driver ------------------------------------------------------------------------------------------------------------------------
def test_cli_step13_with_a_per_slice_mask_variable(P, tmp_path):
    from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
    from pseudo_3d_interpolation_amd.cube_io import Cube, open_cube, save_cube
    from oracle import pocs_oracle as orc
    nt, nil, nxl = 8, 24, 40
    live = np.stack([orc.synthetic_mask(nil, nxl, 0.3 + 0.05 * s) for s in range(nt)]).astype(np.uint8)
    live[5] *= 2                                                                # (values above 1 are clipped by the fold rule)
    data = np.stack([orc.synthetic_slice(nil, nxl, 30 + s, real=True) for s in range(nt)]).astype(np.float32) * (live > 0)
    fold = np.ones((nil, nxl), np.uint8)
    cube = Cube({'env': data, 'fold': fold, 'live': live}, {'env': ('twt', 'iline', 'xline'), 'fold': ('iline', 'xline'), 'live': ('twt', 'iline', 'xline')},
                {'twt': 0.25 * np.arange(nt), 'iline': np.arange(nil), 'xline': np.arange(nxl)},
                {'long_name': 'test cube', 'description': 'synthetic', 'history': 'made;', 'text': ''}, {}, {})
    path = save_cube(cube, str(tmp_path / 'cube_twt.npz'))
    metadata = dict(transform_kind='fft', niter=6, eps=0, thresh_op='soft', thresh_model='exponential', decay_kind='values', p_max=0.99, p_min=0.01,
                    alpha=1.0, sqrt_decay=False, version='regular', verbose=False)
    yml = tmp_path / 'pocs.yml'
    yml.write_text(yaml.safe_dump({'dim': 'twt', 'var': 'env', 'mask_var': 'live', 'batch_chunk': 3, 'output_runtime_results': True, 'metadata': metadata}))
    out_dir = tmp_path / 'out'
    step13.main(['13_cube_interpolate_POCS', path, '--path_pocs_parameter', str(yml), '--path_output_dir', str(out_dir)])
    icube = open_cube(f'{out_dir}.npz')
    params = {k: v for k, v in metadata.items() if k != 'verbose'}
    want = P.pocs_cube(data, np.where(live <= 1, live, 1), **dict(params, transform_kind='FFT'))
    assert np.array_equal(icube.data_vars['env_interp'], want)
    assert not np.array_equal(want, P.pocs_cube(data, fold, **dict(params, transform_kind='FFT')))   # (the fold mask would have given something else)
    assert icube.attrs['mask_var'] == 'live' and 'live' not in icube.data_vars
    assert len([f for f in os.listdir(out_dir) if f.endswith('.npz')]) == 3
