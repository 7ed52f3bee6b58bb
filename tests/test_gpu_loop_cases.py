"""Seeded cross-feature cases (tests/helpers/loop_cases.py) on the GPU.

``test_double_loops_match_their_oracles``: every double-precision loop against its float64 oracle over the product of its features -- per-slice and weight
masks, APOCS / FPOCS, sqrt_decay, percentile operators, data-driven picks, adaptive p_min, every wavelet bank, narrowed input, batch_slices, an eps between
the oracle's costs -- on extents from the tuned powers of two, the register engine's plans and anything else (primes: LDS-image passes, chirp-z).  The only
cases set aside are those on which the ORACLE moves by more than 1e-12 under a perturbation of one part in 1e15 (``loop_cases.conditioned``: the reference
alone decides, at most a quarter of a test's cases -- tests/test_loop_cases_host.py holds the seeds to that without a GPU).

``test_batching_and_masks_do_not_change_the_bits``: properties that need no tolerance and no oracle, for the float32 loops as well.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loop_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

# seeds and case counts live beside the generator: tests/test_loop_cases_host.py checks the same runs without a GPU
PARITY_RUNS = [(f, s) for f in lc.PARITY for s in lc.PARITY_SEEDS[f]]
PROPERTY_RUNS = [(f, s) for f in lc.FAMILIES for s in lc.PROPERTY_SEEDS]

# rel-L2 against the oracle.  Wide cube, continuous operator: the project's bar for every double loop (test_gpu_parity.py:850, test_gpu_wavelet.py:492,
# test_gpu_shearlet.py:398).  Narrowed input, continuous operator: the final cast (test_gpu_parity.py:851).  Hard operators on a wide cube:
# tools/fuzz_r05.py's bars for randomly drawn hard cases.
TOL_CONTINUOUS, TOL_NARROWED = 1e-10, 2e-7
TOL_HARD = dict(fft64=1e-8, dct64=1e-8, shear64=1e-8, wav64=1e-7)


@pytest.fixture(scope="module")
def P():
    from pseudo_3d_interpolation_amd import _ffi
    from pseudo_3d_interpolation_amd.functions import POCS as mod
    assert _ffi.device_count() >= 1, "no GPU visible"
    yield mod
    mod.release_plans()


def _bound(case):
    """The rel-L2 bound of a case, None where only dtype, shape and iteration counts are held (test_gpu_wavelet.py:497: a hard threshold may flip a decision
    of the narrowed input's cast)."""
    hard = case.kw["thresh_op"].startswith("hard")
    if case.narrowed:
        return None if hard else TOL_NARROWED
    return TOL_HARD[case.family] if hard else TOL_CONTINUOUS


def _check_against_the_oracle(P, case, want, infos):
    res = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # (a fall-back to the float32 kernels says so with a RuntimeWarning)
        got = P.pocs_cube(case.cube, case.mask, results=res, **lc.pocs_kwargs(case))
    bound = _bound(case)
    errs = [rel_l2(got[s], want[s]) for s in range(len(want))]
    print(f"{lc.describe(case)}: worst slice rel-L2 {max(errs):.3e} (bound {bound}), niterations {[r['niterations'] for r in res]} "
          f"(oracle {[i['niterations'] for i in infos]})")
    assert got.dtype == case.cube.dtype and got.shape == case.cube.shape, lc.describe(case)
    assert len(res) == len(want)
    for s, err in enumerate(errs):
        where = (lc.describe(case), s)
        if s == case.zero:
            assert not got[s].any() and res[s]["niterations"] == 0, where
            continue
        assert res[s]["niterations"] == infos[s]["niterations"], where + (res[s]["niterations"], infos[s]["niterations"])
        if bound is None:
            continue
        np.testing.assert_allclose(res[s]["costs"], infos[s]["costs"], rtol=1e-6, atol=1e-18, err_msg=str(where))
        assert err <= bound, where + (err, bound)
    return max(errs)


@pytest.mark.parametrize("family,seed", PARITY_RUNS, ids=[f"{f}-{s}" for f, s in PARITY_RUNS])
def test_double_loops_match_their_oracles(P, family, seed):
    ncases, least = lc.PARITY_CASES[family]
    compared = 0
    for index in range(ncases):
        case = lc.draw(family, seed, index)
        want = lc.oracle_run(case)
        if not lc.conditioned(case, want):      # the reference alone decides; nothing below drops a case
            print(f"{lc.describe(case)}: set aside, the oracle itself moves by more than {lc.CONDITION_BAR} here")
            continue
        _check_against_the_oracle(P, case, *want)
        compared += 1
    P.release_plans()
    assert compared >= least, (family, seed, compared)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("family,seed", PROPERTY_RUNS, ids=[f"{f}-{s}" for f, s in PROPERTY_RUNS])
def test_batching_and_masks_do_not_change_the_bits(P, family, seed):
    double = family in lc.PARITY
    for index in range(lc.PROPERTY_CASES[family]):
        case = lc.draw(family, seed, index, derive_eps=False)
        what = lc.describe(case)
        cube, mask = case.cube, case.mask
        n = cube.shape[0]
        assert case.kw["eps"] == 0.0
        with warnings.catch_warnings():
            if double:
                warnings.simplefilter("error")   # (the double-precision loop it is: no fall-back to the float32 kernels)
            kw = lc.pocs_kwargs(case, batch_slices=None)
            res, res_alone, res_split, res_shared, res_stacked = [], [], [], [], []
            got = P.pocs_cube(cube, mask, results=res, **kw)
            assert got.dtype == cube.dtype and got.shape == cube.shape and np.isfinite(got).all(), what
            assert not got[case.zero].any() and res[case.zero]["niterations"] == 0, what
            if case.kw["alpha"] == 1.0 and not case.weights:
                for s in range(n):
                    keep = (mask[s] if mask.ndim == 3 else mask) > 0
                    assert np.array_equal(got[s][keep], cube[s][keep]), (what, s, "observed samples changed")
            pick = case.pick
            # (alone: with its own mask, handed over as a per-slice mask of one slice so that it takes the passes it takes inside the batch)
            alone = P.pocs_cube(cube[pick:pick + 1], mask[pick:pick + 1] if mask.ndim == 3 else mask, results=res_alone, **kw)
            assert _same(alone[0], got[pick]), (what, f"slice {pick} alone differs from the batch", float(np.abs(alone[0] - got[pick]).max()))
            split = P.pocs_cube(cube, mask, results=res_split, **dict(kw, batch_slices=max(1, n // 2)))
            assert _same(split, got), (what, "batch_slices changes the bits")
            assert [r["niterations"] for r in res_split] == [r["niterations"] for r in res], what
            if family != "fft32":   # (fft32: the shared-mask call takes the fused passes, the per-slice one the unfused ones -- test_gpu_mask3d.py holds them to 1e-5)
                one = mask[pick] if mask.ndim == 3 else mask
                shared = P.pocs_cube(cube, one, results=res_shared, **kw)
                stacked = P.pocs_cube(cube, np.ascontiguousarray(np.broadcast_to(one, (n,) + one.shape)), results=res_stacked, **kw)
                assert _same(stacked, shared), (what, "a stack of one mask differs from the shared mask")
            if double:   # no atomics in the double-precision loops (test_gpu_dct64.py:238): the costs are the same bits too
                assert res_alone[0]["costs"] == res[pick]["costs"], (what, "costs of the slice alone")
                assert [r["costs"] for r in res_split] == [r["costs"] for r in res], (what, "costs of the split run")
                assert [r["costs"] for r in res_stacked] == [r["costs"] for r in res_shared], (what, "costs of the stacked run")
        print(f"{what}: same bits alone (slice {pick}), split in batches of {max(1, n // 2)}" + ("" if family == "fft32" else ", stacked mask"))
    P.release_plans()


@pytest.mark.parametrize("shape", [(821, 2), (39, 22)])
def test_large_prime_factors_on_the_unfused_passes(P, shape):
    """Found by fft32[0/2] (four 821 x 2 slices with one mask each, 7 iterations: 2.4 s): a per-slice mask sends the float32 FFT loop to the unfused passes,
    whose line transform left the one butterfly of a prime length to a single thread.  Its outputs are now spread over the threads; the sums are the same.
    Lines of 821 points (one butterfly), of 39 = 3 x 13 and 22 = 2 x 11 (several) against the oracle, with REAL thresholds (decay_kind='factors': the soft
    operator is then continuous, no float32 decision can flip) at the 1e-5 of the float32 loops (test_gpu_parity.py:13, test_gpu_mask3d.py)."""
    from oracle import pocs_oracle as orc
    nil, nxl = shape
    masks = np.stack([orc.synthetic_mask(nil, nxl, f) for f in (0.3, 0.5, 0.6)])
    cube = (np.stack([orc.synthetic_slice(nil, nxl, 40 + s) for s in range(3)]) * masks).astype(np.complex64)
    peak = float(np.abs(np.fft.fft2(cube.astype(np.complex128))).max())
    kw = dict(niter=5, thresh_op="soft", thresh_model="linear", decay_kind="factors", p_max=0.5 * peak, p_min=0.01 * peak, eps=0.0)
    res = []
    got = P.pocs_cube(cube, masks, results=res, **kw)
    for s in range(3):
        want = orc.pocs_slice(cube[s].astype(np.complex128), masks[s], **kw)
        err = rel_l2(got[s], want)
        print(f"{nil}x{nxl} slice {s}: rel-L2 {err:.3e}")
        assert err <= 1e-5 and res[s]["niterations"] == 5, (s, err)
