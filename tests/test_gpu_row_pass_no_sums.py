"""Rows of 1024 samples, jobs that cannot read the cost sums (eps = 0 and no table asked for): the steady-state and last row passes
(row_pipe32_kernel<..., SUMS = false>) neither compute nor store the per-row sums of |x|, and the loop does not add rows up.

The iterate must not notice: `out` and the iteration counts of a job with want_sums=False are compared BIT FOR BIT with the same job
with want_sums=True (the kernels that keep the sums: the path every job took before).  The sums of the job that asks for them are
checked against what they are defined as:
  * sums[0] and sums[niter] against sum |x| of the masked input / of `out`, summed in double by NumPy.  The kernel takes |x| in float32
    (two products, a sum, a square root: <= 4 ulp), adds the 32 moduli of a lane in float32 (<= 32 ulp of the lane's sum) and goes on in
    double: a relative bound of 36 * 2^-24 = 2.2e-6 on a sum of non-negative terms; asserted at 2.5e-6.
  * sums[niter] against the 64-lane kernel family (P3D_NO_PIPE32=1, the generic row pass of the parity tests; its transforms round
    differently): |sum|a| - sum|b|| <= ||a - b||_1 for the two results, plus the rounding bound above for either sum.
  A float32 cube goes through the complex passes: its iterate is COMPLEX (the threshold compares complex numbers lexicographically, as the
  reference does, which does not keep the spectrum Hermitian), the cost is the sum of its moduli and `out` is its real part (np.real, as in
  the reference).  There the last sum is no function of `out`: only sums[niter] >= sum |out| holds (|z| >= |Re z|), and that is asserted.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER = 6
ROUNDING = 2.5e-6


def _job(nil, nslices, dtype):
    from oracle import pocs_oracle as orc
    nxl = 1024
    mask = orc.synthetic_mask(nil, nxl, 0.8)
    cube = np.stack([orc.synthetic_slice(nil, nxl, 700 + s) for s in range(nslices)]) * mask
    cube = (cube.real if dtype == np.float32 else cube).astype(dtype)
    return mask, cube


def _run(cube, mask, op, want_sums, max_slices=None):
    from pseudo_3d_interpolation_amd import _ffi as ffi
    from pseudo_3d_interpolation_amd.functions.POCS import _schedule_from_stats
    n, nil, nxl = cube.shape
    dt = ffi.P3D_F32 if cube.dtype == np.float32 else ffi.P3D_C64
    maskf = mask.astype(np.float32)
    with ffi.Plan(nil, nxl, max_slices or n) as plan:
        x, o, m = plan.alloc(cube.nbytes).upload(cube), plan.alloc(cube.nbytes), plan.alloc(maskf.nbytes).upload(maskf)
        st = plan.prime_dev(x.ptr, dt, m.ptr, n)
        tau = _schedule_from_stats(st, nil * nxl, "exponential", NITER, 0.99, 1e-2, "values")
        done, sums, _ = plan.run_dev(x.ptr, dt, m.ptr, tau, NITER, o.ptr, n, thresh_op=op, eps=0.0, primed=True, want_sums=want_sums)
        got = o.download(cube.shape, cube.dtype)
        frac = plan.last_sparsity()
        for b in (x, o, m):
            b.free()
    return got, np.asarray(done), sums, frac


@pytest.mark.parametrize("op", ["hard", "soft"])
@pytest.mark.parametrize("nil,nslices,dtype", [(256, 5, np.complex64), (256, 5, np.float32), (1024, 3, np.complex64), (1024, 3, np.float32)])
def test_job_without_cost_sums_is_the_job_with_them(nil, nslices, dtype, op, monkeypatch):
    """256 x 5: 640 units of two rows over 512 workgroups of 8 -- a ragged run; 1024 x 3: whole workgroups.  complex64 and float32 cubes
    (float32: through the complex passes, the row-pair path of the hard operator has no sums switch)."""
    monkeypatch.setenv("P3D_NO_REAL", "1")
    mask, cube = _job(nil, nslices, dtype)
    with_sums, done_w, sums, frac_w = _run(cube, mask, op, True)
    without, done_n, none, frac_n = _run(cube, mask, op, False)
    assert none is None and sums.shape == (NITER + 1, nslices)
    assert 0.0 < frac_w < 1.0 and frac_n == frac_w          # tiles that keep something and tiles that do not, in the same run
    assert (done_w == NITER).all() and (done_n == NITER).all()
    assert with_sums.dtype == dtype and np.array_equal(with_sums.view(np.uint8), without.view(np.uint8))
    # the job that asks for the sums still gets them
    first = np.abs(cube.astype(np.complex128)).sum(axis=(1, 2))
    last = np.abs(with_sums.astype(np.complex128)).sum(axis=(1, 2))
    assert np.all(np.abs(sums[0] - first) <= ROUNDING * first), (sums[0], first)
    if dtype == np.float32:
        assert np.all(sums[NITER] >= last * (1.0 - ROUNDING)), (sums[NITER], last)
    else:
        assert np.all(np.abs(sums[NITER] - last) <= ROUNDING * last), (sums[NITER], last)
    assert np.all(sums[1:] > 0) and np.all(np.isfinite(sums))
    # ... and they are the sums of the generic row pass, up to what the two families' results differ by
    monkeypatch.setenv("P3D_NO_PIPE32", "1")
    generic, done_g, sums_g, _ = _run(cube, mask, op, True)
    assert (done_g == NITER).all()
    assert np.all(np.abs(sums_g[0] - sums[0]) <= 2 * ROUNDING * first)
    l1 = np.abs(generic.astype(np.complex128) - with_sums.astype(np.complex128)).sum(axis=(1, 2))
    assert dtype == np.float32 or np.all(np.abs(sums_g[NITER] - sums[NITER]) <= l1 + 2 * ROUNDING * last), (sums_g[NITER], sums[NITER], l1)


def test_plan_wider_than_the_job_and_a_switched_off_slice(monkeypatch):
    """A plan of 8 slices running 5, one of them switched off by the caller (`done` flags in use without the early exit): the passes
    without the sums honour both, like the ones with them."""
    from pseudo_3d_interpolation_amd import _ffi as ffi
    from pseudo_3d_interpolation_amd.functions.POCS import _schedule_from_stats
    mask, cube = _job(256, 5, np.complex64)
    cube[2] = 0
    maskf = mask.astype(np.float32)
    res = {}
    with ffi.Plan(256, 1024, 8) as plan:
        x, o, m = plan.alloc(cube.nbytes).upload(cube), plan.alloc(cube.nbytes), plan.alloc(maskf.nbytes).upload(maskf)
        for want in (True, False):
            o.upload(np.full(cube.shape, 7 + 7j, np.complex64))
            st = plan.prime_dev(x.ptr, ffi.P3D_C64, m.ptr, 5)
            active = st[:, 2] > 0
            st[~active] = 1.0
            tau = _schedule_from_stats(st, 256 * 1024, "exponential", NITER, 0.99, 1e-2, "values")
            done, _, _ = plan.run_dev(x.ptr, ffi.P3D_C64, m.ptr, tau, NITER, o.ptr, 5, thresh_op="hard", eps=0.0, active=active, primed=True, want_sums=want)
            res[want] = (o.download(cube.shape, np.complex64), np.asarray(done), plan.last_sparsity())
        for b in (x, o, m):
            b.free()
    assert not active[2] and list(res[True][1]) == [NITER, NITER, 0, NITER, NITER] and np.array_equal(res[True][1], res[False][1])
    assert not res[False][0][2].any() and 0.0 < res[False][2] < 1.0 and res[False][2] == res[True][2]
    assert np.array_equal(res[True][0].view(np.uint8), res[False][0].view(np.uint8))
