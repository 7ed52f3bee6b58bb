"""The persistent column pass of 1024-point columns (col_pipe_kernel<1024, 8>: tables copied once, the next tile prefetched) against the
one-launch pass (P3D_NO_COLPIPE=1), bit for bit: result cube, iteration counts and the share of kept column blocks (which is a count of
the tile flags either pass writes).  Selected with P3D_FORCE_COLPIPE=1 where it is not the default."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER = 6


def _run(cube, mask, max_slices, eps, niter):
    from pseudo_3d_interpolation_amd import _ffi as ffi
    from pseudo_3d_interpolation_amd.functions.POCS import _schedule_from_stats
    n, nil, nxl = cube.shape
    maskf = mask.astype(np.float32)
    with ffi.Plan(nil, nxl, max_slices) as plan:
        x, o, m = plan.alloc(cube.nbytes).upload(cube), plan.alloc(cube.nbytes), plan.alloc(maskf.nbytes).upload(maskf)
        st = plan.prime_dev(x.ptr, ffi.P3D_C64, m.ptr, n)
        tau = _schedule_from_stats(st, nil * nxl, "exponential", niter, 0.99, 1e-2, "values")
        done, sums, _ = plan.run_dev(x.ptr, ffi.P3D_C64, m.ptr, tau, niter, o.ptr, n, thresh_op="hard", eps=eps, primed=True, want_sums=eps > 0)
        got = o.download(cube.shape, np.complex64)
        frac = plan.last_sparsity()
        for b in (x, o, m):
            b.free()
    return got, list(done), frac


# nil = 256 (32 tiles per slice): 5 slices = 160 tiles, one per workgroup (odd run); 17 slices = 544 tiles over 512 workgroups, runs of two
# (even, the last workgroups idle).  nil = 1024 (128 tiles per slice): 3 slices = 384 tiles, one per workgroup; 5 slices = 640 tiles, runs of
# two with a ragged end; 9 slices = 1152 tiles, runs of three (odd).
@pytest.mark.parametrize("nil,nslices,extra,eps", [(256, 5, 0, 0.0), (256, 17, 0, 0.0), (1024, 3, 0, 0.0), (1024, 5, 2, 0.0), (1024, 9, 0, 0.0),
                                                   (256, 5, 3, 1e-2)])
@pytest.mark.parametrize("sparse", [True, False])
def test_persistent_column_pass_is_the_one_launch_pass(nil, nslices, extra, eps, sparse, monkeypatch):
    from oracle import pocs_oracle as orc
    nxl = 1024
    niter = NITER + 4 if eps > 0 else NITER     # (the convergence test starts at the fourth iteration: cost = (d sum|x| / sum|x|)^2 < eps)
    mask = orc.synthetic_mask(nil, nxl, 0.8)
    cube = (np.stack([orc.synthetic_slice(nil, nxl, 900 + s) for s in range(nslices)]) * mask).astype(np.complex64)
    monkeypatch.setenv("P3D_NO_SPARSE", "1") if not sparse else monkeypatch.delenv("P3D_NO_SPARSE", raising=False)
    monkeypatch.setenv("P3D_NO_COLPIPE", "1")
    monkeypatch.delenv("P3D_FORCE_COLPIPE", raising=False)
    ref, done_ref, frac_ref = _run(cube, mask, nslices + extra, eps, niter)
    monkeypatch.delenv("P3D_NO_COLPIPE")
    monkeypatch.setenv("P3D_FORCE_COLPIPE", "1")
    got, done, frac = _run(cube, mask, nslices + extra, eps, niter)
    if sparse:
        assert 0.0 < frac_ref < 1.0        # tiles that keep something and tiles that do not
    if eps > 0:
        assert min(done_ref) < niter, done_ref   # the early exit switched slices off mid-job
    else:
        assert done_ref == [niter] * nslices
    assert done == done_ref and frac == frac_ref
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8))
