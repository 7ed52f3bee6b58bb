"""The frame every POCS loop shares (csrc/p3d_host.hpp, LoopFrame): a slice the caller switched off reports 0 iterations, a slice that ran
without early exit reports all of them, and the cost table has a row per iteration plus the first one.  One tiny job per plan class and, for
`Plan`, per loop behind p3d_pocs_run_dev (resident kernel, fused passes, generic pipeline).  No tolerance is involved: the assertions follow
from the mapping of the per-slice state alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER = 3


def _job(nil, nxl, dtype):
    rng = np.random.default_rng(11)
    mask = (rng.random((nil, nxl)) < 0.5).astype(np.float64)
    mask[0, 0] = 1.0
    x = rng.standard_normal((2, nil, nxl))
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal((2, nil, nxl))
    return (x * mask).astype(dtype), mask


def _check(plan, x, mask):
    _, done, sums, _ = plan.run(x, mask, 0.1, NITER, thresh_op="soft", eps=0.0, active=[1, 0])
    assert done.tolist() == [NITER, 0] and sums.shape == (NITER + 1, 2)
    _, done, sums, _ = plan.run(x, mask, 0.1, NITER, thresh_op="soft", eps=0.0, active=None)
    assert done.tolist() == [NITER, NITER] and sums.shape == (NITER + 1, 2)


@pytest.mark.parametrize("nil,nxl,switch", [(32, 32, None), (64, 256, None), (32, 32, "P3D_FORCE_GENERIC")],
                         ids=["resident", "fused", "generic"])
def test_plan_iteration_counts(nil, nxl, switch, monkeypatch):
    """32 x 32: the one-kernel resident path; 64 x 256: above its 8192 points, the fused passes; P3D_FORCE_GENERIC=1 (read when the plan is made):
    the unfused pipeline."""
    from pseudo_3d_interpolation_amd import _ffi
    if switch:
        monkeypatch.setenv(switch, "1")
    x, mask = _job(nil, nxl, np.complex64)
    with _ffi.Plan(nil, nxl, 2) as plan:
        _check(plan, x, mask)


@pytest.mark.parametrize("kind", ["Plan64", "WaveletPlan", "WaveletPlan64", "ShearletPlan", "ShearletPlan64"])
def test_other_plans_iteration_counts(kind):
    from pseudo_3d_interpolation_amd import _ffi
    nil = nxl = 32
    double = kind.endswith("64")
    x, mask = _job(nil, nxl, np.float64 if double else np.float32)
    if kind == "Plan64":
        plan = _ffi.Plan64(nil, nxl, 2)
    elif kind.startswith("Wavelet"):
        plan = getattr(_ffi, kind)(nil, nxl, 2, wavelet="db2")
    else:
        psi = np.random.default_rng(5).random((nil, nxl, 3))
        plan = getattr(_ffi, kind)(psi, max_slices=2)
    with plan:
        _check(plan, x, mask)
