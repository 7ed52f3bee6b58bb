"""Seeded test volumes for 3-D FFT POCS (``pocs_volume``), the float64 oracle for them and the reference's own single-precision run.  NumPy / SciPy
only: importable without a GPU and without the built library.

Volume ``i`` of ``SHAPES`` is ``stack(synthetic_slice(n1, n2, 11 i + s, real) for s in range(n0)) * (mask > 0)``, narrowed to complex64 / float32.  The
masks come from ``default_rng([20261021, i, real])`` with 60 % missing and the first sample observed, in three kinds: ``'2d'`` (n1, n2), ``'3d'``
(n0, n1, n2) and ``'weights'``, the 2-D mask times column weights U(0.5, 1).  The shapes cover radices 2 / 3 / 5 / 7 along the first axis, mixed
lengths, n0 = 1 and planes of 24 and 35 positions, which do not fill a tile of the axis-0 pass.

The float64 oracle is ``oracle.pocs_oracle.pocs_slice`` with ``np.fft.fftn`` / ``ifftn`` injected, unchanged: a 2-D mask broadcasts over the volume.
``reference32`` is the same function on the narrowed volume with SciPy's ``fftn`` / ``ifftn`` on complex64 (every transform narrows its argument): what the
reference computes with single-precision transforms.  Its distance from the oracle is the yardstick for what any float32 implementation can be held to.
"""
from functools import lru_cache

import numpy as np

SEED = 20261021
SHAPES = ((1, 16, 16), (2, 8, 8), (3, 5, 7), (8, 16, 32), (12, 20, 24), (16, 32, 32), (35, 6, 10), (64, 8, 8), (100, 4, 6))
FFT3_EXTRA_SHAPES = ((1024, 4, 8), (729, 2, 3), (625, 3, 2), (343, 2, 2))
MASK_KINDS = ("2d", "3d", "weights")
OPERATORS = ("hard", "soft", "garrote")
VERSIONS = ("regular", "fast", "adaptive")
MISSING = 0.6
NITER = 8

BAR = 1e-5               # the project's bar against the float64 oracle
REAL_TAU_CLAIM = 4.1e-7  # real thresholds: the reference's single-precision run stays this close to the oracle on every case (a figure of two digits)
SET_ASIDE_BAR = 2.5e-6   # default schedule: a case may be set aside when the reference's single-precision run leaves the oracle by more than this ...
SET_ASIDE_CAP = 8        # ... at most one case in eight


@lru_cache(maxsize=None)
def masks(i, real):
    """{kind: mask} of volume ``i`` (float64; read-only)."""
    n0, n1, n2 = SHAPES[i]
    rng = np.random.default_rng([SEED, i, int(real)])
    m2 = (rng.random((n1, n2)) >= MISSING).astype(np.float64)
    m2[0, 0] = 1.0
    m3 = (rng.random((n0, n1, n2)) >= MISSING).astype(np.float64)
    m3[0, 0, 0] = 1.0
    out = {"2d": m2, "3d": m3, "weights": m2 * rng.uniform(0.5, 1.0, n2)}
    for m in out.values():
        m.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _full(i, real):
    from oracle import pocs_oracle as orc
    n0, n1, n2 = SHAPES[i]
    return np.stack([orc.synthetic_slice(n1, n2, 11 * i + s, real) for s in range(n0)])


@lru_cache(maxsize=None)
def volume(i, real, kind):
    """(x, mask): the observed volume (complex64, or float32 for ``real``) and its mask of kind ``kind`` (float64).  Both read-only."""
    mask = masks(i, real)[kind]
    x = (_full(i, real) * (mask > 0)).astype(np.float32 if real else np.complex64)
    x.setflags(write=False)
    return x, mask


def grid():
    """(operator, version, mask kind, real) in a fixed order: the 54 combinations every shape is run with."""
    return [(op, ver, kind, real) for op in OPERATORS for ver in VERSIONS for kind in MASK_KINDS for real in (False, True)]


def alpha_of(version):
    return 0.8 if version == "adaptive" else 1.0


def real_tau_kwargs(x, op, version):
    """Test 4: real thresholds (continuous in the reference): factors 0.5 max|X0| ... 0.01 max|X0|, 8 iterations."""
    peak = float(np.abs(np.fft.fftn(x.astype(np.complex128))).max())
    return dict(niter=NITER, thresh_op=op, thresh_model="exponential", eps=0.0, alpha=alpha_of(version), p_max=0.5 * peak, p_min=0.01 * peak,
                decay_kind="factors", version=version)


def default_kwargs(op, version, model):
    """Test 5: the default schedule (complex thresholds p * X0.max()), 8 iterations."""
    return dict(niter=NITER, thresh_op=op, thresh_model=model, eps=0.0, alpha=alpha_of(version), p_max=0.99, p_min=1e-2, decay_kind="values", version=version)


def oracle(x, mask, info=None, **kw):
    """The float64 oracle of ``pocs_volume``: pocs_slice with fftn / ifftn on the widened volume."""
    from oracle import pocs_oracle as orc
    wide = x.astype(np.float64 if x.dtype == np.float32 else np.complex128)
    return np.asarray(orc.pocs_slice(wide, mask, fwd=np.fft.fftn, inv=np.fft.ifftn, info=info, **kw))


def reference32(x, mask, **kw):
    """The reference's own single-precision run: the same loop on the complex64 / float32 volume with SciPy's fftn / ifftn on complex64 (SciPy keeps single
    precision).  NumPy promotes the iterate to double wherever a float64 scalar or mask touches it (the soft / garrote gains, the re-insertion weights), so
    every transform narrows its argument first: all 2 x niter + 1 transforms then run in single precision, as they do on the device, and the pointwise steps
    in between in NumPy's own arithmetic.  (Without the narrowing the soft / garrote runs are double-precision runs from the first threshold on and measure
    nothing.)"""
    import scipy.fft

    from oracle import pocs_oracle as orc

    def fwd(a):
        return scipy.fft.fftn(np.asarray(a).astype(np.complex64))

    def inv(s):
        return scipy.fft.ifftn(np.asarray(s).astype(np.complex64))
    return np.asarray(orc.pocs_slice(x.copy(), mask, fwd=fwd, inv=inv, **kw))


def rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.complex128) - want) / np.linalg.norm(want))


@lru_cache(maxsize=None)
def real_tau_case(i, op, version, kind, real):
    """(kwargs, oracle result, rel-L2 of the reference's single-precision run from it) of one test-4 case.  Computed once, shared."""
    x, mask = volume(i, real, kind)
    kw = real_tau_kwargs(x, op, version)
    want = oracle(x, mask, **kw)
    want.setflags(write=False)
    return kw, want, rel_l2(reference32(x, mask, **kw), want)


@lru_cache(maxsize=None)
def default_case(i, op, version, kind, real, model):
    """The same for one test-5 case (``model``: 'exponential' or 'linear')."""
    x, mask = volume(i, real, kind)
    kw = default_kwargs(op, version, model)
    want = oracle(x, mask, **kw)
    want.setflags(write=False)
    return kw, want, rel_l2(reference32(x, mask, **kw), want)
