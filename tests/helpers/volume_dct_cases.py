"""The seeded volumes of tests/helpers/volume_cases.py for 3-D DCT POCS (``pocs_volume_dct``): the float64 oracle with SciPy's ``dctn`` / ``idctn`` and the
reference's own single-precision run.  NumPy / SciPy only: importable without a GPU and without the built library.

The volumes, masks, the 54-combination grid, ``NITER`` and ``alpha_of`` are those of ``volume_cases``; the nine shapes are also the smallest at which the
axis-0 cosine pass can go wrong: n0 = 1 (its group step alone), 2 (both indices self-paired), 3 (odd, one pair), 8, 12, 16, 35 (odd, radices 5 and 7),
64 (the 32-KiB tile edge), 100, and planes of 24 and 35 positions, which do not fill a tile.

The oracle is ``oracle.pocs_oracle.pocs_slice(wide x, mask, transform_kind='DCT', fwd=partial(dctn, norm=n), inv=partial(idctn, norm=n), ...)``, unchanged:
SciPy's ``dctn`` transforms every axis by default.  ``reference32`` is the same loop with ``dctn`` / ``idctn`` narrowing their argument to float32 /
complex64 at every transform.  A *block* is one of {real thresholds, default exponential, default linear} x {backward, ortho}: 9 shapes x 54 combinations,
243 complex and 243 real runs.
"""
from functools import lru_cache, partial

import numpy as np

import volume_cases as vc

SEED, SHAPES, FFT3_EXTRA_SHAPES, NITER = vc.SEED, vc.SHAPES, vc.FFT3_EXTRA_SHAPES, vc.NITER
grid, alpha_of, volume, masks, rel_l2 = vc.grid, vc.alpha_of, vc.volume, vc.masks, vc.rel_l2
MASK_KINDS, OPERATORS = vc.MASK_KINDS, vc.OPERATORS
NORMS = ("backward", "ortho")
SCHEDULES = ("real", "exponential", "linear")       # real thresholds as factors; the default schedule with either model
BLOCKS = tuple((sched, norm) for norm in NORMS for sched in SCHEDULES)

BAR = 1e-5               # the project's bar against the float64 oracle
SET_ASIDE_BAR = 2.5e-6   # a case may be set aside only when the reference's own single-precision run leaves the oracle by more than this ...
SET_ASIDE_CAP = 16       # ... at most one case in sixteen per block
NONE_ASIDE = (("real", "backward"),)   # complex volumes: the block in which no case is set aside; real (float32) volumes: none in any block


def _pair(norm):
    import scipy.fft
    return partial(scipy.fft.dctn, norm=norm), partial(scipy.fft.idctn, norm=norm)


def dctn64(x, norm):
    """``dctn`` of the widened volume."""
    return _pair(norm)[0](x.astype(np.float64 if x.dtype == np.float32 else np.complex128))


def real_tau_kwargs(x, op, version, norm):
    """Real thresholds (continuous in the reference): factors 0.5 max|X0| ... 0.01 max|X0| with X0 = dctn(x) of that norm, 8 iterations."""
    peak = float(np.abs(dctn64(x, norm)).max())
    return dict(niter=NITER, thresh_op=op, thresh_model="exponential", eps=0.0, alpha=alpha_of(version), p_max=0.5 * peak, p_min=0.01 * peak,
                decay_kind="factors", version=version)


def kwargs_of(x, sched, op, version, norm):
    if sched == "real":
        return real_tau_kwargs(x, op, version, norm)
    return vc.default_kwargs(op, version, sched)


def oracle(x, mask, norm, info=None, **kw):
    """The float64 oracle of ``pocs_volume_dct``: pocs_slice with dctn / idctn of ``norm`` on the widened volume."""
    from oracle import pocs_oracle as orc
    fwd, inv = _pair(norm)
    wide = x.astype(np.float64 if x.dtype == np.float32 else np.complex128)
    return np.asarray(orc.pocs_slice(wide, mask, transform_kind="DCT", fwd=fwd, inv=inv, info=info, **kw))


def reference32(x, mask, norm, **kw):
    """The reference's own single-precision run: the same loop with SciPy's dctn / idctn narrowing their argument to float32 / complex64 at every
    transform (SciPy keeps single precision), the pointwise steps in between in NumPy's own arithmetic -- as ``volume_cases.reference32`` does for fftn."""
    from oracle import pocs_oracle as orc
    f64, i64 = _pair(norm)
    narrow = np.complex64 if np.iscomplexobj(x) else np.float32

    def fwd(a):
        return f64(np.asarray(a).astype(narrow))

    def inv(s):
        return i64(np.asarray(s).astype(narrow))
    return np.asarray(orc.pocs_slice(x.copy(), mask, transform_kind="DCT", fwd=fwd, inv=inv, **kw))


@lru_cache(maxsize=None)
def case(i, sched, norm, op, version, kind, real):
    """(kwargs, oracle result, rel-L2 of the reference's single-precision run from it) of one case.  Computed once, shared, read-only."""
    x, mask = volume(i, real, kind)
    kw = kwargs_of(x, sched, op, version, norm)
    want = oracle(x, mask, norm, **kw)
    want.setflags(write=False)
    return kw, want, rel_l2(reference32(x, mask, norm, **kw), want)


def set_aside(i, sched, norm, op, version, kind, real):
    """The one criterion: the reference's single-precision run alone leaves the oracle by more than SET_ASIDE_BAR.  Never computed from a device result."""
    return not case(i, sched, norm, op, version, kind, real)[2] <= SET_ASIDE_BAR
