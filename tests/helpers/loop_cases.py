"""Seeded cases that cross the features of the POCS loops (transform x operator x model x schedule options x version x mask kind x batching x input
precision), the float64 oracles for them and a conditioning probe.  NumPy / SciPy only: importable without a GPU and without the built library.

``draw(family, seed, index)`` is a pure function of its arguments (``np.random.default_rng([CONSTANT, family_id, seed, index])``).

Parity families (``fft64``, ``dct64``, ``wav64``, ``shear64``): the double-precision loops, which are held to the float64 oracles.  Property
families (``fft32``, ``dct32``, ``wav32``, ``shear32``): the float32 loops, for checks that do not depend on a threshold decision (alpha = 1, a binary mask,
eps = 0: the float32 loops add their block sums atomically, test_gpu_dct.py:255, so a positive eps could make the stopping iteration depend on the order).

EXCLUSIONS of the parity domain.  Each of these is discontinuous in the REFERENCE: multiplying the observed samples by 1 + 1e-15 N(0, 1) moved the
oracle's own result by 1e-3 ... 1.5 there, so no implementation can be held to the oracle on them:
  1. ``hard`` with an ``inverse_proportional*`` model (every transform): tau_1 = max|X0| exactly, the peak coefficient sits on the threshold by construction
     (test_golden_inverse_proportional_is_threshold_sensitive).
  2. ``hard-percentile`` on REAL cubes: Hermitian pairs have equal moduli, the interpolated percentile lands on a coefficient.  Complex cubes are fine.
  3. ``garrote`` (not ``garrote-percentile``) with a complex threshold: complex cubes of every transform (test_gpu_wavelet.py:477), and ``data-driven`` on
     real FFT cubes, whose thresholds are complex spectrum values.
  4. ``p_min='adaptive'`` outside real FFT / DCT cubes.
``violations(case)`` names the ones a case breaks (none, for every case ``draw`` returns); with them removed the oracle's own movement under that
perturbation was <= 2e-15 in 219 of 220 cases (worst 8.5e-12), so ``conditioned`` (bar 1e-12, computed from the oracle alone) sets aside about 1 case in 200.
"""
import json
import os
import re
from functools import lru_cache, partial
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PACKAGE = os.path.join(ROOT, "pseudo-3d-interpolation_amd")

CONSTANT = 0x504F4353
PARITY = ("fft64", "dct64", "wav64", "shear64")
PROPERTY = ("fft32", "dct32", "wav32", "shear32")
FAMILIES = PARITY + PROPERTY
KIND = dict(fft="FFT", dct="DCT", wav="WAVELET", shear="SHEARLET")
VERSIONS = ("regular", "fast", "adaptive")
CONDITION_BAR = 1e-12
FFT32_EDGES = (2, 3, 4, 7, 8, 16, 31, 32, 64, 97, 128, 256, 509, 512, 1009, 1024, 2048)
SHEAR32_EXTENTS = (32, 48, 64, 96, 100, 128, 150)

# What the GPU tests run (tests/test_gpu_loop_cases.py) and tests/test_loop_cases_host.py checks without a GPU.  The parity seeds are picked so that the
# cases of a family together cover its features (coverage_gaps); per family (cases per seed, the least number that must be compared -- at most a quarter
# may be set aside by ``conditioned``).
PARITY_SEEDS = dict(fft64=(0, 1, 2), dct64=(0, 1, 2), wav64=(0, 4, 11), shear64=(0, 1, 2))
PARITY_CASES = dict(fft64=(12, 9), dct64=(12, 9), wav64=(6, 5), shear64=(6, 5))
PROPERTY_SEEDS = (0, 1)
PROPERTY_CASES = dict(fft64=8, dct64=8, wav64=4, shear64=4, fft32=8, dct32=8, wav32=4, shear32=4)


def kind_of(family):
    return KIND[family[:-2]]


@lru_cache(maxsize=None)
def planned_lengths():
    """Line lengths with a plan on the double-precision register engine (test_every_planned_length_of_the_double_precision_engine_transforms_like_numpy)."""
    with open(os.path.join(PACKAGE, "csrc", "p3d_mix64_plans.inc")) as f:
        return tuple(sorted(int(m) for m in re.findall(r"^X\((\d+),", f.read(), re.M)))


@lru_cache(maxsize=None)
def wavelet_taps():
    """{bank name: filter length} of every bank in wavelets.json."""
    with open(os.path.join(PACKAGE, "wavelets.json")) as f:
        return {name: len(bank["dec_lo"]) for name, bank in sorted(json.load(f)["wavelets"].items())}


@lru_cache(maxsize=8)
def frame(nil, nxl):
    from oracle import shearlet_oracle as so
    psi = so.scales_shears_and_spectra((nil, nxl))
    psi.setflags(write=False)
    return psi


def _frame_ok(psi):
    return bool(np.all(np.abs(psi).reshape(-1, psi.shape[2]).max(axis=0) > 0))   # (a shearlet without any sample: the reference's schedule divides by zero)


def _choice(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _pooled_extent(rng, pow2, planned, integers):
    """One extent from three pools with equal weight: powers of two, planned lengths of the double register engine, any integer -- each within its own
    (lo, hi).  Returns (extent, name of the pool)."""
    pool = int(rng.integers(3))
    if pool == 0:
        return int(_choice(rng, [n for n in (1 << p for p in range(1, 13)) if pow2[0] <= n <= pow2[1]])), "pow2"
    if pool == 1:
        return int(_choice(rng, [n for n in planned_lengths() if planned[0] <= n <= planned[1]])), "planned"
    return int(rng.integers(integers[0], integers[1] + 1)), "any"


def _parity_extents(rng, family):
    """(nil, nxl, pools of the two extents, transform options)."""
    while True:
        if family == "fft64":
            (nil, a), (nxl, b) = (_pooled_extent(rng, (16, 512), (16, 400), (17, 400)) for _ in range(2))
            if nil * nxl <= 1 << 16:
                return nil, nxl, (a, b), {}
        elif family == "dct64":
            (nil, a), (nxl, b) = (_pooled_extent(rng, (2, 300), (2, 300), (2, 300)) for _ in range(2))
            return nil, nxl, (a, b), {}
        elif family == "wav64":
            (nil, a), (nxl, b) = (_pooled_extent(rng, (24, 260), (24, 260), (24, 260)) for _ in range(2))
            taps = wavelet_taps()
            bank = _choice(rng, list(taps))
            if min(nil, nxl) >= 2 * (taps[bank] - 1):   # (at least one decomposition level)
                return nil, nxl, (a, b), dict(wavelet=bank)
        else:
            planned = [n for n in planned_lengths() if n <= 300]
            one = (int(_choice(rng, planned)), "planned")
            other = (int(_choice(rng, planned)), "planned") if rng.integers(2) else (int(rng.integers(24, 201)), "any")
            (nil, a), (nxl, b) = (one, other) if rng.integers(2) else (other, one)
            if nil * nxl <= 1 << 14 and _frame_ok(frame(nil, nxl)):
                return nil, nxl, (a, b), {}


def _masks(rng, n, nil, nxl, per_slice):
    """Binary masks with a missing fraction U(0.3, 0.8) each, at least one observed sample in every one: (nil, nxl) or (n, nil, nxl)."""
    out = []
    for _ in range(n if per_slice else 1):
        while True:
            m = (rng.random((nil, nxl)) >= rng.uniform(0.3, 0.8)).astype(np.float64)
            if m.any():
                break
        out.append(m)
    return np.stack(out) if per_slice else out[0]


def _slices(n, nil, nxl, first, real):
    from oracle import pocs_oracle as orc
    full = np.stack([orc.synthetic_slice(nil, nxl, first + s, real=real) for s in range(n)])
    return full.astype(np.float64 if real else np.complex128)


def _case(family, seed, index, **fields):
    case = SimpleNamespace(family=family, seed=seed, index=index, kind=kind_of(family), **fields)
    case.name = f"{family}[{seed}/{index}]"
    return case


def pocs_kwargs(case, **override):
    """Keyword arguments of ``pocs_cube`` for the case (the frame of a SHEARLET case included)."""
    kw = dict(case.kw, transform_kind=case.kind, **case.call)
    if case.kind == "SHEARLET":
        kw["auxiliary_data"] = frame(*case.cube.shape[1:])
    kw.update(override)
    return kw


def describe(case):
    n, nil, nxl = case.cube.shape
    return (f"{case.name} {n}x{nil}x{nxl} {case.cube.dtype.name} {'per-slice' if case.mask.ndim == 3 else 'shared'}{' weights' if case.weights else ''} "
            + " ".join(f"{k}={v}" for k, v in {**case.kw, **case.call}.items()))


def operators_of(family):
    return ("hard", "soft", "garrote") + (("hard-percentile", "soft-percentile", "garrote-percentile") if family == "fft64" else ())


def coverage_gaps(family, cases_and_infos):
    """What the (case, oracle infos) pairs of a parity family do NOT cover of: a per-slice mask, a weight mask, each operator, each version, a narrowed
    input, every extent pool, and eps > 0 with two slices stopping at different iterations."""
    cases = [c for c, _ in cases_and_infos]
    seen = {
        "a per-slice mask": any(c.mask.ndim == 3 for c in cases),
        "a weight mask": any(c.weights for c in cases),
        "a narrowed input": any(c.narrowed for c in cases),
        "a wide input": any(not c.narrowed for c in cases),
        "batch_slices": any(c.call["batch_slices"] for c in cases),
        "eps > 0 with slices that stop at different iterations": any(
            c.kw["eps"] > 0 and len({i["niterations"] for s, i in enumerate(infos) if s != c.zero}) > 1 for c, infos in cases_and_infos),
    }
    seen.update({f"thresh_op={op}": any(c.kw["thresh_op"] == op for c in cases) for op in operators_of(family)})
    seen.update({f"version={v}": any(c.kw["version"] == v for c in cases) for v in VERSIONS})
    seen.update({f"an extent from the pool '{p}'": any(p in c.pools for c in cases) for p in (("planned", "any") if family == "shear64" else ("pow2", "planned", "any"))})
    return sorted(k for k, v in seen.items() if not v)


def violations(case):
    """The exclusions (module docstring) that the case breaks."""
    kw, real, bad = case.kw, not np.iscomplexobj(case.cube), []
    op, model = kw["thresh_op"], kw["thresh_model"]
    if op == "hard" and "inverse_proportional" in model:
        bad.append("1: hard with an inverse_proportional model")
    if op == "hard-percentile" and real:
        bad.append("2: hard-percentile on a real cube")
    if op == "garrote" and (not real or (model == "data-driven" and case.kind == "FFT")):
        bad.append("3: garrote with a complex threshold")
    if kw["p_min"] == "adaptive" and not (real and case.kind in ("FFT", "DCT")):
        bad.append("4: p_min='adaptive' outside real FFT / DCT cubes")
    return bad


# ------------------------------------------------------------------------------------------------------------------------------------------------
# parity families
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _draw_parity(rng, family, seed, index, derive_eps):
    nil, nxl, pools, extra = _parity_extents(rng, family)
    n = int(rng.integers(3, 6))
    real = bool(rng.integers(2))
    wide = _slices(n, nil, nxl, int(rng.integers(1000)), real)
    if family == "shear64" and real:
        wide = wide + 1.5   # (a positive low-pass maximum, as tools/fuzz_r05.py)
    per_slice = bool(rng.integers(2))
    mask = _masks(rng, n, nil, nxl, per_slice)
    wide = wide * mask
    zero = int(rng.integers(n))
    wide[zero] = 0
    weights = rng.integers(4) == 0
    w = rng.uniform(0.5, 1.0, nxl)
    if weights:
        mask = mask * w

    ops = ["hard", "soft"] + (["garrote"] if real else [])
    if family == "fft64":
        ops += ["soft-percentile", "garrote-percentile"] + ([] if real else ["hard-percentile"])
    op = _choice(rng, ops)
    percentile = op.endswith("-percentile")
    models = ["exponential", "exponential-2", "linear"]
    if not percentile:
        if family != "wav64" and op != "hard":
            models += ["inverse_proportional", "inverse_proportional-2"]
        if family == "fft64" and not (real and op == "garrote"):
            models += ["data-driven"]
    model = _choice(rng, models)
    p_mins = [1e-2, 1e-3, 0.05]
    if real and family in ("fft64", "dct64") and model in ("exponential", "exponential-2", "linear"):
        p_mins += ["adaptive"]
    p_min = _choice(rng, p_mins)
    p_max = 0.99
    pct_max, pct_min = float(rng.uniform(90, 99)), float(rng.uniform(40, 70))
    if percentile:
        p_max, p_min = pct_max, pct_min
    sqrt_decay = bool(rng.integers(4) == 0) and model != "data-driven"
    norm = _choice(rng, ["backward", "ortho"])
    niter = int(rng.integers(2, 7 if family == "wav64" else 12))   # (WAVELET: the 'smooth' iteration is expansive, long runs amplify the last bit)
    version = _choice(rng, ["regular", "regular", "fast", "adaptive"])
    alpha = _choice(rng, [0.8, 0.7] if version == "adaptive" else [1.0, 1.0, 0.9])
    batch = _choice(rng, [None, 2])
    narrowed = bool(rng.integers(2))
    want_eps = bool(rng.integers(2))

    kw = dict(niter=niter, thresh_op=op, thresh_model=model, eps=0.0, alpha=float(alpha), p_max=p_max, p_min=p_min, sqrt_decay=sqrt_decay,
              decay_kind="factors" if percentile else "values", version=version)
    call = dict(batch_slices=batch, **extra)
    if family == "dct64":
        call["dct_norm"] = norm
    cube = wide
    if narrowed:
        cube = wide.astype(np.float32 if real else np.complex64)
        wide = cube.astype(wide.dtype)     # the oracle is fed what the loop is fed
    if narrowed or family == "dct64":
        call["precision"] = "reference"
    case = _case(family, seed, index, cube=cube, wide=wide, mask=mask, kw=kw, call=call, zero=zero, pick=int(rng.integers(n)), pools=pools, narrowed=narrowed,
                 weights=bool(weights))
    if want_eps and derive_eps:
        case.kw["eps"] = _eps_between_costs(oracle_run(case)[1])
    return case


def _eps_between_costs(infos):
    """The precedent of test_gpu_mask3d.py: of the costs the early exit compares (k > 2), over all slices, the two adjacent sorted values with the largest
    ratio between them; eps is their geometric mean, at least a factor 1.2 from either -- else 0."""
    costs = np.sort(np.array([c for info in infos if info["niterations"] for c in info["costs"][3:] if c > 0], dtype=np.float64))
    if costs.size < 2:
        return 0.0
    ratio = costs[1:] / costs[:-1]
    i = int(np.argmax(ratio))
    return float(np.sqrt(costs[i] * costs[i + 1])) if ratio[i] >= 1.2 ** 2 else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# property families
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _draw_property(rng, family, seed, index):
    extra = {}
    while True:
        if family == "fft32":
            nil, nxl = (int(_choice(rng, FFT32_EDGES)) if rng.integers(3) == 0 else int(rng.integers(2, 1501)) for _ in range(2))
            n = int(rng.integers(2, 6))
            if nil * nxl <= 1 << 18:
                break
        elif family == "dct32":
            nil, nxl = (int(rng.integers(2, 301)) for _ in range(2))
            n = int(rng.integers(2, 6))
            extra["dct_norm"] = _choice(rng, ["backward", "ortho"])
            break
        elif family == "wav32":
            nil, nxl = (int(rng.integers(16, 401)) for _ in range(2))
            n = int(rng.integers(2, 5))
            taps = wavelet_taps()
            bank = _choice(rng, list(taps))
            if taps[bank] <= 64 and min(nil, nxl) >= 2 * (taps[bank] - 1):
                extra["wavelet"] = bank
                break
        else:
            nil, nxl = (int(_choice(rng, SHEAR32_EXTENTS)) for _ in range(2))
            n = int(rng.integers(2, 4))
            if _frame_ok(frame(nil, nxl)):
                break
    real = bool(rng.integers(2))
    op = _choice(rng, ["hard", "soft", "garrote"])
    if op == "garrote" and not real and family in ("wav32", "shear32"):
        op = "soft"
    kw = dict(niter=int(rng.integers(1, 8)), thresh_op=op, thresh_model=_choice(rng, ["exponential", "linear"]), eps=0.0, alpha=1.0, p_max=0.99, p_min=1e-2,
              sqrt_decay=False, decay_kind="values", version=_choice(rng, ["regular", "adaptive"]))
    per_slice = bool(rng.integers(2))
    mask = _masks(rng, n, nil, nxl, per_slice)
    cube = (_slices(n, nil, nxl, int(rng.integers(1000)), real) * mask).astype(np.float32 if real else np.complex64)
    zero = int(rng.integers(n))
    cube[zero] = 0
    return _case(family, seed, index, cube=cube, wide=cube.astype(np.float64 if real else np.complex128), mask=mask, kw=kw,
                 call=dict(batch_slices=None, precision="float32", **extra), zero=zero, pick=int(rng.integers(n)), pools=None, narrowed=False, weights=False)


def draw(family, seed, index, derive_eps=True):
    """Case ``index`` of ``(family, seed)``.  ``derive_eps=False``: the same case with eps = 0 (what the bit-for-bit tests run)."""
    rng = np.random.default_rng([CONSTANT, FAMILIES.index(family), int(seed), int(index)])
    if family in PARITY:
        return _draw_parity(rng, family, seed, index, derive_eps)
    return _draw_property(rng, family, seed, index)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the oracles and the conditioning probe
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _oracle_slice(case):
    from oracle import pocs_oracle as orc
    if case.kind == "FFT":
        return orc.pocs_slice
    if case.kind == "DCT":
        from scipy.fft import dctn, idctn
        norm = case.call["dct_norm"]
        return partial(orc.pocs_slice, transform_kind="DCT", fwd=partial(dctn, norm=norm), inv=partial(idctn, norm=norm))
    if case.kind == "WAVELET":
        from oracle import wavelet_oracle as wo
        return partial(wo.pocs_slice_wavelet, wavelet=case.call["wavelet"])
    from oracle import shearlet_oracle as so
    psi = frame(*case.cube.shape[1:])
    return lambda x, m, info=None, **kw: so.pocs_slice_shearlet(x, m, psi, info=info, **kw)


def oracle_run(case, cube=None):
    """(results, infos) of the matching float64 oracle, one slice at a time with that slice's own mask; ``cube``: instead of the case's (wide) cube."""
    cube = case.wide if cube is None else cube
    fn = _oracle_slice(case)
    outs, infos = [], []
    for s in range(cube.shape[0]):
        info = {}
        outs.append(np.array(fn(cube[s].copy(), case.mask[s] if case.mask.ndim == 3 else case.mask, info=info, **case.kw)))
        infos.append(info)
    return outs, infos


def movement(case, want):
    """Per slice: (rel-L2 by which the oracle's result moves when the observed samples are multiplied by 1 + 1e-15 N(0, 1), whether its iteration count
    stays).  ``want``: ``oracle_run(case)``.  The noise is fixed (its generator does not depend on the case)."""
    noise = np.random.default_rng(CONSTANT).standard_normal(case.wide.shape)
    outs, infos = oracle_run(case, case.wide * (1.0 + 1e-15 * noise))
    moved = []
    for a, b, ia, ib in zip(outs, want[0], infos, want[1]):
        nb = np.linalg.norm(b)
        moved.append((float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b)), ia["niterations"] == ib["niterations"]))
    return moved


def conditioned(case, want):
    """False when that perturbation moves any slice of the oracle's result by more than 1e-12 rel-L2 or changes its iteration count: the reference itself is
    ill-conditioned there.  Computed from the oracle alone."""
    return all(np.isfinite(m) and m <= CONDITION_BAR and same for m, same in movement(case, want))
