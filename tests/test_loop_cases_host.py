"""The seeded cross-feature cases of tests/test_gpu_loop_cases.py, checked without a GPU: for every (family, seed) the GPU tests use, the generator is
reproducible, stays inside its domain (none of the excluded combinations), the oracle returns finite results for every case, the conditioning probe sets
aside no more than a quarter of a test's cases, and the cases of a parity family together still cover its features -- so that a later change to the
generator cannot silently lose a test's cases or its coverage."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loop_cases as lc  # noqa: E402

PARITY_RUNS = [(f, s) for f in lc.PARITY for s in lc.PARITY_SEEDS[f]]
PROPERTY_RUNS = [(f, s) for f in lc.FAMILIES for s in lc.PROPERTY_SEEDS]


@functools.lru_cache(maxsize=None)
def _survey(family, seed):
    """[(case, oracle results, oracle infos, accepted by the probe)] of one GPU parity test, computed once."""
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (the oracle's own: it divides by |X| = 0 under np.errstate only in part)
        for index in range(lc.PARITY_CASES[family][0]):
            case = lc.draw(family, seed, index)
            want = lc.oracle_run(case)
            rows.append((case, want[0], want[1], lc.conditioned(case, want)))
    return rows


def _assert_same_case(a, b):
    assert a.name == b.name and a.kind == b.kind
    assert a.cube.dtype == b.cube.dtype and np.array_equal(a.cube, b.cube) and np.array_equal(a.wide, b.wide) and np.array_equal(a.mask, b.mask)
    assert a.kw == b.kw and a.call == b.call
    assert (a.zero, a.pick, a.pools, a.narrowed, a.weights) == (b.zero, b.pick, b.pools, b.narrowed, b.weights)


def _check_domain(case):
    n, nil, nxl = case.cube.shape
    assert case.mask.shape in ((nil, nxl), (n, nil, nxl)) and case.mask.min() >= 0 and case.mask.max() <= 1
    assert not case.cube[case.zero].any() and 0 <= case.pick < n
    assert all((case.mask[s] if case.mask.ndim == 3 else case.mask).any() for s in range(n))
    if case.family in lc.PARITY:
        assert not lc.violations(case), (lc.describe(case), lc.violations(case))
        assert 3 <= n <= 5 and 2 <= case.kw["niter"] <= (6 if case.family == "wav64" else 11)
        assert case.narrowed == (case.cube.dtype in (np.float32, np.complex64)) and case.wide.dtype in (np.float64, np.complex128)
        assert np.array_equal(case.wide, case.cube.astype(case.wide.dtype))
        assert case.call.get("precision") == ("reference" if case.narrowed or case.family == "dct64" else None)
        assert case.kw["alpha"] in ((0.8, 0.7) if case.kw["version"] == "adaptive" else (1.0, 0.9))
        assert not (case.kw["sqrt_decay"] and case.kw["thresh_model"] == "data-driven")
        assert (case.kw["decay_kind"] == "factors") == case.kw["thresh_op"].endswith("-percentile")
        limit = dict(fft64=1 << 16, dct64=300 * 300, wav64=260 * 260, shear64=1 << 14)[case.family]
        assert nil * nxl <= limit
    else:
        assert case.cube.dtype in (np.float32, np.complex64) and case.call["precision"] == "float32"
        assert case.kw["alpha"] == 1.0 and case.kw["eps"] == 0.0 and set(np.unique(case.mask)) <= {0.0, 1.0}
        if case.family == "wav32":
            assert lc.wavelet_taps()[case.call["wavelet"]] <= 64
    if case.kind == "WAVELET":
        assert min(nil, nxl) >= 2 * (lc.wavelet_taps()[case.call["wavelet"]] - 1)


@pytest.mark.parametrize("family,seed", PARITY_RUNS, ids=[f"{f}-{s}" for f, s in PARITY_RUNS])
def test_parity_cases_are_reproducible_finite_and_mostly_well_conditioned(family, seed):
    rows = _survey(family, seed)
    ncases, least = lc.PARITY_CASES[family]
    assert len(rows) == ncases and 4 * (ncases - least) <= ncases
    for index, (case, outs, infos, _) in enumerate(rows):
        _check_domain(case)
        assert all(np.isfinite(o).all() for o in outs), lc.describe(case)
        assert infos[case.zero]["niterations"] == 0 and not outs[case.zero].any()
        assert all(1 <= i["niterations"] <= case.kw["niter"] for s, i in enumerate(infos) if s != case.zero), lc.describe(case)
        again = lc.draw(family, seed, index, derive_eps=False)       # (the oracle run behind eps is deterministic: held by the first case of each run below)
        again.kw["eps"] = case.kw["eps"]
        _assert_same_case(case, again)
    _assert_same_case(rows[0][0], lc.draw(family, seed, 0))
    accepted = sum(ok for *_, ok in rows)
    print(f"{family} seed {seed}: {accepted} of {ncases} cases accepted by the conditioning probe")
    assert accepted >= least, [lc.describe(c) for c, _, _, ok in rows if not ok]


@pytest.mark.parametrize("family", lc.PARITY)
def test_parity_seeds_together_cover_the_features_of_their_family(family):
    pairs = [(case, infos) for seed in lc.PARITY_SEEDS[family] for case, _, infos, _ in _survey(family, seed)]
    assert not lc.coverage_gaps(family, pairs)
    if family == "wav64":
        assert len({c.call["wavelet"] for c, _ in pairs}) > 6      # (banks beyond the six the other tests name)
    if family == "fft64":
        assert any(c.kw["thresh_model"] == "data-driven" for c, _ in pairs) and any(c.kw["p_min"] == "adaptive" for c, _ in pairs)
    assert any(c.kw["sqrt_decay"] for c, _ in pairs)


@pytest.mark.parametrize("family,seed", PROPERTY_RUNS, ids=[f"{f}-{s}" for f, s in PROPERTY_RUNS])
def test_bit_for_bit_cases_are_reproducible_and_inside_their_domain(family, seed):
    for index in range(lc.PROPERTY_CASES[family]):
        case = lc.draw(family, seed, index, derive_eps=False)
        _check_domain(case)
        assert case.kw["eps"] == 0.0
        _assert_same_case(case, lc.draw(family, seed, index, derive_eps=False))


def test_property_families_include_per_slice_masks_and_both_dct_norms():
    cases = {f: [lc.draw(f, s, i, derive_eps=False) for s in lc.PROPERTY_SEEDS for i in range(lc.PROPERTY_CASES[f])] for f in lc.PROPERTY}
    for family, drawn in cases.items():
        assert any(c.mask.ndim == 3 for c in drawn) and any(c.mask.ndim == 2 for c in drawn), family
        assert any(np.iscomplexobj(c.cube) for c in drawn) and any(not np.iscomplexobj(c.cube) for c in drawn), family
    assert {c.call["dct_norm"] for c in cases["dct32"]} == {"backward", "ortho"}


def test_violations_names_each_excluded_combination():
    """The check itself: a case moved into each of the four exclusions is reported."""
    case = lc.draw("fft64", 0, 0, derive_eps=False)
    real, cplx = case.cube.real.astype(np.float64), case.cube.astype(np.complex128)

    def bad(cube, kind="FFT", **kw):
        probe = lc.SimpleNamespace(cube=cube, kind=kind, kw=dict(case.kw, **kw))
        return [v[0] for v in lc.violations(probe)]

    assert bad(real, thresh_op="soft", thresh_model="linear", p_min=1e-2) == []
    assert bad(real, thresh_op="hard", thresh_model="inverse_proportional-2", p_min=1e-2) == ["1"]
    assert bad(real, thresh_op="hard-percentile", thresh_model="linear", p_min=50.0) == ["2"]
    assert bad(cplx, thresh_op="hard-percentile", thresh_model="linear", p_min=50.0) == []
    assert bad(cplx, thresh_op="garrote", thresh_model="linear", p_min=1e-2) == ["3"]
    assert bad(real, thresh_op="garrote", thresh_model="data-driven", p_min=1e-2) == ["3"]
    assert bad(cplx, thresh_op="garrote-percentile", thresh_model="linear", p_min=50.0) == []
    assert bad(cplx, thresh_op="soft", thresh_model="linear", p_min="adaptive") == ["4"]
    assert bad(real, kind="WAVELET", thresh_op="soft", thresh_model="linear", p_min="adaptive") == ["4"]
    assert bad(real, kind="DCT", thresh_op="soft", thresh_model="linear", p_min="adaptive") == []
