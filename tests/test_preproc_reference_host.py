"""The float64 references of tests/test_gpu_preproc_edges.py, checked on the CPU: the float32-storage model of the filter cascade
reduces to scipy.signal.sosfiltfilt when no group boundary is left, and the listed designs have the section counts and pad lengths
the GPU test builds its cases on (which ``sos_*_kernel<NS>`` instantiation a case reaches follows from the section count alone)."""
import numpy as np
import pytest
import scipy.signal as ss

from helpers import preproc_reference as R

IDS = [d[0] for d in R.FILTER_DESIGNS]


@pytest.mark.parametrize('name,args,nsec', R.FILTER_DESIGNS, ids=IDS)
def test_design_sections_and_padlen(name, args, nsec):
    sos, zi, padlen = R.design(args)
    assert sos.shape == (nsec, 6) and zi.shape == (nsec, 2)
    assert np.all(sos[:, 3] == 1.0)
    # an odd-order lowpass has one first-order section (one zero coefficient pair less); the others are full biquads
    assert padlen == (6 * nsec if args[2] == 'lowpass' else 3 * (2 * nsec + 1))
    # ... and it is the pad length scipy itself uses: padlen samples are refused, padlen + 1 are filtered
    with pytest.raises(ValueError, match='padlen'):
        ss.sosfiltfilt(sos, np.zeros(padlen))
    assert ss.sosfiltfilt(sos, np.zeros(padlen + 1)).shape == (padlen + 1,)


def test_every_kernel_instantiation_has_a_design():
    """Groups of 8: a cascade of n sections runs sizes 8, 8 ... and n mod 8.  The listed counts reach NS = 1 ... 8 in the fused
    kernel and NS = 8 and 1 in the grouped ones, with two groups (9, 16) and three (17)."""
    counts = sorted({d[2] for d in R.FILTER_DESIGNS})
    assert counts == [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17]
    for btype, want in (('lowpass', {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17}), ('bandpass', {1, 4, 7, 8, 9, 16, 17}), ('highpass', {1, 8, 9})):
        assert {d[2] for d in R.FILTER_DESIGNS if d[1][2] == btype} == want


@pytest.mark.parametrize('name,args,nsec', R.FILTER_DESIGNS, ids=IDS)
def test_model_without_group_boundary_is_sosfiltfilt(name, args, nsec):
    sos, zi, padlen = R.design(args)
    for nt in (padlen + 1, 1500):
        x = R.traces(nt, 5, seed=nsec)
        got = R.sosfiltfilt_f32_storage(sos, x, padlen, group=nsec + 1)
        assert got.dtype == np.float32 and got.shape == x.shape
        err = R.rel_l2(got, R.sosfiltfilt(sos, x))
        print(f'{name} nt={nt}: model(no boundary) vs sosfiltfilt {err.max():.2e}')
        assert err.max() <= 1e-7, (name, nt)

