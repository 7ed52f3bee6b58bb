"""Host side of transform_kind='DCT' (no GPU): which callables POCS_algorithm accepts for it, how the norm of the pair is resolved, what is refused
before anything reaches a device, the YAML key of the step-13 driver, and the schedules of get_threshold_decay(..., 'DCT', ...) against the reference's
(tests/golden/dct.npz)."""
from functools import partial

import numpy as np
import pytest

from conftest import load_golden

from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
from pseudo_3d_interpolation_amd.functions import POCS as P


def _named(name, module):
    def f(*a, **k):
        raise AssertionError('the transform callables are never called')
    f.__name__ = f.__qualname__ = name
    f.__module__ = module
    return f


dctn, idctn = _named('dctn', 'scipy.fft._realtransforms'), _named('idctn', 'scipy.fft._realtransforms')
pk_dctn, pk_idctn = _named('dctn', 'scipy.fftpack._realtransforms'), _named('idctn', 'scipy.fftpack._realtransforms')
dct, idct = _named('dct', 'scipy.fft._realtransforms'), _named('idct', 'scipy.fft._realtransforms')

ACCEPTED = [
    (dctn, idctn),
    (pk_dctn, pk_idctn),
    (partial(dctn, norm='ortho'), partial(idctn, norm='ortho')),
    (partial(dctn, norm='backward'), idctn),                                   # None and 'backward' are the same norm
    (partial(dctn, norm=None), partial(idctn, norm='backward')),
    (partial(dctn, type=2, norm='ortho', axes=(-2, -1)), partial(idctn, type=2, norm='ortho', axes=[0, 1])),
    (partial(partial(dctn, norm='ortho'), axes=None), partial(idctn, norm='ortho')),
]
REFUSED = [
    (partial(dctn, type=1), partial(idctn, type=1)),
    (partial(dctn, type=3), partial(idctn, type=3)),
    (partial(dctn, type=4), partial(idctn, type=4)),
    (partial(dctn, norm='forward'), partial(idctn, norm='forward')),
    (partial(dctn, s=(8, 8)), idctn),
    (partial(dctn, orthogonalize=True), partial(idctn, orthogonalize=True)),
    (partial(dctn, axes=(0,)), idctn),
    (dct, idct),
    (idctn, dctn),                                                             # a swapped pair
    (partial(dctn, norm='ortho'), idctn),                                      # differing norms
    (partial(dctn, norm='ortho'), partial(idctn, norm='backward')),
    (partial(dctn, np.zeros((2, 2))), idctn),                                  # a bound positional argument
    (_named('dctn', 'mypackage.transforms'), _named('idctn', 'mypackage.transforms')),
    (np.fft.fft2, np.fft.ifft2),
]


@pytest.mark.parametrize('pair', ACCEPTED)
def test_accepted_callables(pair):
    P._check_transform_callables('DCT', *pair)


@pytest.mark.parametrize('pair', REFUSED)
def test_refused_callables(pair):
    with pytest.raises(NotImplementedError, match='cannot run an arbitrary callable'):
        P._check_transform_callables('DCT', *pair)


def test_dct_is_a_hip_transform_and_pocs_algorithm_checks_its_callables():
    assert 'DCT' in P._HIP_TRANSFORMS and 'CURVELET' not in P._HIP_TRANSFORMS
    x, m = np.ones((4, 4), np.float32), np.ones((4, 4), np.uint8)
    with pytest.raises(NotImplementedError, match='cannot run an arbitrary callable'):
        P.POCS_algorithm(x, m, transform=partial(dctn, type=3), itransform=partial(idctn, type=3), transform_kind='DCT')
    with pytest.raises(NotImplementedError, match='cannot run an arbitrary callable'):
        P.POCS(x, m, transform=np.fft.fft2, itransform=np.fft.ifft2, transform_kind='dct')


def test_norm_resolution_explicit_over_keyword_over_default():
    assert P._dct_norm(None) == 'backward'                                     # SciPy's default
    assert P._dct_norm(dctn) == 'backward'
    assert P._dct_norm(partial(dctn, norm=None)) == 'backward'
    assert P._dct_norm(partial(dctn, norm='ortho')) == 'ortho'
    assert P._dct_norm(partial(partial(dctn, norm='ortho'), type=2)) == 'ortho'
    assert P._dct_norm(partial(dctn, norm='ortho'), 'backward') == 'backward'  # explicit wins
    assert P._dct_norm(dctn, 'ortho') == 'ortho'
    with pytest.raises(NotImplementedError, match='forward'):
        P._dct_norm(dctn, 'forward')


def test_data_driven_with_dct_raises_before_any_device_work():
    x, m = np.ones((2, 4, 4), np.complex64), np.ones((4, 4), np.uint8)
    with pytest.raises(NotImplementedError, match='data-driven.*DCT'):
        P.pocs_cube(x, m, transform_kind='DCT', thresh_model='data-driven', niter=3)
    with pytest.raises(NotImplementedError, match='forward'):
        P.pocs_cube(x, m, transform_kind='DCT', dct_norm='forward', niter=3)
    with pytest.raises(NotImplementedError, match='data-driven.*DCT'):
        P.POCS(x[0], m, transform=dctn, itransform=idctn, transform_kind='DCT', thresh_model='data-driven', niter=3)


def test_sharded_entry_refuses_dct_instead_of_running_another_transform(monkeypatch):
    import sys
    import types
    monkeypatch.setitem(sys.modules, 'torch', types.ModuleType('torch'))       # (the refusal comes before anything of torch is used: keep it out of this process)
    from pseudo_3d_interpolation_amd import sharding
    x, m = np.ones((2, 4, 4), np.complex64), np.ones((4, 4), np.uint8)
    with pytest.raises(NotImplementedError, match='DCT'):
        sharding.pocs_block_on_device(x, m, transform_kind='DCT', niter=3)


def test_yaml_key_of_the_step13_driver():
    import yaml
    meta = yaml.safe_load('transform_kind: dct\nniter: 5\n')
    assert step13.dct_norm_from_metadata(meta) == 'ortho'                      # absent: ortho
    assert step13.dct_norm_from_metadata(yaml.safe_load('transform_kind: DCT\ndct_norm: backward\n')) == 'backward'
    assert step13.dct_norm_from_metadata({'dct_norm': 'Ortho'}) == 'ortho'
    with pytest.raises(ValueError, match='dct_norm'):
        step13.dct_norm_from_metadata({'dct_norm': 'forward'})


def test_schedules_equal_the_reference():
    G = load_golden('dct.npz')
    n = int(G['sched_count'][0])
    assert n == 24
    for i in range(n):
        sname, model, kind, p_max, p_min, niter = [str(v) for v in G[f'sched{i:02d}_meta']]
        p_min = p_min if p_min == 'adaptive' else float(p_min)
        tau = P.get_threshold_decay(model, int(niter), 'DCT', float(p_max), p_min, G[f'sched_X0_{sname}'], kind)
        want = G[f'sched{i:02d}_tau']
        assert np.shape(tau) == want.shape and np.iscomplexobj(tau) == np.iscomplexobj(want), (i, model, kind)
        assert np.allclose(tau, want, rtol=1e-14, atol=0), (i, model, kind, p_min)
    # ... and the batch form the GPU path uses gives the same numbers from the six statistics
    X0 = G['sched_X0_niter1']
    st = np.array([[X0.max().real, X0.max().imag, np.abs(X0).max(), np.abs(X0).min(), np.linalg.norm(X0) ** 2, 0.0]])
    for model, p_min in (('exponential', 1e-3), ('linear', 'adaptive'), ('inverse_proportional', 1e-3)):
        a = P._schedule_from_stats(st, X0.size, model, 9, 0.99, p_min, 'values')[0]
        b = P.get_threshold_decay(model, 9, 'DCT', 0.99, p_min, X0, 'values')
        assert np.allclose(a, b, rtol=1e-13, atol=0)
