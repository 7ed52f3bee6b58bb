"""Per-slice masks, the host side: the argument check of the batched entry points, the ``mask_var`` key of the step-13 driver and the mask
cutting of ``pocs_cube_sharded``.  No GPU: the device call is replaced by a recorder."""
import numpy as np
import pytest
import yaml

from pseudo_3d_interpolation_amd import cube_POCS_interpolation_3D as step13
from pseudo_3d_interpolation_amd import sharding
from pseudo_3d_interpolation_amd.cube_io import Cube, open_cube, save_cube
from pseudo_3d_interpolation_amd.functions import POCS as P

N, NIL, NXL = 4, 6, 5


def _check(cube, mask):
    return P._check_cube_args(cube, mask, "FFT", "hard", "regular", 5, 0.0, 0.99, 1.0, 1e-3)


def test_check_cube_args_takes_one_mask_per_slice():
    cube = np.ones((N, NIL, NXL), np.complex64)
    mask = (np.arange(N * NIL * NXL).reshape(N, NIL, NXL) % 3 != 0).astype(np.uint8)
    out = _check(cube, mask)
    assert out[1].shape == (N, NIL, NXL) and np.array_equal(out[1], mask)
    assert _check(cube, mask[0])[1].shape == (NIL, NXL)          # the shared mask, as before
    weights = mask * 0.5                                          # (a 3-D mask may be non-binary like a 2-D one)
    assert np.array_equal(_check(cube, weights)[1], weights)


@pytest.mark.parametrize("shape", [(N + 1, NIL, NXL), (1, NIL, NXL), (NIL, NXL, 1)])
def test_check_cube_args_refuses_other_shapes_with_the_message_of_the_shared_mask(shape):
    cube = np.ones((N, NIL, NXL), np.complex64)
    with pytest.raises(ValueError) as e:
        _check(cube, np.ones(shape, np.uint8))
    assert str(e.value) == f"mask shape {shape} does not match slice shape {(NIL, NXL)}"


def test_check_cube_args_looks_at_the_whole_per_slice_mask():
    cube = np.ones((N, NIL, NXL), np.complex64)
    mask = np.ones((N, NIL, NXL), np.uint8)
    mask[N - 1, NIL - 1, NXL - 1] = 2
    with pytest.raises(ValueError, match="mask should be quasi-boolean .* maximum of 2"):
        _check(cube, mask)


# ---- step-13 driver ------------------------------------------------------------------------------------------------------------------------
NT = 7


def _time_cube(tmp_path, extra_vars, extra_dims):
    """A time-domain cube whose data variable has `twt` LAST (the driver moves it first) and fold 0 / 1 / 2."""
    rng = np.random.default_rng(3)
    data = rng.standard_normal((NIL, NXL, NT)).astype(np.float32)
    fold = rng.integers(0, 3, (NIL, NXL)).astype(np.uint8)
    dv = {'env': data, 'fold': fold}
    dims = {'env': ('iline', 'xline', 'twt'), 'fold': ('iline', 'xline')}
    dv.update(extra_vars)
    dims.update(extra_dims)
    cube = Cube(dv, dims, {'twt': 0.25 * np.arange(NT), 'iline': np.arange(NIL), 'xline': np.arange(NXL)},
                {'long_name': 'test cube', 'description': 'synthetic', 'history': 'made;', 'text': ''}, {}, {})
    return save_cube(cube, str(tmp_path / 'cube_twt.npz')), data, fold


def _run_driver(tmp_path, monkeypatch, path, mask_var=None):
    calls = []

    def fake_pocs_cube(cube, mask, out=None, **kw):
        calls.append((np.array(cube), np.array(mask), kw))
        out[...] = 0
        if kw.get('results') is not None:
            kw['results'].extend({'niterations': 1, 'runtime': 0.0, 'cost': 0.0, 'costs': [0.0]} for _ in range(cube.shape[0]))
        return out

    monkeypatch.setattr(step13, 'pocs_cube', fake_pocs_cube)
    meta = dict(transform_kind='fft', niter=3, eps=0, thresh_op='hard', thresh_model='exponential', decay_kind='values', p_max=0.99, p_min=0.01, alpha=1.0,
                sqrt_decay=False, version='regular', verbose=False)
    cfg = {'dim': 'twt', 'var': 'env', 'batch_chunk': 3, 'output_runtime_results': False, 'metadata': meta}
    if mask_var is not None:
        cfg['mask_var'] = mask_var
    yml = tmp_path / 'pocs.yml'
    yml.write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / 'out'
    step13.main(['13_cube_interpolate_POCS', path, '--path_pocs_parameter', str(yml), '--path_output_dir', str(out_dir)])
    return calls, out_dir


def test_driver_without_mask_var_calls_as_before(tmp_path, monkeypatch):
    path, data, fold = _time_cube(tmp_path, {}, {})
    calls, out_dir = _run_driver(tmp_path, monkeypatch, path)
    assert len(calls) == 1
    cube, mask, kw = calls[0]
    assert np.array_equal(cube, np.moveaxis(data, 2, 0))
    assert mask.shape == (NIL, NXL) and np.array_equal(mask, np.where(fold <= 1, fold, 1))
    assert 'mask_var' not in kw
    assert 'mask_var' not in open_cube(f'{out_dir}.npz').attrs


def test_driver_mask_var_with_the_dims_of_fold_gives_a_shared_mask(tmp_path, monkeypatch):
    live = (np.arange(NIL * NXL).reshape(NIL, NXL) % 4).astype(np.uint8)      # 0, 1 and larger: the fold rule clips at 1
    path, data, fold = _time_cube(tmp_path, {'live': live}, {'live': ('iline', 'xline')})
    calls, out_dir = _run_driver(tmp_path, monkeypatch, path, mask_var='live')
    cube, mask, kw = calls[0]
    assert mask.shape == (NIL, NXL) and np.array_equal(mask, np.where(live <= 1, live, 1)) and not np.array_equal(mask, np.where(fold <= 1, fold, 1))
    merged = open_cube(f'{out_dir}.npz')
    assert merged.attrs['mask_var'] == 'live'
    assert 'live' not in merged.data_vars                         # the mask variable is not written out
    import glob
    batch_files = sorted(glob.glob(str(out_dir / '*.npz')))
    assert batch_files and all('live' not in open_cube(f).data_vars for f in batch_files)


def test_driver_mask_var_with_the_dims_of_the_data_gives_one_mask_per_slice(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    live = rng.integers(0, 3, (NIL, NXL, NT)).astype(np.uint8)               # dims of the data variable: `twt` last
    path, data, fold = _time_cube(tmp_path, {'live': live}, {'live': ('iline', 'xline', 'twt')})
    calls, out_dir = _run_driver(tmp_path, monkeypatch, path, mask_var='live')
    assert len(calls) == 1
    cube, mask, kw = calls[0]
    want = np.moveaxis(np.where(live <= 1, live, 1), 2, 0)
    assert cube.shape == (NT, NIL, NXL) and mask.shape == (NT, NIL, NXL)
    assert np.array_equal(mask, want)                             # moved like the data: slice s of the mask belongs to slice s of the cube
    assert open_cube(f'{out_dir}.npz').attrs['mask_var'] == 'live'


def test_driver_hands_every_group_its_own_part_of_the_mask(tmp_path, monkeypatch):
    rng = np.random.default_rng(6)
    live = rng.integers(0, 2, (NIL, NXL, NT)).astype(np.uint8)
    path, data, fold = _time_cube(tmp_path, {'live': live}, {'live': ('iline', 'xline', 'twt')})
    monkeypatch.setenv('P3D_CLI_GROUP_GIB', '0')                  # one batch (3 slices) per call
    calls, _ = _run_driver(tmp_path, monkeypatch, path, mask_var='live')
    want = np.moveaxis(live, 2, 0)
    assert [c[0].shape[0] for c in calls] == [3, 3, 1]
    lo = 0
    for cube, mask, _ in calls:
        assert np.array_equal(mask, want[lo:lo + cube.shape[0]])
        lo += cube.shape[0]


def test_driver_mask_var_with_other_dims_is_refused(tmp_path, monkeypatch):
    path, data, fold = _time_cube(tmp_path, {'live': np.ones((NXL, NIL), np.uint8)}, {'live': ('xline', 'iline')})
    with pytest.raises(ValueError) as e:
        _run_driver(tmp_path, monkeypatch, path, mask_var='live')
    msg = str(e.value)
    assert "('xline', 'iline')" in msg and "('iline', 'xline')" in msg and "('iline', 'xline', 'twt')" in msg


# ---- sharding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [0, 1, 2])
def test_sharded_entry_cuts_a_per_slice_mask_like_the_cube(monkeypatch, rank):
    import torch.distributed as dist
    world, n = 3, 7
    monkeypatch.setattr(dist, 'get_rank', lambda group=None: rank)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: world)
    monkeypatch.setattr(dist, 'get_backend', lambda group=None: 'gloo')
    monkeypatch.setattr(dist, 'barrier', lambda group=None: None)
    rng = np.random.default_rng(7)
    cube = rng.standard_normal((n, NIL, NXL)).astype(np.float32)
    mask = rng.integers(0, 2, (n, NIL, NXL)).astype(np.uint8)
    lo, hi = sharding.slice_block(n, world, rank)
    seen = []

    def compute(block, m, **kw):
        seen.append((np.array(block), np.array(m)))
        return block * m

    own = sharding.pocs_cube_sharded(cube, mask, compute=compute, gather='none', niter=3)
    assert len(seen) == 1 and np.array_equal(seen[0][0], cube[lo:hi]) and np.array_equal(seen[0][1], mask[lo:hi])
    assert np.array_equal(own, cube[lo:hi] * mask[lo:hi])
    seen.clear()
    sharding.pocs_cube_sharded(cube, mask[0], compute=compute, gather='none', niter=3)     # a shared mask goes to every rank as it is
    assert seen[0][1].shape == (NIL, NXL) and np.array_equal(seen[0][1], mask[0])
    with pytest.raises(ValueError, match="does not match slice shape"):
        sharding.pocs_cube_sharded(cube, mask[:-1], compute=compute, gather='none', niter=3)
