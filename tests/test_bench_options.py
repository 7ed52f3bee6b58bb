"""bench.py without a GPU: what a plain run leaves out, and the sample --dump-outputs writes (on a host stand-in for a device cube)."""
import os
import sys

import numpy as np

import bench


class HostArray:
    """The shape / dtype / download interface of _ffi.DeviceArray over a NumPy array."""

    def __init__(self, a):
        self.a, self.shape, self.dtype = a, a.shape, a.dtype

    def download(self, first=0, count=None, out=None):
        count = self.shape[0] - first if count is None else count
        return self.a[first:first + count].copy()


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.repeats == 0 and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_profile and a.no_dense and a.only_main and a.no_end_to_end
    f = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert f.full and f.dump_outputs == "d"
    assert not (f.no_cpu_baseline or f.no_profile or f.no_dense or f.only_main or f.no_end_to_end)


def test_dump_is_a_fixed_float_sample(tmp_path):
    rng = np.random.default_rng(0)
    cube = (rng.standard_normal((40, 64, 48)) + 1j * rng.standard_normal((40, 64, 48))).astype(np.complex64)
    done = np.full(40, 5, np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), HostArray(cube), done)
    res = np.load(tmp_path / "a" / "result.npy")
    assert res.dtype == np.float32 and res.shape == (40, 64, 48, 2)          # small enough: every slice
    assert np.array_equal(res[..., 0] + 1j * res[..., 1], cube)
    assert np.array_equal(res, np.load(tmp_path / "b" / "result.npy"))
    it = np.load(tmp_path / "a" / "iterations_done.npy")
    assert it.dtype == np.float64 and np.array_equal(it, done)


def test_dump_of_a_large_cube_stays_under_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 6 * 32 * 40 * 4)                    # room for six float32 slices of 32 x 40
    cube = np.arange(20 * 32 * 40, dtype=np.float32).reshape(20, 32, 40)
    bench.dump_outputs(str(tmp_path), HostArray(cube), np.zeros(20))
    res = np.load(tmp_path / "result.npy")
    assert res.dtype == np.float32 and res.shape == (6, 32, 40) and res.nbytes <= bench.DUMP_BYTES
    picked = res[:, 0, 0].astype(np.int64) // (32 * 40)
    assert np.all(np.diff(picked) > 0) and np.array_equal(res, cube[picked])
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 40 * 8)                         # less than one complex slice: rows are sampled too
    big = (cube + 1j).astype(np.complex64)
    bench.dump_outputs(str(tmp_path), HostArray(big), np.zeros(20))
    res = np.load(tmp_path / "result.npy")
    assert res.dtype == np.float32 and res.shape == (1, 10, 40, 2) and res.nbytes <= bench.DUMP_BYTES
    assert os.path.isfile(tmp_path / "iterations_done.npy")
