"""The device selection all HIP units share (p3d::use_device, csrc/p3d_host.hpp): one entry point of each unit, called with a device that
does not exist and otherwise valid, tiny arguments, reports P3D_ERR_INVALID and 'device 99 out of range (N visible)' before any kernel runs;
a valid call afterwards works."""
import numpy as np
import pytest

from conftest import rel_l2
from helpers import agc_numpy
from pseudo_3d_interpolation_amd import _ffi

pytestmark = pytest.mark.gpu

BAD = 99
SLICE = np.arange(64, dtype=np.float32).reshape(1, 8, 8) + 1.0           # one 8 x 8 slice
SECTION = (np.arange(64, dtype=np.float32).reshape(4, 16) % 7.0) + 1.0   # 4 traces of 16 samples
LINES = np.array([[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]], np.float64)   # two lines of 3 vertices
LINE_OFF = np.array([0, 3, 6], np.int64)


def _bin_stack(device):
    # one bin, one trace of 16 samples
    return _ffi.bin_stack(SECTION[0], [0], [16], [0], [0, 1], 1, 1, 16, device=device)


CALLS = {
    "agc": lambda d: _ffi.agc(SECTION.T, 3, "mean", device=d),
    "smooth_slices": lambda d: _ffi.smooth_slices(SLICE, "median", size=3, device=d),
    "upsample_slices": lambda d: _ffi.upsample_slices(SLICE, np.arange(8), np.zeros(8), np.arange(8), np.zeros(8), device=d),
    "bin_stack": _bin_stack,
    "despike_detect": lambda d: _ffi.despike_detect(SECTION, 3, "mean", 2.0, 16, device=d),
    "static_shift": lambda d: _ffi.static_shift(SECTION, np.zeros(4, np.int32), device=d),
    "mistie_nearest": lambda d: _ffi.mistie_nearest(LINES, LINE_OFF, [[1.0, 0.5]], [[0, 1]], device=d),
    "trace_ops": lambda d: _ffi.trace_ops(SECTION.T, [("reduce", 0)], device=d),
    "DeviceArray": lambda d: _ffi.DeviceArray((4,), np.float32, device=d),
    "time2freq": lambda d: _ffi.time2freq(SECTION.T, 0.004, device=d),
    "Plan": lambda d: _ffi.Plan(8, 8, 1, device=d),
    "Plan64": lambda d: _ffi.Plan64(8, 8, 1, device=d),
    "WaveletPlan": lambda d: _ffi.WaveletPlan(8, 8, 1, wavelet="db2", device=d),
    "WaveletPlan64": lambda d: _ffi.WaveletPlan64(8, 8, 1, wavelet="db2", device=d),
}


def _expect_out_of_range(call):
    with pytest.raises(_ffi.P3DError) as exc:
        call(BAD)
    print(f"code {exc.value.code}: {exc.value}")
    assert exc.value.code == _ffi.P3D_ERR_INVALID
    assert f"device {BAD} out of range ({_ffi.device_count()} visible)" in str(exc.value)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_device_that_does_not_exist_is_refused(name):
    """('trace_ops' asks p3d_dev_mem_info and p3d_dev_malloc for the device before it reaches the step-11 unit: they select it the same way;
    test_preproc_entry_point_refuses_the_device calls that unit directly.)"""
    _expect_out_of_range(CALLS[name])


def test_preproc_entry_point_refuses_the_device():
    """p3d_pre_reduce_dev, the first call trace_ops makes into p3d_preproc.hip (the pointers are never read: the device check comes first)."""
    ref = np.empty(4, np.float32)
    _expect_out_of_range(lambda d: _ffi.check(_ffi.lib().p3d_pre_reduce_dev(d, _ffi._ptr(SECTION), 16, 4, 0, _ffi._ptr(ref))))


def test_a_refused_device_leaves_no_state_behind():
    x = np.ascontiguousarray(SECTION.T)
    with pytest.raises(_ffi.P3DError):
        _ffi.agc(x, 3, "mean", device=BAD)
    got = _ffi.agc(x, 3, "mean", device=0)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert rel_l2(got, agc_numpy.agc(x, 3, "mean", axis=0)) <= 1e-5
