"""ctypes binding of include/p3d.h (libp3d_hip.so).  No fallback: if the library is missing or no
GPU is visible, every compute entry point raises."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P3D_LIB_PATH") or os.path.join(_HERE, "libp3d_hip.so")  # env override: experiments only

P3D_OK = 0
P3D_ERR_INVALID, P3D_ERR_UNSUPPORTED, P3D_ERR_HIP = -1, -2, -3
P3D_C64, P3D_F32 = 0, 1
P3D_C128, P3D_F64 = 2, 3      # the double-precision entry points only (Plan64)
P3D_OP = {"hard": 0, "soft": 1, "garrote": 2, "garotte": 2}
P3D_OP_PERCENTILE = 16
P3D_OP.update({f"{k}-percentile": v | P3D_OP_PERCENTILE for k, v in list(P3D_OP.items())})
P3D_VER = {"regular": 0, "fast": 1, "adaptive": 2}
P3D_FLAG_PROFILE = 1
P3D_FLAG_PRIMED = 2
P3D_FLAG_MASK_PER_SLICE = 4
STATS_PER_SLICE = 6
P3D_DCT_NORM = {None: 0, "backward": 0, "ortho": 1}   # P3D_DCT_BACKWARD / P3D_DCT_ORTHO: the `norm` of scipy.fft.dctn / idctn


class P3DError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libp3d_hip error {code}: {msg}")
        self.code = code


class UnsupportedError(P3DError, NotImplementedError):
    pass


class PocsParams(C.Structure):
    _fields_ = [("niter", C.c_int32), ("thresh_op", C.c_int32), ("version", C.c_int32), ("flags", C.c_int32),
                ("eps", C.c_double), ("alpha", C.c_double)]


_lib = None

# name -> (restype, argtypes); kept in one table so tests can check it against include/p3d.h
PROTOTYPES = {
    "p3d_abi_version": (C.c_int, []),
    "p3d_last_error": (C.c_char_p, []),
    "p3d_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "p3d_device_cus": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "p3d_shape_supported": (C.c_int, [C.c_int, C.c_int]),
    "p3d_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "p3d_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_malloc": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "p3d_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "p3d_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "p3d_host_free": (C.c_int, [C.c_void_p]),
    "p3d_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "p3d_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "p3d_fft2_c64_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_fft2_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_fft2_shrink_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "p3d_pocs_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_runtime_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "p3d_plan64_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "p3d_plan64_destroy": (C.c_int, [C.c_void_p]),
    "p3d_pocs64_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_fft2_c128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_pocs64_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_pocs64_percentile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_pocs64_sorted_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_pocs64_data_driven_pick": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_dct2_c128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "p3d_pocs64_dct_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "p3d_pocs64_dct_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "p3d_dev_malloc": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_size_t]),
    "p3d_dev_free": (C.c_int, [C.c_void_p]),
    "p3d_dev_memcpy": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "p3d_dev_memset": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t]),
    "p3d_dev_synchronize": (C.c_int, [C.c_int]),
    "p3d_dev_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "p3d_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "p3d_host_unregister": (C.c_int, [C.c_void_p]),
    "p3d_pocs_prime_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_pocs_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_pocs_sorted_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_pocs_data_driven_pick": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_pocs_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double)]),
    "p3d_dct2_c64_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "p3d_dct2_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "p3d_dct_shrink_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "p3d_pocs_dct_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "p3d_pocs_dct_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "p3d_pocs_dct_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double), C.c_int]),
    "p3d_pocs_dct_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_double), C.c_int]),
    "p3d_pocs_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_double)]),
    "p3d_patch_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int]),
    "p3d_patch_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_patch_plan_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "p3d_patch_gather_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_patch_mask_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "p3d_patch_route": (C.c_int, [C.c_void_p, C.POINTER(PocsParams), C.POINTER(C.c_int)]),
    "p3d_patch_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_patch_dct_route": (C.c_int, [C.c_void_p, C.POINTER(PocsParams), C.c_int, C.POINTER(C.c_int)]),
    "p3d_patch_dct_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_patch_blend_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_multi_stats": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_multi_run": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(PocsParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_time2freq": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p]),
    "p3d_freq2time": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int,
                                C.c_void_p]),
    "p3d_time2freq_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "p3d_freq2time_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int,
                                    C.c_void_p]),
    "p3d_last_sparsity": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_smooth_gaussian": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "p3d_smooth_median": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "p3d_agc": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_agc_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_pre_reduce_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]),
    "p3d_pre_balance_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_pre_gain_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_pre_sosfiltfilt_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "p3d_pre_upfirdn_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                      C.c_size_t, C.c_void_p]),
    "p3d_pre_spectral_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                       C.c_double, C.c_void_p, C.c_void_p]),
    "p3d_upsample": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_bin_stack": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p]),
    "p3d_bin_stack_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p]),
    "p3d_despike_detect": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    "p3d_despike_detect_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "p3d_despike_replace": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    "p3d_despike_replace_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_float]),
    "p3d_static_scan_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_static_stalta_max_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "p3d_static_stalta_cross_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                              C.c_void_p]),
    "p3d_static_peak_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_static_shift_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_static_detect": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p,
                                    C.c_void_p]),
    "p3d_static_peak": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_static_shift": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_mistie_cross_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "p3d_mistie_nearest_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "p3d_mistie_xcorr_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_mistie_cross": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "p3d_mistie_nearest": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "p3d_mistie_xcorr": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "p3d_delrt_pad_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_delrt_pad": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_delrt_windows_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_delrt_windows": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_proj_tmerc_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_proj_tmerc": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_proj_smooth_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_tide_predict_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_tide_predict": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_segy_encode_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_segy_encode": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_segy_decode_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_segy_decode": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "p3d_merge_keys_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_merge_keys": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_merge_records_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_merge_records": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "p3d_last_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int)]),
    "p3d_wavelet_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_wavelet_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_wavelet_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_void_p]),
    "p3d_wavedec2_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_waverec2_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_wavelet_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_wavelet_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams),
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_wavelet64_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_wavelet64_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_wavelet64_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "p3d_wavelet64_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_wavelet64_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams),
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_shearlet_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "p3d_shearlet64_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "p3d_shearlet64_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_shearlet64_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "p3d_shearlet64_fused_shape": (C.c_int, [C.c_int, C.c_int]),
    "p3d_shearlet64_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_shearlet64_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams),
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_shearlet_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_shearlet_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "p3d_shearlet_transform_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_shearlet_inverse_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_shearlet_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_shearlet_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PocsParams),
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "p3d_vol_shape_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "p3d_vol_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "p3d_vol_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_vol_fft3_c64_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_vol_fft3_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_vol_shrink_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol_last_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "p3d_vol_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_double)]),
    "p3d_vol_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(C.c_double)]),
    "p3d_vol64_shape_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "p3d_vol64_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "p3d_vol64_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_vol64_fft3_c128_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_vol64_fft3_c128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "p3d_vol64_shrink_c128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol64_last_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "p3d_vol64_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol64_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "p3d_vol64_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_double)]),
    "p3d_vol64_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_double)]),
    "p3d_voldct_shape_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "p3d_voldct_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "p3d_voldct_plan_destroy": (C.c_int, [C.c_void_p]),
    "p3d_voldct_dct3_c64_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_voldct_dct3_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "p3d_voldct_shrink_c64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_voldct_last_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "p3d_voldct_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_voldct_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "p3d_voldct_run_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_double)]),
    "p3d_voldct_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PocsParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_double)]),
}


def _preload_torch_hip():
    """PyTorch-ROCm wheels bring their own HIP runtime (same SONAME as /opt/rocm's).  The library is built against the SYSTEM runtime and, by
    default, runs on it: nothing is preloaded.  A process that ALSO uses ``torch.cuda`` must let torch go first -- once this library's
    runtime has initialised, a later ``torch.cuda`` call finds no device ("No HIP GPUs are available", measured on the MI355X boxes), the
    other order works: ``import torch`` before the first call into this package (``sharding.py`` and ``bench.py --gpus N>1`` do), or set
    ``P3D_TORCH_HIP_PRELOAD=1`` to have torch's runtime library dlopen'ed ahead of ours without importing torch.  In both cases the
    library then runs on torch's runtime; `_check_runtime` records the pair of versions and warns when they differ."""
    if not os.environ.get("P3D_TORCH_HIP_PRELOAD") or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
        if path and os.path.isfile(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (ImportError, OSError, ValueError):
        pass


def lib():
    """Load libp3d_hip.so once.  Raises ``ImportError`` if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        _preload_torch_hip()
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
        _check_runtime(handle)
    return _lib


_runtime = None


def _check_runtime(handle):
    """Which HIP runtime did the process bind?  libp3d_hip.so is built against /opt/rocm; when a PyTorch wheel's copy of libamdhip64 (same
    SONAME) is mapped first -- `_preload_torch_hip` does that on purpose, see there -- the library runs on THAT runtime.  Record both
    versions and the file, and warn when major.minor differ (an unchecked ABI / code-object skew otherwise)."""
    global _runtime
    comp, run = C.c_int(0), C.c_int(0)
    path = None
    try:
        if handle.p3d_runtime_info(C.byref(comp), C.byref(run)) != P3D_OK:
            return
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
    except OSError:
        pass

    def split(v):
        return v // 10000000, (v // 100000) % 100, v % 100000
    _runtime = {"compiled_hip_version": "%d.%d.%d" % split(comp.value), "runtime_hip_version": "%d.%d.%d" % split(run.value), "runtime_library": path}
    if split(comp.value)[:2] != split(run.value)[:2]:
        import warnings
        warnings.warn(f"libp3d_hip.so was compiled against HIP {_runtime['compiled_hip_version']} but the process runs HIP "
                      f"{_runtime['runtime_hip_version']} ({path}): another copy of the runtime was mapped first (PyTorch imported before this package, or "
                      f"P3D_TORCH_HIP_PRELOAD=1); processes that do not need torch.cuda should load this package first", RuntimeWarning, stacklevel=3)


def runtime_info():
    """{'compiled_hip_version', 'runtime_hip_version', 'runtime_library'} of the loaded library (bench.py records it)."""
    lib()
    return dict(_runtime or {})


def check(code):
    if code != P3D_OK:
        msg = lib().p3d_last_error().decode("utf-8", "replace")
        raise (UnsupportedError if code == P3D_ERR_UNSUPPORTED else P3DError)(code, msg)


def device_count():
    n = C.c_int(0)
    check(lib().p3d_device_count(C.byref(n)))
    return n.value


def device_cus(device=0):
    """Compute units of a device (the persistent row and column passes size their grids by it)."""
    n = C.c_int(0)
    check(lib().p3d_device_cus(int(device), C.byref(n)))
    return n.value


def shape_supported(nil, nxl):
    return bool(lib().p3d_shape_supported(int(nil), int(nxl)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceBuffer:
    """A hipMalloc'ed buffer owned through a plan (for callers that keep cubes resident in HBM)."""

    def __init__(self, plan, nbytes):
        self.plan, self.nbytes = plan, int(nbytes)
        p = C.c_void_p()
        check(lib().p3d_malloc(plan.handle, C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().p3d_memcpy_h2d(self.plan.handle, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().p3d_memcpy_d2h(self.plan.handle, _ptr(out), self.ptr, out.nbytes))
        return out

    def download_into(self, arr):
        """Copy the first ``arr.nbytes`` bytes into a C-contiguous host array (e.g. a slab of the result cube)."""
        if not arr.flags.c_contiguous or arr.nbytes > self.nbytes:
            raise ValueError("destination must be C-contiguous and no larger than the buffer")
        check(lib().p3d_memcpy_d2h(self.plan.handle, _ptr(arr), self.ptr, arr.nbytes))
        return arr

    def free(self):
        if self.ptr:
            check(lib().p3d_free(self.plan.handle, self.ptr))
            self.ptr = None


def _tau_table(tau, shape):
    """Thresholds broadcast to ``shape`` -> float64 ``shape + (2,)`` of (Re, Im) pairs: the layout every C entry takes."""
    tau = np.broadcast_to(np.asarray(tau), shape)
    t = np.empty(tau.shape + (2,), np.float64)
    t[..., 0] = tau.real
    t[..., 1] = tau.imag if np.iscomplexobj(tau) else 0.0
    return t


def _filter_bank(wavelet):
    """A wavelet name or (dec_lo, dec_hi, rec_lo, rec_hi) -> the four float64 filters of equal length."""
    bank = wavelet if isinstance(wavelet, (tuple, list)) else wavelet_filters(wavelet)
    bank = [np.ascontiguousarray(b, dtype=np.float64) for b in bank]
    if len(bank) != 4 or len({b.size for b in bank}) != 1:
        raise ValueError("a filter bank is (dec_lo, dec_hi, rec_lo, rec_hi) of equal length")
    return bank


def _real_psi(psi):
    """Shearlet spectra (nil, nxl, nsh), real."""
    psi = np.asarray(psi)
    if psi.ndim != 3:
        raise ValueError(f"Psi must be (nil, nxl, nshearlets), got shape {psi.shape}")
    if np.iscomplexobj(psi):
        raise NotImplementedError("complex shearlet spectra (realCoefficients=False) are not implemented")
    return psi


class _PlanBase:
    """What the six plan classes share: the life of the C handle (``_DESTROY``) and the marshalling of one POCS job for the entry ``_RUN``
    (thresholds per slice and iteration: ``_tau_shape()``).  This one holds the float32 side: complex64 / float32 cubes, a float32 mask."""
    _DESTROY = _RUN = None
    _MASK_DT = np.float32

    def close(self):
        if getattr(self, "handle", None):
            getattr(lib(), self._DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        if lib is not None:   # (module globals are gone while the interpreter shuts down: the process's device memory goes with it)
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _cube(self, x):
        x = np.asarray(x)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (self.nil, self.nxl):
            raise ValueError(f"expected (nslices, {self.nil}, {self.nxl}), got {x.shape}")
        if x.shape[0] > self.max_slices:
            raise ValueError(f"{x.shape[0]} slices > max_slices {self.max_slices}")
        if np.iscomplexobj(x):
            return np.ascontiguousarray(x, dtype=np.complex64), P3D_C64
        return np.ascontiguousarray(x, dtype=np.float32), P3D_F32

    def _tau_shape(self):
        return ()

    def _host_job(self, x, mask):
        """The host cube as the library takes it, its dtype code, the mask in the plan's precision -- (nil, nxl), shared by the batch, or
        (nslices, nil, nxl), one mask per slice (P3D_FLAG_MASK_PER_SLICE) -- and an empty result."""
        xc, dt = self._cube(x)
        m = np.ascontiguousarray(mask, dtype=self._MASK_DT)
        if m.shape != (self.nil, self.nxl) and m.shape != xc.shape:
            raise ValueError(f"mask shape {m.shape} != {(self.nil, self.nxl)}")
        return xc, dt, m, np.empty_like(xc)

    def _run_entry(self, entry, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, n, thresh_op, version, eps, alpha, active, profile=False, want_sums=True,
                   primed=False, extra=(), mask_per_slice=False):
        """One call of a p3d_*_run entry on raw pointers (``extra``: what the entry takes behind the common arguments).  Returns (niter_done, sums or
        None, device ms of the loop)."""
        t = _tau_table(tau, (n, niter) + self._tau_shape())
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        prm = Plan._params(niter, thresh_op, version, eps, alpha, profile, primed, mask_per_slice)
        done = np.zeros(n, np.int32)
        sums = np.zeros((niter + 1, n), np.float64) if want_sums else None
        ms = C.c_double(0.0)
        check(getattr(lib(), entry)(self.handle, x_ptr, dtype, mask_ptr, _ptr(t), None if act is None else _ptr(act), C.byref(prm), out_ptr, n,
                                    _ptr(done), None if sums is None else _ptr(sums), C.byref(ms), *extra))
        return done, sums, ms.value

    def stats(self, x):
        """`stats_dev` of a host cube."""
        xc, dt = self._cube(x)
        return self.stats_dev(xc.ctypes.data, dt, xc.shape[0])

    def run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None):
        """Host arrays in, host array out (as `_cube` converts ``x``).  tau: anything that broadcasts to (nslices, niter) + the plan's thresholds per
        iteration, real or complex.  Returns (out, niter_done, sums, elapsed_ms)."""
        xc, dt, m, out = self._host_job(x, mask)
        done, sums, ms = self.run_dev(xc.ctypes.data, dt, m.ctypes.data, tau, niter, out.ctypes.data, xc.shape[0], thresh_op=thresh_op, version=version,
                                      eps=eps, alpha=alpha, active=active, mask_per_slice=m.ndim == 3)
        return out, done, sums, ms

    def run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, n, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None,
                mask_per_slice=False):
        """`run` on raw pointers (host or device; the mask in the plan's precision, [nil][nxl], or [n][nil][nxl] with ``mask_per_slice``).  Returns
        (niter_done, sums, device ms of the loop)."""
        return self._run_entry(self._RUN, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, n, thresh_op, version, eps, alpha, active,
                               mask_per_slice=mask_per_slice)


class _PlanBase64(_PlanBase):
    """... and the double-precision side: cubes of all four types as they are, a float64 mask."""
    _DT = {np.dtype(np.complex128): P3D_C128, np.dtype(np.float64): P3D_F64, np.dtype(np.complex64): P3D_C64, np.dtype(np.float32): P3D_F32}
    _MASK_DT = np.float64

    def _cube(self, x):
        x = np.asarray(x)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (self.nil, self.nxl) or x.shape[0] > self.max_slices:
            raise ValueError(f"expected (<= {self.max_slices}, {self.nil}, {self.nxl}), got {x.shape}")
        if x.dtype not in self._DT:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        return np.ascontiguousarray(x), self._DT[x.dtype]


class WaveletPlan64(_PlanBase64):
    """p3d_wplan64 wrapper: the WAVELET POCS loop in double precision (include/p3d.h) for complex128 / float64 cubes, and for complex64 /
    float32 cubes on request (``precision='reference'``).  tau: (nslices, niter, nlev, 3), levels coarse -> fine."""
    _DESTROY, _RUN = "p3d_wavelet64_plan_destroy", "p3d_wavelet64_run"

    def __init__(self, nil, nxl, max_slices, wavelet="coif5", level=None, device=0):
        self.nil, self.nxl, self.max_slices, self.device = int(nil), int(nxl), int(max_slices), int(device)
        self.wavelet = wavelet
        bank = _filter_bank(wavelet)
        h = C.c_void_p()
        check(lib().p3d_wavelet64_plan_create(C.byref(h), self.device, self.nil, self.nxl, self.max_slices, *map(_ptr, bank),
                                              bank[0].size, -1 if level is None else int(level)))
        self.handle = h
        nlev, ncoef = C.c_int(0), C.c_int64(0)
        check(lib().p3d_wavelet64_info(self.handle, C.byref(nlev), C.byref(ncoef)))
        self.nlev, self.ncoef = nlev.value, ncoef.value

    def _tau_shape(self):
        return (self.nlev, 3)

    @staticmethod
    def _tau(tau, n, niter, nlev):
        return _tau_table(tau, (n, niter, nlev, 3))

    def stats_dev(self, x_ptr, dtype, n):
        """(nslices, nlev, 3, 4): Re / Im of the lexicographic max, max |d|, min |d| per detail array (coarsest level first), in double."""
        st = np.empty((n, self.nlev, 3, 4), np.float64)
        check(lib().p3d_wavelet64_stats(self.handle, x_ptr, dtype, n, _ptr(st)))
        return st


class DeviceArray:
    """A typed block of device memory that belongs to no plan (``p3d_dev_malloc``): cubes that stay resident in HBM across several plans
    and jobs, without any other GPU runtime in the process.  ``ptr`` is what the ``*_dev`` entry points take."""

    def __init__(self, shape, dtype, device=0):
        self.shape, self.dtype, self.device = tuple(int(n) for n in shape), np.dtype(dtype), int(device)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().p3d_dev_malloc(self.device, C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value

    def _span(self, first, count):
        per = self.nbytes // self.shape[0] if self.shape[0] else 0
        count = self.shape[0] - first if count is None else count
        if first < 0 or count < 0 or first + count > self.shape[0]:
            raise ValueError(f'rows {first}:{first + count} outside an array of {self.shape[0]}')
        return self.ptr + first * per, count * per, count

    def upload(self, host, first=0):
        """rows ``first ...`` <- ``host`` (C-contiguous, this dtype, trailing shape of the array)."""
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.shape[1:] != self.shape[1:]:
            raise ValueError(f'trailing shape {host.shape[1:]} does not match {self.shape[1:]}')
        dst, nbytes, _ = self._span(first, host.shape[0])
        check(lib().p3d_dev_memcpy(self.device, dst, _ptr(host), nbytes, 0))
        return self

    def download(self, first=0, count=None, out=None):
        src, nbytes, count = self._span(first, count)
        if out is None:
            out = np.empty((count,) + self.shape[1:], self.dtype)
        elif not out.flags.c_contiguous or out.nbytes != nbytes or out.dtype != self.dtype:
            raise ValueError('out must be C-contiguous with the dtype and size of the rows asked for')
        check(lib().p3d_dev_memcpy(self.device, _ptr(out), src, nbytes, 1))
        return out

    def copy_from(self, other):
        if other.nbytes != self.nbytes:
            raise ValueError('size mismatch')
        check(lib().p3d_dev_memcpy(self.device, self.ptr, other.ptr, self.nbytes, 2))
        return self

    def zero(self):
        check(lib().p3d_dev_memset(self.device, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr:
            check(lib().p3d_dev_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


def device_synchronize(device=0):
    check(lib().p3d_dev_synchronize(int(device)))


def device_mem_info(device=0):
    free, total = C.c_size_t(0), C.c_size_t(0)
    check(lib().p3d_dev_mem_info(int(device), C.byref(free), C.byref(total)))
    return free.value, total.value


def host_register(arr):
    """Page-lock a C-contiguous NumPy array in place (p3d_host_register).  True when it is registered now (and must be handed to
    :func:`host_unregister` later), False when the runtime refused -- the array is usable either way."""
    if not arr.flags.c_contiguous or arr.nbytes == 0:
        return False
    return lib().p3d_host_register(_ptr(arr), arr.nbytes) == P3D_OK


def host_unregister(arr):
    check(lib().p3d_host_unregister(_ptr(arr)))


def host_register_range(addr, nbytes):
    """Page-lock ``nbytes`` of host memory from address ``addr`` (the caller keeps the memory alive); True when registered."""
    return nbytes > 0 and lib().p3d_host_register(C.c_void_p(addr), nbytes) == P3D_OK


def host_unregister_range(addr):
    check(lib().p3d_host_unregister(C.c_void_p(addr)))


class PinnedBuffer:
    """Page-locked host memory (p3d_host_alloc) viewed as NumPy arrays: the staging area of the chunk pipeline."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().p3d_host_alloc(C.byref(p), self.nbytes))
        self.ptr = p.value
        self._raw = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def view(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if n > self.nbytes:
            raise ValueError("view larger than the buffer")
        return self._raw[:n].view(dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self._raw = None
            check(lib().p3d_host_free(self.ptr))
            self.ptr = None


class Plan(_PlanBase):
    """p3d_plan wrapper: one device, one (nil, nxl) slice shape, up to ``max_slices`` per call."""
    _DESTROY = "p3d_plan_destroy"

    def __init__(self, nil, nxl, max_slices, device=0):
        self.nil, self.nxl, self.max_slices, self.device = int(nil), int(nxl), int(max_slices), int(device)
        h = C.c_void_p()
        check(lib().p3d_plan_create(C.byref(h), self.device, self.nil, self.nxl, self.max_slices))
        self.handle = h

    # ---- helpers ---------------------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # ---- transforms ------------------------------------------------------------------------
    def fft2(self, x, inverse=False):
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        out = np.empty_like(xc)
        check(lib().p3d_fft2_c64(self.handle, _ptr(xc), _ptr(out), xc.shape[0], int(bool(inverse))))
        return out[0] if squeeze else out

    def fft2_dev(self, in_ptr, out_ptr, nslices, inverse=False):
        """fft2 / ifft2 (numpy conventions) of complex64 slices resident on the device; `out_ptr` may equal `in_ptr`."""
        check(lib().p3d_fft2_c64_dev(self.handle, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(nslices), int(bool(inverse))))

    def fft2_shrink(self, x, tau, thresh_op="hard"):
        """threshold(fft2(x), tau, kind) on the device; ``tau`` scalar or one value per slice."""
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        n = xc.shape[0]
        t = _tau_table(tau, (n,))
        out = np.empty_like(xc)
        check(lib().p3d_fft2_shrink_c64(self.handle, _ptr(xc), _ptr(t), P3D_OP[thresh_op], _ptr(out), n))
        return out[0] if squeeze else out

    # ---- POCS ------------------------------------------------------------------------------
    def stats(self, x):
        xc, dt = self._cube(x)
        st = np.empty((xc.shape[0], STATS_PER_SLICE), np.float64)
        check(lib().p3d_pocs_stats(self.handle, _ptr(xc), dt, xc.shape[0], _ptr(st)))
        return st

    def sorted_spectrum(self, x):
        """fft2 of every slice, sorted on the device in NumPy's complex order (kept in the plan); returns x_fwd.max() per slice
        (complex64) -- first half of the 'data-driven' schedule (POCS.py:356-362)."""
        xc = np.ascontiguousarray(x, dtype=np.complex64)
        if xc.ndim != 3 or xc.shape[1:] != (self.nil, self.nxl):
            raise ValueError(f"cube shape {xc.shape} != (n, {self.nil}, {self.nxl})")
        peaks = np.empty((xc.shape[0], 2), np.float32)
        check(lib().p3d_pocs_sorted_spectrum(self.handle, _ptr(xc), xc.shape[0], _ptr(peaks)))
        return peaks.view(np.complex64)[:, 0]

    def sorted_spectrum_dev(self, x_ptr, n):
        """`sorted_spectrum` of a complex64 batch resident on the device (raw pointer)."""
        peaks = np.empty((n, 2), np.float32)
        check(lib().p3d_pocs_sorted_spectrum(self.handle, C.c_void_p(x_ptr), n, _ptr(peaks)))
        return peaks.view(np.complex64)[:, 0]

    def data_driven_pick(self, tau_min, tau_max, niter):
        """Second half: per slice the number of coefficients strictly between the bounds (complex64, NumPy's order) and the
        niter thresholds picked from them (POCS.py:359-362); must follow sorted_spectrum directly."""
        lo = np.ascontiguousarray(tau_min, dtype=np.complex64)
        hi = np.ascontiguousarray(tau_max, dtype=np.complex64)
        n = lo.shape[0]
        bounds = np.empty((n, 4), np.float32)
        bounds[:, 0], bounds[:, 1], bounds[:, 2], bounds[:, 3] = lo.real, lo.imag, hi.real, hi.imag
        tau = np.empty((n, int(niter), 2), np.float32)
        count = np.empty((n,), np.int64)
        check(lib().p3d_pocs_data_driven_pick(self.handle, n, int(niter), _ptr(bounds), _ptr(tau), _ptr(count)))
        return tau.view(np.complex64)[..., 0], count

    def stats_dev(self, x_ptr, dtype, nslices):
        st = np.empty((nslices, STATS_PER_SLICE), np.float64)
        check(lib().p3d_pocs_stats_dev(self.handle, x_ptr, dtype, nslices, _ptr(st)))
        return st

    @staticmethod
    def _params(niter, thresh_op, version, eps, alpha, profile, primed=False, mask_per_slice=False):
        if thresh_op not in P3D_OP:
            raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"thresh_op {thresh_op!r} is not implemented by the HIP kernels")
        return PocsParams(int(niter), P3D_OP[thresh_op], P3D_VER[version],
                          (P3D_FLAG_PROFILE if profile else 0) | (P3D_FLAG_PRIMED if primed else 0) | (P3D_FLAG_MASK_PER_SLICE if mask_per_slice else 0),
                          float(eps), float(alpha))

    @staticmethod
    def _tau(tau, nslices, niter):
        return _tau_table(tau, (nslices, niter))

    def run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None,
            profile=False):
        """Host arrays in, host arrays out; ``mask`` (nil, nxl) or, one per slice, (nslices, nil, nxl).  Returns (out, niter_done, sums, elapsed_ms)."""
        xc, dt, m, out = self._host_job(x, mask)
        done, sums, ms = self._run_entry("p3d_pocs_run", _ptr(xc), dt, _ptr(m), tau, niter, _ptr(out), xc.shape[0], thresh_op, version, eps, alpha,
                                         active, profile, mask_per_slice=m.ndim == 3)
        return out, done, sums, ms

    def prime_dev(self, x_ptr, dtype, mask_ptr, nslices):
        """`stats_dev` that doubles as the first pass of the job: follow it with ``run_dev(..., primed=True)`` on the same
        pointers and batch (include/p3d.h, p3d_pocs_prime_dev).

        ``primed=True`` is a promise about the CONTENTS of the two device buffers: the plan can only check that pointers, dtype and
        batch are the ones it primed and that nothing else ran on it in between -- a caller that rewrites ``x`` or ``mask`` in
        place between the two calls must not pass the flag (the run would use the work buffer, compact samples and ``sum |x_obs|``
        of the old contents)."""
        st = np.empty((nslices, STATS_PER_SLICE), np.float64)
        check(lib().p3d_pocs_prime_dev(self.handle, x_ptr, dtype, mask_ptr, nslices, _ptr(st)))
        return st

    def run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, nslices, thresh_op="hard", version="regular",
                eps=0.0, alpha=1.0, active=None, profile=False, want_sums=True, primed=False, mask_per_slice=False):
        """Device pointers in/out (cube stays resident in HBM); ``mask_per_slice``: ``mask_ptr`` holds [nslices][nil][nxl] (the unfused passes; ``primed``
        is then ignored).  Returns (niter_done, sums -- None unless ``want_sums`` --, elapsed_ms)."""
        return self._run_entry("p3d_pocs_run_dev", x_ptr, dtype, mask_ptr, tau, niter, out_ptr, nslices, thresh_op, version, eps, alpha, active, profile,
                               want_sums, primed, mask_per_slice=mask_per_slice)

    # ---- transform_kind = 'DCT': scipy.fft.dctn / idctn (type 2) as the transform of the loop ------------
    @staticmethod
    def _dct_norm(norm):
        if norm not in P3D_DCT_NORM:
            raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"DCT norm {norm!r} is not implemented by the HIP kernels (None, 'backward', 'ortho')")
        return P3D_DCT_NORM[norm]

    def dct2(self, x, inverse=False, norm=None):
        """scipy.fft.dctn (``inverse``: idctn) of complex64 slices over the last two axes, type 2."""
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        out = np.empty_like(xc)
        check(lib().p3d_dct2_c64(self.handle, _ptr(xc), _ptr(out), xc.shape[0], int(bool(inverse)), self._dct_norm(norm)))
        return out[0] if squeeze else out

    def dct_shrink(self, x, tau, thresh_op="hard", norm=None):
        """threshold(dctn(x), tau, kind) on the device; ``tau`` scalar or one value per slice."""
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        n = xc.shape[0]
        t = _tau_table(tau, (n,))
        out = np.empty_like(xc)
        check(lib().p3d_dct_shrink_c64(self.handle, _ptr(xc), _ptr(t), P3D_OP[thresh_op], _ptr(out), n, self._dct_norm(norm)))
        return out[0] if squeeze else out

    def dct_stats(self, x, norm=None):
        xc, dt = self._cube(x)
        st = np.empty((xc.shape[0], STATS_PER_SLICE), np.float64)
        check(lib().p3d_pocs_dct_stats(self.handle, _ptr(xc), dt, xc.shape[0], _ptr(st), self._dct_norm(norm)))
        return st

    def dct_stats_dev(self, x_ptr, dtype, nslices, norm=None):
        st = np.empty((nslices, STATS_PER_SLICE), np.float64)
        check(lib().p3d_pocs_dct_stats_dev(self.handle, x_ptr, dtype, nslices, _ptr(st), self._dct_norm(norm)))
        return st

    def dct_run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None, norm=None):
        """`run` with the DCT pair as the transform.  Returns (out, niter_done, sums, elapsed_ms)."""
        xc, dt, m, out = self._host_job(x, mask)
        done, sums, ms = self._run_entry("p3d_pocs_dct_run", _ptr(xc), dt, _ptr(m), tau, niter, _ptr(out), xc.shape[0], thresh_op, version, eps, alpha,
                                         active, extra=(self._dct_norm(norm),), mask_per_slice=m.ndim == 3)
        return out, done, sums, ms

    def dct_run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, nslices, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None,
                    norm=None, want_sums=True, mask_per_slice=False):
        """`run_dev` with the DCT pair as the transform.  Returns (niter_done, sums, elapsed_ms)."""
        return self._run_entry("p3d_pocs_dct_run_dev", x_ptr, dtype, mask_ptr, tau, niter, out_ptr, nslices, thresh_op, version, eps, alpha, active,
                               want_sums=want_sums, extra=(self._dct_norm(norm),), mask_per_slice=mask_per_slice)

    def last_sparsity(self):
        """Fraction of 8-column spectrum blocks that kept a coefficient in the last run (-1: dense path)."""
        v = C.c_double(-1.0)
        check(lib().p3d_last_sparsity(self.handle, C.byref(v)))
        return v.value

    def last_profile(self):
        cm, rm, cn, rn = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        check(lib().p3d_last_profile(self.handle, C.byref(cm), C.byref(cn), C.byref(rm), C.byref(rn)))
        return {"colpass_ms": cm.value, "colpass_launches": cn.value, "rowpass_ms": rm.value,
                "rowpass_launches": rn.value}


class PatchPlan:
    """p3d_patch_plan wrapper: the windows of (nil, nxl) slices over a ``Plan`` of the window shape that holds ``max_slices * npatch`` jobs (borrowed: the
    plan must stay open).  ``starts_*``: the window starts per axis, ``taper_*``: the blend's taper per axis (float32 on the device).  Window ``p = a * n_xl + b``
    of slice ``s`` is job ``s * npatch + p``.

    ``test_hook`` (class attribute, None by default): a callable ``hook(windows, done, active)`` that ``functions.POCS.pocs_cube`` calls for every batch of a
    windowed job with the UN-BLENDED window results (``(njobs, w_il, w_xl)``, downloaded for the purpose), the iterations of every window and its activity."""
    test_hook = None

    def __init__(self, plan, nil, nxl, starts_il, starts_xl, taper_il, taper_xl, max_slices):
        self.plan, self.nil, self.nxl, self.max_slices = plan, int(nil), int(nxl), int(max_slices)
        si, sx = (np.ascontiguousarray(s, dtype=np.int32) for s in (starts_il, starts_xl))
        ti, tx = (np.ascontiguousarray(t, dtype=np.float32) for t in (taper_il, taper_xl))
        if ti.shape != (plan.nil,) or tx.shape != (plan.nxl,):
            raise ValueError(f"tapers of {ti.shape[0]} and {tx.shape[0]} points for windows of {plan.nil} x {plan.nxl}")
        self.npatch = si.size * sx.size
        self.handle = None
        h = C.c_void_p()
        check(lib().p3d_patch_plan_create(C.byref(h), plan.handle, self.nil, self.nxl, _ptr(si), si.size, _ptr(sx), sx.size, _ptr(ti), _ptr(tx), self.max_slices))
        self.handle = h
        n, jobs, res = C.c_int(), C.c_int(), C.c_int()
        check(lib().p3d_patch_plan_info(self.handle, C.byref(n), C.byref(jobs), C.byref(res)))
        assert n.value == self.npatch
        self.max_jobs, self.resident_shape = jobs.value, bool(res.value)

    def close(self):
        if getattr(self, "handle", None):
            lib().p3d_patch_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        if lib is not None:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def gather_dev(self, cube_ptr, dtype, nslices, patches_ptr):
        """cube (device, [nslices][nil][nxl]) -> patch cube (device, [nslices * npatch][w_il][w_xl])."""
        check(lib().p3d_patch_gather_dev(self.handle, cube_ptr, dtype, int(nslices), patches_ptr))

    def mask_dev(self, mask_ptr, mask_slices, nslices, windows_ptr=None):
        """Pack the windows of the float32 mask on the device (``mask_slices`` 1: shared, ``nslices``: one per slice) for `run_dev`; with ``windows_ptr``
        also one float32 mask window per job, for the plan's own loops.  Returns True when a weight is neither 0 nor 1."""
        odd = C.c_int(0)
        check(lib().p3d_patch_mask_dev(self.handle, mask_ptr, int(mask_slices), int(nslices), windows_ptr, C.byref(odd)))
        return bool(odd.value)

    def route(self, thresh_op="hard", version="regular", transform="FFT", norm=None):
        """True when `run_dev` (the single-kernel loop; ``transform='DCT'``: `dct_run_dev` with the DCT pair of ``norm``) takes such a job with the masks of
        the last `mask_dev`."""
        if thresh_op not in P3D_OP or transform not in ("FFT", "DCT"):
            return False
        one = C.c_int(0)
        prm = Plan._params(1, thresh_op, version, 0.0, 1.0, False)
        if transform == "DCT":
            if norm not in P3D_DCT_NORM:
                return False
            check(lib().p3d_patch_dct_route(self.handle, C.byref(prm), P3D_DCT_NORM[norm], C.byref(one)))
        else:
            check(lib().p3d_patch_route(self.handle, C.byref(prm), C.byref(one)))
        return bool(one.value)

    def run_dev(self, patches_ptr, dtype, tau, niter, out_ptr, nslices, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None):
        """The loop of every window of ``nslices`` slices in one kernel.  tau: broadcasts to (nslices * npatch, niter).  Returns (niter_done, sums, device ms)."""
        n = int(nslices) * self.npatch
        t = _tau_table(tau, (n, niter))
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        prm = Plan._params(niter, thresh_op, version, eps, alpha, False)
        done = np.zeros(n, np.int32)
        sums = np.zeros((niter + 1, n), np.float64)
        ms = C.c_double(0.0)
        check(lib().p3d_patch_run_dev(self.handle, patches_ptr, dtype, _ptr(t), None if act is None else _ptr(act), C.byref(prm), out_ptr, int(nslices), _ptr(done),
                                      _ptr(sums), C.byref(ms)))
        return done, sums, ms.value

    def dct_run_dev(self, patches_ptr, dtype, tau, niter, out_ptr, nslices, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None, norm=None):
        """`run_dev` with scipy.fft.dctn / idctn (type 2, ``norm``) as the transform of every window: the single-kernel DCT loop.  tau: the schedule of the
        windows' DCT spectra.  Returns (niter_done, sums, device ms)."""
        n = int(nslices) * self.npatch
        t = _tau_table(tau, (n, niter))
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        prm = Plan._params(niter, thresh_op, version, eps, alpha, False)
        done = np.zeros(n, np.int32)
        sums = np.zeros((niter + 1, n), np.float64)
        ms = C.c_double(0.0)
        check(lib().p3d_patch_dct_run_dev(self.handle, patches_ptr, dtype, _ptr(t), None if act is None else _ptr(act), C.byref(prm), Plan._dct_norm(norm), out_ptr,
                                          int(nslices), _ptr(done), _ptr(sums), C.byref(ms)))
        return done, sums, ms.value

    def blend_dev(self, patches_ptr, dtype, active, out_ptr, nslices):
        """Window results (device) -> blended cube (device, [nslices][nil][nxl]); ``active``: one flag per job (None: all)."""
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        check(lib().p3d_patch_blend_dev(self.handle, patches_ptr, dtype, None if act is None else _ptr(act), out_ptr, int(nslices)))


def vol_shape_supported(n0, n1, n2):
    return bool(lib().p3d_vol_shape_supported(int(n0), int(n1), int(n2)))


class VolumePlan(_PlanBase):
    """p3d_vol_plan wrapper: 3-D FFT POCS of one ``(n0, n1, n2)`` volume (csrc/p3d_vol.hip).  ``plan``: a :class:`Plan` for ``(n1, n2)`` slices on the same
    device to borrow (kept alive here), or None: the volume plan owns one.  ``max_slices`` is 1: a volume is one job."""
    _DESTROY = "p3d_vol_plan_destroy"
    _ENTRY, _HOOK = "p3d_vol_", "c64"        # the C entries are _ENTRY + name; the transform hooks end in _HOOK, the type they take
    max_slices = 1

    def __init__(self, n0, n1, n2, device=0, plan=None):
        self.n0, self.n1, self.n2, self.device = int(n0), int(n1), int(n2), int(device)
        self.shape = (self.n0, self.n1, self.n2)
        self.plan = plan
        h = C.c_void_p()
        check(self._c("plan_create")(C.byref(h), self.device, self.n0, self.n1, self.n2, None if plan is None else plan.handle))
        self.handle = h

    def _c(self, name):
        return getattr(lib(), self._ENTRY + name)

    def _volume(self, x, complex_only=False):
        x = np.asarray(x)
        if x.shape != self.shape:
            raise ValueError(f"expected a volume of shape {self.shape}, got {x.shape}")
        if complex_only or np.iscomplexobj(x):
            return np.ascontiguousarray(x, dtype=np.complex64), P3D_C64
        return np.ascontiguousarray(x, dtype=np.float32), P3D_F32

    def fft3(self, x, inverse=False):
        """np.fft.fftn (``inverse``: ifftn) of a complex64 volume through the loop's own passes."""
        xc, _ = self._volume(x, complex_only=True)
        out = np.empty_like(xc)
        check(self._c("fft3_" + self._HOOK)(self.handle, _ptr(xc), _ptr(out), int(bool(inverse))))
        return out

    def fft3_dev(self, in_ptr, out_ptr, inverse=False):
        check(self._c("fft3_" + self._HOOK + "_dev")(self.handle, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(bool(inverse))))

    def shrink(self, x, tau, thresh_op="hard"):
        """threshold(fftn(x), tau, kind) on the device: the keep / zero decision of every coefficient."""
        xc, _ = self._volume(x, complex_only=True)
        t = _tau_table(tau, ())
        out = np.empty_like(xc)
        check(self._c("shrink_" + self._HOOK)(self.handle, _ptr(xc), _ptr(t), P3D_OP[thresh_op], _ptr(out)))
        return out

    def stats(self, x):
        """The six statistics of ``fftn(x)`` as a (1, 6) array (one row: the volume), the layout ``_schedule_from_stats`` takes."""
        xc, dt = self._volume(x)
        st = np.empty((1, STATS_PER_SLICE), np.float64)
        check(self._c("stats")(self.handle, _ptr(xc), dt, _ptr(st)))
        return st

    def stats_dev(self, x_ptr, dtype):
        st = np.empty((1, STATS_PER_SLICE), np.float64)
        check(self._c("stats_dev")(self.handle, C.c_void_p(x_ptr), int(dtype), _ptr(st)))
        return st

    def _run(self, entry, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op, version, eps, alpha, mask_per_slice, profile=False):
        t = _tau_table(tau, (int(niter),))
        prm = Plan._params(niter, thresh_op, version, eps, alpha, profile, False, mask_per_slice)
        if prm.thresh_op & P3D_OP_PERCENTILE:
            raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"thresh_op {thresh_op!r} is not implemented for volumes")
        done = np.zeros(1, np.int32)
        sums = np.zeros(int(niter) + 1, np.float64)
        ms = C.c_double(0.0)
        check(self._c(entry)(self.handle, C.c_void_p(x_ptr), int(dtype), C.c_void_p(mask_ptr), _ptr(t), C.byref(prm), C.c_void_p(out_ptr), _ptr(done),
                             _ptr(sums), C.byref(ms)))
        return int(done[0]), sums, ms.value

    def run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0):
        """Host arrays in, host array out; ``mask`` (n1, n2) or (n0, n1, n2); ``tau``: (niter,), real or complex.  Returns (out, niter_done, sums,
        elapsed_ms) with sums[k] = sum |x_k| over the volume."""
        xc, dt = self._volume(x)
        m = np.ascontiguousarray(mask, dtype=self._MASK_DT)
        if m.shape != self.shape[1:] and m.shape != self.shape:
            raise ValueError(f"mask shape {m.shape} is neither {self.shape[1:]} nor {self.shape}")
        out = np.empty_like(xc)
        done, sums, ms = self._run("run", xc.ctypes.data, dt, m.ctypes.data, tau, niter, out.ctypes.data, thresh_op, version, eps, alpha, m.ndim == 3)
        return out, done, sums, ms

    def run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, mask_per_slice=False,
                profile=False):
        """`run` on device pointers (``out_ptr`` may be ``x_ptr``); ``profile``: time every axis-0 pass (`last_profile`).  Returns (niter_done, sums,
        elapsed_ms)."""
        return self._run("run_dev", x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op, version, eps, alpha, mask_per_slice, profile)

    def last_profile(self):
        """After a run with ``profile=True``: mean device milliseconds of the axis-0 pass and its launches."""
        ms, n = C.c_double(), C.c_int()
        check(self._c("last_profile")(self.handle, C.byref(ms), C.byref(n)))
        return {"zpass_ms": ms.value, "zpass_launches": n.value}


def voldct_shape_supported(n0, n1, n2):
    return bool(lib().p3d_voldct_shape_supported(int(n0), int(n1), int(n2)))


class VolumePlanDct(VolumePlan):
    """p3d_voldct_plan wrapper: 3-D DCT POCS of one ``(n0, n1, n2)`` volume (csrc/p3d_vol_dct.hip), scipy.fft.dctn / idctn (type 2) over all three axes.
    The methods of :class:`VolumePlan` with a ``norm`` keyword (None / 'backward' / 'ortho'); the transform hook is `dct3`.  ``plan``: a :class:`Plan` for
    ``(n1, n2)`` slices to borrow, or None."""
    _DESTROY = "p3d_voldct_plan_destroy"
    _ENTRY, _HOOK = "p3d_voldct_", "c64"

    def dct3(self, x, inverse=False, norm=None):
        """scipy.fft.dctn (``inverse``: idctn) of a complex64 volume through the loop's own passes."""
        xc, _ = self._volume(x, complex_only=True)
        out = np.empty_like(xc)
        check(self._c("dct3_c64")(self.handle, _ptr(xc), _ptr(out), Plan._dct_norm(norm), int(bool(inverse))))
        return out

    def dct3_dev(self, in_ptr, out_ptr, inverse=False, norm=None):
        check(self._c("dct3_c64_dev")(self.handle, C.c_void_p(in_ptr), C.c_void_p(out_ptr), Plan._dct_norm(norm), int(bool(inverse))))

    def fft3(self, *args, **kwargs):
        """Not part of this plan: there is no ``p3d_voldct_fft3_*`` entry."""
        raise UnsupportedError(P3D_ERR_UNSUPPORTED, "VolumePlanDct has no fft3 / fft3_dev: its transform hooks are dct3 / dct3_dev")

    fft3_dev = fft3

    def shrink(self, x, tau, thresh_op="hard", norm=None):
        """threshold(dctn(x), tau, kind) on the device: the keep / zero decision of every coefficient."""
        xc, _ = self._volume(x, complex_only=True)
        t = _tau_table(tau, ())
        out = np.empty_like(xc)
        check(self._c("shrink_c64")(self.handle, _ptr(xc), _ptr(t), P3D_OP[thresh_op], Plan._dct_norm(norm), _ptr(out)))
        return out

    def stats(self, x, norm=None):
        """The six statistics of ``dctn(x)`` as a (1, 6) array (one row: the volume), the layout ``_schedule_from_stats`` takes."""
        xc, dt = self._volume(x)
        st = np.empty((1, STATS_PER_SLICE), np.float64)
        check(self._c("stats")(self.handle, _ptr(xc), dt, Plan._dct_norm(norm), _ptr(st)))
        return st

    def stats_dev(self, x_ptr, dtype, norm=None):
        st = np.empty((1, STATS_PER_SLICE), np.float64)
        check(self._c("stats_dev")(self.handle, C.c_void_p(x_ptr), int(dtype), Plan._dct_norm(norm), _ptr(st)))
        return st

    def _run(self, entry, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op, version, eps, alpha, mask_per_slice, profile=False, norm=None):
        t = _tau_table(tau, (int(niter),))
        prm = Plan._params(niter, thresh_op, version, eps, alpha, profile, False, mask_per_slice)
        if prm.thresh_op & P3D_OP_PERCENTILE:
            raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"thresh_op {thresh_op!r} is not implemented for volumes")
        done = np.zeros(1, np.int32)
        sums = np.zeros(int(niter) + 1, np.float64)
        ms = C.c_double(0.0)
        check(self._c(entry)(self.handle, C.c_void_p(x_ptr), int(dtype), C.c_void_p(mask_ptr), _ptr(t), C.byref(prm), Plan._dct_norm(norm), C.c_void_p(out_ptr),
                             _ptr(done), _ptr(sums), C.byref(ms)))
        return int(done[0]), sums, ms.value

    def run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, norm=None):
        """`VolumePlan.run` with the DCT pair of ``norm``; ``tau``: the schedule of ``dctn(x)``."""
        xc, dt = self._volume(x)
        m = np.ascontiguousarray(mask, dtype=self._MASK_DT)
        if m.shape != self.shape[1:] and m.shape != self.shape:
            raise ValueError(f"mask shape {m.shape} is neither {self.shape[1:]} nor {self.shape}")
        out = np.empty_like(xc)
        done, sums, ms = self._run("run", xc.ctypes.data, dt, m.ctypes.data, tau, niter, out.ctypes.data, thresh_op, version, eps, alpha, m.ndim == 3, norm=norm)
        return out, done, sums, ms

    def run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, mask_per_slice=False,
                profile=False, norm=None):
        """`VolumePlan.run_dev` with the DCT pair of ``norm``."""
        return self._run("run_dev", x_ptr, dtype, mask_ptr, tau, niter, out_ptr, thresh_op, version, eps, alpha, mask_per_slice, profile, norm)


def vol64_shape_supported(n0, n1, n2):
    return bool(lib().p3d_vol64_shape_supported(int(n0), int(n1), int(n2)))


class VolumePlan64(VolumePlan):
    """p3d_vol64_plan wrapper: the volume loop in double precision (csrc/p3d_vol64.hip) with the methods of :class:`VolumePlan`.  Volumes of complex128,
    float64, complex64 and float32 go in as they are (anything else is widened) and come back in their own type; the arithmetic is double, the mask
    float64, the transform hooks take complex128.  ``plan``: a :class:`Plan64` for ``(n1, n2)`` slices to borrow, or None."""
    _DESTROY = "p3d_vol64_plan_destroy"
    _ENTRY, _HOOK = "p3d_vol64_", "c128"
    _MASK_DT = np.float64

    def _volume(self, x, complex_only=False):
        x = np.asarray(x)
        if x.shape != self.shape:
            raise ValueError(f"expected a volume of shape {self.shape}, got {x.shape}")
        if complex_only:
            return np.ascontiguousarray(x, dtype=np.complex128), P3D_C128
        if x.dtype not in _PlanBase64._DT:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        return np.ascontiguousarray(x), _PlanBase64._DT[x.dtype]


# ---- WAVELET variant -----------------------------------------------------------------------
_BANKS = None


def wavelet_filters(name):
    """(dec_lo, dec_hi, rec_lo, rec_hi) of a PyWavelets wavelet name (data file wavelets.json; pywt is not required)."""
    global _BANKS
    if _BANKS is None:
        import json
        with open(os.path.join(_HERE, "wavelets.json")) as f:
            _BANKS = json.load(f)["wavelets"]
    try:
        b = _BANKS[str(name)]
    except KeyError:
        raise ValueError(f"Unknown wavelet name {name!r}, check wavelets.json for the list of available builtin wavelets.") from None
    return tuple(np.ascontiguousarray(b[k], dtype=np.float64) for k in ("dec_lo", "dec_hi", "rec_lo", "rec_hi"))


class WaveletPlan(_PlanBase):
    """p3d_wplan wrapper: multilevel 2-D DWT ('smooth' extension) of (nil, nxl) slices and the WAVELET POCS loop.  tau: (nslices, niter, nlev, 3),
    levels coarse -> fine."""
    _DESTROY, _RUN = "p3d_wavelet_plan_destroy", "p3d_wavelet_run"

    def __init__(self, nil, nxl, max_slices, wavelet="coif5", level=None, device=0):
        self.nil, self.nxl, self.max_slices, self.device = int(nil), int(nxl), int(max_slices), int(device)
        self.wavelet = wavelet
        bank = _filter_bank(wavelet)
        h = C.c_void_p()
        check(lib().p3d_wavelet_plan_create(C.byref(h), self.device, self.nil, self.nxl, self.max_slices, *map(_ptr, bank),
                                            bank[0].size, -1 if level is None else int(level)))
        self.handle = h
        nlev, ncoef = C.c_int(0), C.c_int64(0)
        check(lib().p3d_wavelet_info(self.handle, C.byref(nlev), C.byref(ncoef), None))
        self.nlev, self.ncoef = nlev.value, ncoef.value
        shapes = np.zeros((self.nlev + 1, 2), np.int32)
        check(lib().p3d_wavelet_info(self.handle, None, None, _ptr(shapes)))
        self.shapes = [tuple(int(v) for v in r) for r in shapes]   # cA, then details coarsest -> finest

    def _tau_shape(self):
        return (self.nlev, 3)

    def unpack(self, vec):
        """flat coefficient vector of ONE slice -> [cA, (cH, cV, cD), ...] like pywt.wavedec2."""
        r, c = self.shapes[0]
        out, off = [vec[:r * c].reshape(r, c)], r * c
        for r, c in self.shapes[1:]:
            det = []
            for _ in range(3):
                det.append(vec[off:off + r * c].reshape(r, c))
                off += r * c
            out.append(tuple(det))
        return out

    def pack(self, coeffs):
        return np.concatenate([np.ravel(coeffs[0])] + [np.ravel(d) for lvl in coeffs[1:] for d in lvl]).astype(np.complex64)

    def wavedec2(self, x):
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        coef = np.empty((xc.shape[0], self.ncoef), np.complex64)
        check(lib().p3d_wavedec2_c64(self.handle, _ptr(xc), _ptr(coef), xc.shape[0]))
        return coef[0] if squeeze else coef

    def waverec2(self, coef):
        coef = np.ascontiguousarray(coef, dtype=np.complex64)
        squeeze = coef.ndim == 1
        coef = coef.reshape(-1, self.ncoef)
        if coef.shape[0] > self.max_slices:
            raise ValueError(f"{coef.shape[0]} slices > max_slices {self.max_slices}")
        out = np.empty((coef.shape[0], self.nil, self.nxl), np.complex64)
        check(lib().p3d_waverec2_c64(self.handle, _ptr(coef), _ptr(out), coef.shape[0]))
        return out[0] if squeeze else out

    def stats_dev(self, x_ptr, dtype, n):
        """(nslices, nlev, 3, 4): Re/Im of the lexicographic max, max |d|, min |d| per detail array (coarsest level first); raw pointer (host or
        device), P3D_C64 / P3D_F32."""
        st = np.empty((n, self.nlev, 3, 4), np.float64)
        check(lib().p3d_wavelet_stats(self.handle, x_ptr, dtype, n, _ptr(st)))
        return st


# ---- the loop in the reference's precision ---------------------------------------------------
class Plan64(_PlanBase64):
    """p3d_plan64 wrapper: the FFT POCS loop in double precision (include/p3d.h) for complex128 / float64 cubes, and for complex64 /
    float32 cubes whose reference run is a double-precision one (soft / garrote / FPOCS / APOCS, or any run under NumPy < 2)."""
    _DESTROY, _RUN = "p3d_plan64_destroy", "p3d_pocs64_run"

    def __init__(self, nil, nxl, max_slices, device=0):
        self.nil, self.nxl, self.max_slices, self.device = int(nil), int(nxl), int(max_slices), int(device)
        h = C.c_void_p()
        check(lib().p3d_plan64_create(C.byref(h), self.device, self.nil, self.nxl, self.max_slices))
        self.handle = h

    def fft2(self, x, inverse=False):
        """Test hook: fft2 / ifft2 of complex128 slices through the loop's own passes (``p3d_fft2_c128``)."""
        xc = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
        squeeze = xc.ndim == 2
        if squeeze:
            xc = xc[None]
        if xc.shape[1:] != (self.nil, self.nxl) or xc.shape[0] > self.max_slices:
            raise ValueError(f"expected (<= {self.max_slices}, {self.nil}, {self.nxl}), got {xc.shape}")
        out = np.empty_like(xc)
        check(lib().p3d_fft2_c128(self.handle, _ptr(xc), _ptr(out), xc.shape[0], 1 if inverse else 0))
        return out[0] if squeeze else out

    def stats_dev(self, x_ptr, dtype, n):
        """(nslices, 6) float64, the layout of ``Plan.stats``: statistics of the double-precision ``fft2(x)``; raw pointer (host or device)."""
        st = np.empty((n, 6), np.float64)
        check(lib().p3d_pocs64_stats(self.handle, x_ptr, dtype, n, _ptr(st)))
        return st

    # ---- order statistics of the double-precision spectrum (csrc/p3d_select64.hip), mirroring Plan's methods ---------------------
    def percentile(self, spectrum, perc):
        """Test hook: ``np.percentile(np.abs(spectrum[s]), perc[s])`` per complex128 slice through the loop's own select kernels."""
        xc = np.ascontiguousarray(np.asarray(spectrum, dtype=np.complex128))
        if xc.ndim != 3 or xc.shape[1:] != (self.nil, self.nxl) or xc.shape[0] > self.max_slices:
            raise ValueError(f"expected (<= {self.max_slices}, {self.nil}, {self.nxl}), got {xc.shape}")
        pc = np.ascontiguousarray(np.broadcast_to(np.asarray(perc, dtype=np.float64), (xc.shape[0],)))
        thr = np.empty((xc.shape[0],), np.float64)
        check(lib().p3d_pocs64_percentile(self.handle, _ptr(xc), xc.shape[0], _ptr(pc), _ptr(thr)))
        return thr

    def sorted_spectrum(self, x):
        """The double-precision fft2 of every slice, sorted on the device in NumPy's complex order (kept in the plan); returns x_fwd.max() per
        slice (complex128) -- first half of the 'data-driven' schedule (POCS.py:356-362).  ``x``: a host cube of any of the four dtypes."""
        xc, dt = self._cube(x)
        return self.sorted_spectrum_dev(xc.ctypes.data, dt, xc.shape[0])

    def sorted_spectrum_dev(self, x_ptr, dtype, n):
        """`sorted_spectrum` on a raw pointer (host or device) to ``n`` slices of ``dtype``."""
        peaks = np.empty((n, 2), np.float64)
        check(lib().p3d_pocs64_sorted_spectrum(self.handle, C.c_void_p(x_ptr), dtype, n, _ptr(peaks)))
        return peaks.view(np.complex128)[:, 0]

    def data_driven_pick(self, tau_min, tau_max, niter):
        """Second half: per slice the number of coefficients strictly between the bounds (complex128, NumPy's order) and the niter
        thresholds picked from them (POCS.py:359-362); must follow sorted_spectrum directly."""
        lo = np.ascontiguousarray(tau_min, dtype=np.complex128)
        hi = np.ascontiguousarray(tau_max, dtype=np.complex128)
        n = lo.shape[0]
        bounds = np.empty((n, 4), np.float64)
        bounds[:, 0], bounds[:, 1], bounds[:, 2], bounds[:, 3] = lo.real, lo.imag, hi.real, hi.imag
        tau = np.empty((n, int(niter), 2), np.float64)
        count = np.empty((n,), np.int64)
        check(lib().p3d_pocs64_data_driven_pick(self.handle, n, int(niter), _ptr(bounds), _ptr(tau), _ptr(count)))
        return tau.view(np.complex128)[..., 0], count

    # ---- transform_kind = 'DCT' in double precision (csrc/p3d_dct64.hip): hard / soft / garrote, mirroring Plan.dct_* ------------
    _dct_norm = staticmethod(Plan._dct_norm)

    @staticmethod
    def _dct_op(thresh_op):
        if thresh_op not in ("hard", "soft", "garrote"):
            raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"thresh_op {thresh_op!r}: the double-precision DCT loop has hard, soft and garrote")

    def dct2(self, x, inverse=False, norm=None):
        """Test hook: scipy.fft.dctn (``inverse``: idctn) of complex128 slices over the last two axes, type 2, through the loop's own passes."""
        norm = self._dct_norm(norm)
        xc = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
        squeeze = xc.ndim == 2
        if squeeze:
            xc = xc[None]
        if xc.ndim != 3 or xc.shape[1:] != (self.nil, self.nxl) or xc.shape[0] > self.max_slices:
            raise ValueError(f"expected (<= {self.max_slices}, {self.nil}, {self.nxl}), got {xc.shape}")
        out = np.empty_like(xc)
        check(lib().p3d_dct2_c128(self.handle, _ptr(xc), _ptr(out), xc.shape[0], 1 if inverse else 0, norm))
        return out[0] if squeeze else out

    def dct_stats_dev(self, x_ptr, dtype, n, norm=None):
        """`stats_dev` of the double-precision ``dctn(x)``; raw pointer (host or device)."""
        norm = self._dct_norm(norm)
        st = np.empty((n, 6), np.float64)
        check(lib().p3d_pocs64_dct_stats(self.handle, x_ptr, dtype, n, _ptr(st), norm))
        return st

    def dct_run(self, x, mask, tau, niter, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None, norm=None):
        """`run` with the DCT pair as the transform.  Returns (out, niter_done, sums, elapsed_ms)."""
        self._dct_norm(norm)      # (both refusals come before the cube is converted)
        self._dct_op(thresh_op)
        xc, dt, m, out = self._host_job(x, mask)
        done, sums, ms = self.dct_run_dev(xc.ctypes.data, dt, m.ctypes.data, tau, niter, out.ctypes.data, xc.shape[0], thresh_op=thresh_op, version=version,
                                          eps=eps, alpha=alpha, active=active, norm=norm, mask_per_slice=m.ndim == 3)
        return out, done, sums, ms

    def dct_run_dev(self, x_ptr, dtype, mask_ptr, tau, niter, out_ptr, n, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None,
                    norm=None, mask_per_slice=False):
        """`run_dev` with the DCT pair as the transform (pointers host or device).  Returns (niter_done, sums, device ms of the loop)."""
        norm = self._dct_norm(norm)
        self._dct_op(thresh_op)
        return self._run_entry("p3d_pocs64_dct_run", x_ptr, dtype, mask_ptr, tau, niter, out_ptr, n, thresh_op, version, eps, alpha, active,
                               extra=(norm,), mask_per_slice=mask_per_slice)


# ---- SHEARLET variant ----------------------------------------------------------------------
class ShearletPlan(_PlanBase):
    """p3d_splan wrapper: frequency-domain shearlet frame with caller-supplied spectra ``psi`` (nil, nxl, nsh) -- the layout of
    ``FFST.scalesShearsAndSpectra`` -- and the SHEARLET POCS loop for up to ``max_slices`` slices per call.  tau: (nslices, niter, nsh)."""
    _DESTROY, _RUN = "p3d_shearlet_plan_destroy", "p3d_shearlet_run"

    def __init__(self, psi, max_slices=1, device=0):
        psi = _real_psi(psi)
        self.nil, self.nxl, self.nsh = (int(v) for v in psi.shape)
        self.max_slices, self.device = int(max_slices), int(device)
        dev_psi = np.ascontiguousarray(np.moveaxis(psi, -1, 0), dtype=np.float32)
        h = C.c_void_p()
        check(lib().p3d_shearlet_plan_create(C.byref(h), self.device, self.nil, self.nxl, self.nsh, _ptr(dev_psi), self.max_slices))
        self.handle = h
        frac, paired = C.c_double(1.0), C.c_int(0)
        check(lib().p3d_shearlet_info(self.handle, C.byref(frac), C.byref(paired)))
        # share of the (shearlet, 8-row group) pairs on which the spectrum does not vanish: what the fused passes actually touch;
        # float32 cubes on symmetric spectra additionally work on Hermitian half slices, two columns per transform
        self.row_group_fraction, self.paired = frac.value, bool(paired.value)

    def _tau_shape(self):
        return (self.nsh,)

    def transform(self, x):
        """(…, nil, nxl) -> (…, nil, nxl, nsh) complex64 (the reference's layout: shearlets on the last axis)."""
        x = np.asarray(x)
        squeeze = x.ndim == 2
        xc, _ = self._cube(x.astype(np.complex64, copy=False))
        st = np.empty((xc.shape[0], self.nsh, self.nil, self.nxl), np.complex64)
        check(lib().p3d_shearlet_transform_c64(self.handle, _ptr(xc), _ptr(st), xc.shape[0]))
        st = np.moveaxis(st, 1, -1)
        return st[0] if squeeze else st

    def inverse(self, st):
        st = np.asarray(st)
        squeeze = st.ndim == 3
        if squeeze:
            st = st[None]
        if st.shape[1:] != (self.nil, self.nxl, self.nsh) or st.shape[0] > self.max_slices:
            raise ValueError(f"expected (<= {self.max_slices}, {self.nil}, {self.nxl}, {self.nsh}), got {st.shape}")
        dev = np.ascontiguousarray(np.moveaxis(st, -1, 1), dtype=np.complex64)
        out = np.empty((st.shape[0], self.nil, self.nxl), np.complex64)
        check(lib().p3d_shearlet_inverse_c64(self.handle, _ptr(dev), _ptr(out), st.shape[0]))
        return out[0] if squeeze else out

    def stats_dev(self, x_ptr, dtype, n):
        """(nslices, nsh, 5): Re/Im of the lexicographic (real cubes: signed) max, max |c|, min |c|, sum |c|^2 per shearlet; raw pointer (host or
        device), P3D_C64 / P3D_F32."""
        st = np.empty((n, self.nsh, 5), np.float64)
        check(lib().p3d_shearlet_stats(self.handle, x_ptr, dtype, n, _ptr(st)))
        return st


def shearlet64_fused_shape(nil, nxl):
    """True when the double-precision SHEARLET loop runs its fused passes for (nil, nxl) slices (both extents on the register engine)."""
    return bool(lib().p3d_shearlet64_fused_shape(int(nil), int(nxl)))


class ShearletPlan64(_PlanBase64):
    """p3d_splan64 wrapper: the SHEARLET POCS loop in double precision (include/p3d.h) for complex128 / float64 cubes, and for complex64 /
    float32 cubes on request (``precision='reference'``); ``psi`` (nil, nxl, nsh) as for :class:`ShearletPlan`, kept in double.
    tau: (nslices, niter, nsh)."""
    _DESTROY, _RUN = "p3d_shearlet64_plan_destroy", "p3d_shearlet64_run"

    def __init__(self, psi, max_slices=1, device=0):
        psi = _real_psi(psi)
        self.nil, self.nxl, self.nsh = (int(v) for v in psi.shape)
        self.max_slices, self.device = int(max_slices), int(device)
        dev_psi = np.ascontiguousarray(np.moveaxis(psi, -1, 0), dtype=np.float64)
        h = C.c_void_p()
        check(lib().p3d_shearlet64_plan_create(C.byref(h), self.device, self.nil, self.nxl, self.nsh, _ptr(dev_psi), self.max_slices))
        self.handle = h
        fused, frac = C.c_int(0), C.c_double(1.0)
        check(lib().p3d_shearlet64_info(self.handle, C.byref(fused), C.byref(frac)))
        self.fused = bool(fused.value & 1)   # three fused passes per iteration on the double-precision register engine (both extents have a plan there)
        self.paired = bool(fused.value & 2)  # ... and real cubes on Hermitian coefficient slices, two columns per transform (symmetric spectra, even extents)
        self.row_group_fraction = frac.value   # share of the (shearlet, row group) pairs those passes touch (rows off a spectrum's support are skipped)

    def _tau_shape(self):
        return (self.nsh,)

    def stats_dev(self, x_ptr, dtype, n):
        """(nslices, nsh, 5): Re / Im of the lexicographic (real cubes: signed) max, max |c|, min |c|, sum |c|^2 per shearlet, in double."""
        st = np.empty((n, self.nsh, 5), np.float64)
        check(lib().p3d_shearlet64_stats(self.handle, x_ptr, dtype, n, _ptr(st)))
        return st


def time2freq(x, dt, t0=0.0, nfft=None, real_only=False, window=None, device=0):
    """(nt, ...) float32 -> (nfreq, ...) complex64 with xrft's true_phase / true_amplitude convention
    (include/p3d.h, p3d_time2freq).  Trailing axes are flattened to traces and restored."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    nt = x.shape[0]
    ntr = int(np.prod(x.shape[1:])) if x.ndim > 1 else 1
    nfft = int(nfft or nt)
    nfreq = nfft // 2 + 1 if real_only else nfft
    out = np.empty((nfreq,) + x.shape[1:], np.complex64)
    win = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
    if win is not None and win.shape != (nfreq,):
        raise ValueError(f"window must have {nfreq} entries")
    check(lib().p3d_time2freq(int(device), _ptr(x), nt, ntr, float(dt), float(t0), nfft, int(bool(real_only)),
                              None if win is None else _ptr(win), _ptr(out)))
    return out


def freq2time(X, dt, t0=0.0, nfft=None, real_only=False, kidx=None, device=0):
    """(nfreq, ...) complex64 -> (nfft, ...) float32: exact inverse of :func:`time2freq` (real part)."""
    X = np.ascontiguousarray(X, dtype=np.complex64)
    nfreq = X.shape[0]
    ntr = int(np.prod(X.shape[1:])) if X.ndim > 1 else 1
    if nfft is None:
        nfft = 2 * (nfreq - 1) if real_only else nfreq
    nfft = int(nfft)
    k = np.arange(nfreq, dtype=np.int32) if kidx is None else np.ascontiguousarray(kidx, dtype=np.int32)
    out = np.empty((nfft,) + X.shape[1:], np.float32)
    check(lib().p3d_freq2time(int(device), _ptr(X), nfreq, _ptr(k), ntr, float(dt), float(t0), nfft, int(bool(real_only)),
                              _ptr(out)))
    return out


def smooth_slices(x, kind, device=0, **kw):
    """scipy.ndimage.gaussian_filter / median_filter ('reflect' boundary) of every (ny, nx) slice of a float32 stack
    (include/p3d.h, p3d_smooth_gaussian / p3d_smooth_median)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError("expected a stack of slices (n, ny, nx)")
    out = np.empty_like(x)
    n, ny, nx = x.shape
    if kind == "gaussian":
        check(lib().p3d_smooth_gaussian(int(device), _ptr(x), n, ny, nx, float(kw["sigma"]), float(kw.get("truncate", 4.0)), _ptr(out)))
    elif kind == "median":
        check(lib().p3d_smooth_median(int(device), _ptr(x), n, ny, nx, int(kw["size"]), _ptr(out)))
    else:
        raise ValueError(f"unknown smoothing filter {kind!r}")
    return out


AGC_KIND = {"rms": 0, "mean": 1, "median": 2}


def agc(x, win, kind="rms", squared=False, return_gain=False, device=0):
    """Automatic gain control along axis 0 of a float32 array [nt][ntraces...] (include/p3d.h, p3d_agc); returns a new array
    (and the gain function when ``return_gain``)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim < 1 or x.size == 0:
        raise ValueError("expected a non-empty array with time on axis 0")
    nt = x.shape[0]
    ntr = x.size // nt
    out = np.empty_like(x)
    gain = np.empty_like(x) if return_gain else None
    check(lib().p3d_agc(int(device), _ptr(x), nt, ntr, int(win), AGC_KIND[kind], int(bool(squared)), _ptr(out),
                        None if gain is None else _ptr(gain)))
    return (out, gain) if return_gain else out


def upsample_slices(x, iy, wy, ix, wx, device=0):
    """Separable linear / nearest upsampling of a stack of (ny, nx) slices, float32 or complex64 (include/p3d.h, p3d_upsample):
    output line o of an axis reads source line idx[o] and, with weight w[o], line idx[o] + 1."""
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("expected a stack of slices (n, ny, nx)")
    if np.iscomplexobj(x):
        x, dtype = np.ascontiguousarray(x, dtype=np.complex64), P3D_C64
    else:
        x, dtype = np.ascontiguousarray(x, dtype=np.float32), P3D_F32
    iy, ix = np.ascontiguousarray(iy, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.int32)
    wy, wx = np.ascontiguousarray(wy, dtype=np.float32), np.ascontiguousarray(wx, dtype=np.float32)
    n, ny, nx = x.shape
    out = np.empty((n, iy.size, ix.size), x.dtype)
    check(lib().p3d_upsample(int(device), _ptr(x), dtype, n, ny, nx, _ptr(iy), _ptr(wy), iy.size, _ptr(ix), _ptr(wx), ix.size, _ptr(out)))
    return out


BIN_METHOD = {"average": 0, "median": 1, "nearest": 2, "IDW": 3}


def _bin_tables(samples, trace_off, trace_len, shift, weight, bin_start, nil, nxl, method):
    samples = np.ascontiguousarray(samples, dtype=np.float32).ravel()
    trace_off = np.ascontiguousarray(trace_off, dtype=np.int64)
    trace_len = np.ascontiguousarray(trace_len, dtype=np.int32)
    shift = np.ascontiguousarray(shift, dtype=np.int32)
    bin_start = np.ascontiguousarray(bin_start, dtype=np.int64)
    ntr = trace_off.size
    if trace_len.size != ntr or shift.size != ntr or bin_start.size != int(nil) * int(nxl) + 1:
        raise ValueError("inconsistent binning tables")
    if ntr and int((trace_off + trace_len).max()) > samples.size:
        raise ValueError("a trace reaches past the end of the sample buffer")
    if method not in BIN_METHOD:
        raise ValueError(f"unknown stacking method {method!r} (use one of {sorted(BIN_METHOD)})")
    if method == "IDW":
        if weight is None:
            raise ValueError("IDW needs weights")
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        if weight.size != ntr:
            raise ValueError("one weight per trace")
    else:
        weight = None
    return samples, trace_off, trace_len, shift, weight, bin_start


def bin_stack(samples, trace_off, trace_len, shift, bin_start, nil, nxl, nt, method="average", weight=None, max_bytes=0, device=0):
    """Stack the traces of every (iline, xline) bin into a slice-major float32 cube [nt][nil][nxl] (include/p3d.h, p3d_bin_stack).
    CSR layout: traces in bin order, bin ``il * nxl + xl`` owns traces ``bin_start[b] .. bin_start[b + 1]``; trace t's sample i lands on
    output sample ``i + shift[t]``.  ``max_bytes`` caps the device memory of one chunk of inlines (0: half of the free memory)."""
    samples, trace_off, trace_len, shift, weight, bin_start = _bin_tables(samples, trace_off, trace_len, shift, weight, bin_start, nil, nxl,
                                                                         method)
    out = np.empty((int(nt), int(nil), int(nxl)), np.float32)
    check(lib().p3d_bin_stack(int(device), _ptr(samples), _ptr(trace_off), _ptr(trace_len), _ptr(shift), None if weight is None else _ptr(weight),
                              trace_off.size, _ptr(bin_start), int(nil), int(nxl), int(nt), BIN_METHOD[method], int(max_bytes), _ptr(out)))
    return out


def bin_stack_dev(samples, trace_off, trace_len, shift, bin_start, out, nil, nxl, nt, method="average", weight=None, device=0):
    """p3d_bin_stack_dev on device pointers (integers, e.g. from `DeviceBuffer.ptr`); ``out`` receives [nt][nil][nxl] float32."""
    if method not in BIN_METHOD:
        raise ValueError(f"unknown stacking method {method!r}")
    check(lib().p3d_bin_stack_dev(int(device), samples, trace_off, trace_len, shift, weight, bin_start, int(nil), int(nxl), int(nt),
                                  BIN_METHOD[method], out))


DESPIKE_MODE = {"mean": 0, "median": 1, "rms": 2}
DESPIKE_OUT = {"scaled": 0, "mode": 1, "threshold": 2, "zeros": 3, "median": 4}
DESPIKE_MAX_TRACES = 31      # P3D_DESPIKE_MAX_TRACES of include/p3d.h
DESPIKE_NO_VIEW = 2**31 - 1  # add_start when there is no additional view


def _despike_window(w, mode):
    if mode not in DESPIKE_MODE:
        raise ValueError(f"unknown amplitude mode {mode!r} (use one of {sorted(DESPIKE_MODE)})")
    w = int(w)
    if w % 2 == 0:
        raise ValueError("Number of traces must be odd integer.")
    if w > DESPIKE_MAX_TRACES:
        raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"trace windows of up to {DESPIKE_MAX_TRACES} traces are supported, got {w}")
    return w


def _despike_splits(splits, ntr):
    if splits is None:
        return None, 0
    b = np.ascontiguousarray(splits, dtype=np.int32)
    if b.ndim != 1 or b.size < 2 or b[0] != 0 or b[-1] != ntr or np.any(np.diff(b) <= 0):
        raise ValueError("splits are ascending trace boundaries from 0 to the number of traces")
    return b, b.size - 1


def despike_detect(section, w, mode, threshold, main_end, add_start=None, splits=None, device=0):
    """Candidate mask and per-view counts of a trace-major float32 section [ntr][ns] (include/p3d.h, p3d_despike_detect).  Returns
    ``mask`` uint64 [ntr][ceil(ns / 64)] (bit t % 64 of word t // 64) and ``counts`` int32 [2][ntr] (main view, additional view)."""
    w = _despike_window(w, mode)
    section = np.ascontiguousarray(section, dtype=np.float32)
    if section.ndim != 2:
        raise ValueError("section is [ntraces][nsamples]")
    ntr, ns = section.shape
    b, nb = _despike_splits(splits, ntr)
    mask = np.empty((ntr, (ns + 63) // 64), np.uint64)
    counts = np.empty((2, ntr), np.int32)
    check(lib().p3d_despike_detect(int(device), _ptr(section), ntr, ns, w, DESPIKE_MODE[mode], float(threshold), int(main_end),
                                   DESPIKE_NO_VIEW if add_start is None else int(add_start), None if b is None else _ptr(b), nb, _ptr(mask), _ptr(counts)))
    return mask, counts


def despike_detect_dev(section, ntr, ns, w, mode, threshold, main_end, add_start, mask, counts, splits=None, device=0):
    """p3d_despike_detect_dev on device pointers (``DeviceArray.ptr``): ``mask`` receives [ntr][ceil(ns / 64)] uint64, ``counts`` [2][ntr] int32."""
    w = _despike_window(w, mode)
    b, nb = _despike_splits(splits, ntr)
    check(lib().p3d_despike_detect_dev(int(device), section, int(ntr), int(ns), w, DESPIKE_MODE[mode], float(threshold), int(main_end),
                                       DESPIKE_NO_VIEW if add_start is None else int(add_start), None if b is None else _ptr(b), nb, mask, counts))


def _despike_records(spikes, level_start, mode, out):
    if mode not in DESPIKE_MODE:
        raise ValueError(f"unknown amplitude mode {mode!r}")
    if out not in DESPIKE_OUT:
        raise ValueError(f"unknown output amplitude option {out!r}")
    spikes = np.ascontiguousarray(spikes, dtype=np.int32).reshape(-1, 8)
    level_start = np.ascontiguousarray(level_start, dtype=np.int32)
    return spikes, level_start


def despike_replace(section, spikes, level_start, mode, out, threshold, device=0):
    """Replace the spikes of a trace-major float32 section [ntr][ns]; returns the new section.  ``spikes`` int32 [n][8] records
    (trace, lo, hi, first, last, c0, c1, 0) sorted by level, ``level_start`` the offsets of the levels (include/p3d.h, p3d_despike_replace)."""
    spikes, level_start = _despike_records(spikes, level_start, mode, out)
    res = np.array(section, dtype=np.float32, order="C", copy=True)
    if res.ndim != 2:
        raise ValueError("section is [ntraces][nsamples]")
    check(lib().p3d_despike_replace(int(device), _ptr(res), res.shape[0], res.shape[1], _ptr(spikes), spikes.shape[0], _ptr(level_start),
                                    level_start.size - 1, DESPIKE_MODE[mode], DESPIKE_OUT[out], float(threshold)))
    return res


def despike_replace_dev(section, ntr, ns, spikes, level_start, mode, out, threshold, device=0):
    """p3d_despike_replace_dev: ``section`` is a device pointer, rewritten in place; the records stay on the host."""
    spikes, level_start = _despike_records(spikes, level_start, mode, out)
    check(lib().p3d_despike_replace_dev(int(device), section, int(ntr), int(ns), _ptr(spikes), spikes.shape[0], _ptr(level_start),
                                        level_start.size - 1, DESPIKE_MODE[mode], DESPIKE_OUT[out], float(threshold)))


# ---- step 5: static correction (include/p3d.h, p3d_static.hip) ------------------------------------------------
STATIC_MAX_WIN = 255         # P3D_STATIC_MAX_WIN of include/p3d.h
STATIC_MAX_NLTA = 7680       # P3D_STATIC_MAX_NLTA


def _static_windows(nsta, nlta):
    nsta, nlta = int(nsta), int(nlta)
    if nsta < 1 or nlta < nsta:
        raise ValueError(f"the STA / LTA windows must satisfy 1 <= nsta <= nlta, got nsta={nsta}, nlta={nlta}")
    if nlta > STATIC_MAX_NLTA:
        raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"long windows of up to {STATIC_MAX_NLTA} samples are supported, got {nlta}")
    return nsta, nlta


def _static_pick(win, n):
    win, n = int(win), int(n)
    if win < 1 or n < 1:
        raise ValueError(f"the search window and the number of amplitudes must be at least 1, got win={win}, n={n}")
    if win > STATIC_MAX_WIN:
        raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"search windows of up to +- {STATIC_MAX_WIN} samples are supported, got {win}")
    if n > 2 * win + 1:
        raise UnsupportedError(P3D_ERR_UNSUPPORTED, f"a window of {2 * win + 1} samples cannot give {n} amplitudes")
    return win, n


def _static_section(section):
    section = np.ascontiguousarray(section, dtype=np.float32)
    if section.ndim != 2 or section.size == 0:
        raise ValueError("section is [ntraces][nsamples]")
    return section


def _static_slice(ns, nvalid):
    """(padded, nvalid) as the library takes them; ``nvalid`` None: the whole trace."""
    if nvalid is None:
        return 0, int(ns)
    if not 1 <= int(nvalid) <= ns:
        raise ValueError(f"{nvalid} valid samples do not fit traces of {ns} samples")
    return 1, int(nvalid)


def static_scan_dev(section, ntr, ns, first, device=0):
    """p3d_static_scan_dev on device pointers: ``first`` receives int32 [ntr], the first non-zero sample of every trace (-1: none)."""
    check(lib().p3d_static_scan_dev(int(device), section, int(ntr), int(ns), first))


def static_stalta_max_dev(section, ntr, ns, first, nsta, nlta, peak, nvalid=None, device=0):
    """p3d_static_stalta_max_dev: ``peak`` receives float64 [ntr], the largest STA/LTA ratio of rows nlta ... 2 nlta - 1 of every live trace."""
    nsta, nlta = _static_windows(nsta, nlta)
    padded, nvalid = _static_slice(ns, nvalid)
    check(lib().p3d_static_stalta_max_dev(int(device), section, int(ntr), int(ns), first, padded, nvalid, nsta, nlta, peak))


def static_stalta_cross_dev(section, ntr, ns, first, nsta, nlta, threshold, cross, nvalid=None, device=0):
    """p3d_static_stalta_cross_dev: ``cross`` receives int32 [ntr], the first row of the valid slice whose ratio exceeds ``threshold``."""
    nsta, nlta = _static_windows(nsta, nlta)
    padded, nvalid = _static_slice(ns, nvalid)
    check(lib().p3d_static_stalta_cross_dev(int(device), section, int(ntr), int(ns), first, padded, nvalid, nsta, nlta, float(threshold), cross))


def static_peak_dev(section, ntr, ns, first, base, win, n, out, nvalid=None, device=0):
    """p3d_static_peak_dev: ``out`` receives int32 [ntr], the picked row of the valid slice (-1 for zero traces)."""
    win, n = _static_pick(win, n)
    padded, nvalid = _static_slice(ns, nvalid)
    check(lib().p3d_static_peak_dev(int(device), section, int(ntr), int(ns), first, padded, nvalid, base, win, n, out))


def static_shift_dev(section, ntr, ns, shift, out, device=0):
    """p3d_static_shift_dev: out[x][t] = section[x][t - shift[x]] or 0; all device pointers, ``out`` another buffer than ``section``."""
    check(lib().p3d_static_shift_dev(int(device), section, int(ntr), int(ns), shift, out))


def static_detect(section, nsta, nlta, threshold=None, nvalid=None, device=0):
    """Trace scan and both STA/LTA passes on a host section [ntr][ns] (p3d_static_detect).  Returns ``(first, threshold, cross)``: int32
    [ntr] first non-zero sample (-1: zero trace), the threshold used (the one given, or the largest ratio of rows nlta ... 2 nlta - 1
    over the live traces), int32 [ntr] first row of the valid slice whose ratio exceeds it."""
    nsta, nlta = _static_windows(nsta, nlta)
    section = _static_section(section)
    ntr, ns = section.shape
    padded, nvalid = _static_slice(ns, nvalid)
    thr = C.c_double(float("nan") if threshold is None else float(threshold))
    first, cross = np.empty(ntr, np.int32), np.empty(ntr, np.int32)
    check(lib().p3d_static_detect(int(device), _ptr(section), ntr, ns, padded, nvalid, nsta, nlta, C.byref(thr), _ptr(first), _ptr(cross)))
    return first, thr.value, cross


def static_peak(section, first, base, win, n, nvalid=None, device=0):
    """The peak pick on a host section [ntr][ns] (p3d_static_peak); ``first`` as `static_detect` returns it, ``base`` int32 [ntr] rows of the
    valid slice.  Returns int32 [ntr] (-1 for zero traces)."""
    win, n = _static_pick(win, n)
    section = _static_section(section)
    ntr, ns = section.shape
    padded, nvalid = _static_slice(ns, nvalid)
    first = np.ascontiguousarray(first, dtype=np.int32)
    base = np.ascontiguousarray(base, dtype=np.int32)
    if first.shape != (ntr,) or base.shape != (ntr,):
        raise ValueError("one value per trace")
    out = np.empty(ntr, np.int32)
    check(lib().p3d_static_peak(int(device), _ptr(section), ntr, ns, _ptr(first), padded, nvalid, _ptr(base), win, n, _ptr(out)))
    return out


def static_shift(section, shift, device=0):
    """Shift the traces of a host section [ntr][ns] by ``shift`` samples each (p3d_static_shift); returns the new section."""
    section = _static_section(section)
    shift = np.ascontiguousarray(shift, dtype=np.int32)
    if shift.shape != (section.shape[0],):
        raise ValueError("one shift per trace")
    out = np.empty_like(section)
    check(lib().p3d_static_shift(int(device), _ptr(section), section.shape[0], section.shape[1], _ptr(shift), _ptr(out)))
    return out


# ---- steps 3 and 4: DelayRecordingTime correction and padding (include/p3d.h, p3d_delrt.hip) ------------------------
def _delrt_window(n_traces, n_samples):
    n_traces, n_samples = int(n_traces), int(n_samples)
    if n_traces < 1 or n_samples < 1:
        raise ValueError(f"the comparison window needs at least 1 trace to either side and 1 sample, got n_traces={n_traces}, n_samples={n_samples}")
    return n_traces, n_samples


def delrt_pad_dev(section, ntr, ns_in, ns_out, top, out, device=0):
    """p3d_delrt_pad_dev on device pointers: out[x][t] = section[x][t - top[x]] or 0, ``out`` [ntr][ns_out] another buffer than ``section``
    [ntr][ns_in], ``top`` int32 [ntr] with 0 <= top[x] <= ns_out - ns_in (else the library refuses before it launches anything)."""
    check(lib().p3d_delrt_pad_dev(int(device), section, int(ntr), int(ns_in), int(ns_out), top, out))


def delrt_pad(section, top, ns_out, device=0):
    """Zero-pad the traces of a host section [ntr][ns_in] to ``ns_out`` samples, trace x behind ``top[x]`` zeros (p3d_delrt_pad)."""
    section = _static_section(section)
    top = np.ascontiguousarray(top, dtype=np.int32)
    if top.shape != (section.shape[0],):
        raise ValueError("one top padding per trace")
    ns_out = int(ns_out)
    if ns_out < 1:
        raise ValueError(f"padded traces of {ns_out} samples")
    out = np.empty((section.shape[0], ns_out), np.float32)
    check(lib().p3d_delrt_pad(int(device), _ptr(section), section.shape[0], section.shape[1], ns_out, _ptr(top), _ptr(out)))
    return out


def delrt_windows_dev(section, ntr, ns, ref, n_traces, n_samples, peak_idx, peak_val, maxima, device=0):
    """p3d_delrt_windows_dev: ``section`` and the three results are device pointers (int32 [m], float32 [m], float32 [m][2 n_traces + 1]),
    ``ref`` a HOST array of the m reference-trace indices."""
    n_traces, n_samples = _delrt_window(n_traces, n_samples)
    ref = np.ascontiguousarray(ref, dtype=np.int32).ravel()
    check(lib().p3d_delrt_windows_dev(int(device), section, int(ntr), int(ns), _ptr(ref), ref.size, n_traces, n_samples, peak_idx, peak_val, maxima))


def delrt_windows(subsets, n_samples, device=0):
    """Peak and window maxima of the packed subsets [m][2 n_traces + 1][ns] of m delay changes (p3d_delrt_windows).  Returns ``(peak_idx,
    peak_val, maxima)``: int32 [m] first row of the maximum of every reference trace (the middle one), float32 [m] that maximum, float32
    [m][2 n_traces + 1] the maxima of all traces within n_samples // 2 rows of it."""
    subsets = np.ascontiguousarray(subsets, dtype=np.float32)
    if subsets.ndim != 3 or subsets.shape[1] % 2 != 1 or subsets.shape[1] < 3 or subsets.shape[2] < 1:
        raise ValueError("subsets are [nchanges][2 n_traces + 1][nsamples]")
    m, width, ns = subsets.shape
    n_traces, n_samples = _delrt_window(width // 2, n_samples)
    peak_idx, peak_val, maxima = np.empty(m, np.int32), np.empty(m, np.float32), np.empty((m, width), np.float32)
    check(lib().p3d_delrt_windows(int(device), _ptr(subsets), m, ns, n_traces, n_samples, _ptr(peak_idx), _ptr(peak_val), _ptr(maxima)))
    return peak_idx, peak_val, maxima


# ---- steps 9 and 16: SEG-Y records <-> float32 sections (include/p3d.h, p3d_segy.hip) -------------------------------
SEGY_LAYOUT = {"trace": 0, "slice": 1}
SEGY_SAMPLE_BYTES = {1: 4, 2: 4, 3: 2, 5: 4, 8: 1}


def _segy_table(rows, width):
    """A small HOST table of header words as int32 [n][width]; an empty one for no rows."""
    table = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, width)
    return table, table.shape[0]


def segy_encode_dev(section, ntr, ns, layout, fmt, template, columns, values, records, device=0):
    """p3d_segy_encode_dev on device pointers: ``section`` float32 [ntr][ns] (``layout`` 'trace') or [ns][ntr] ('slice'), ``template`` 240 bytes,
    ``values`` int32 [ncol][ntr], ``records`` ntr x (240 + 4 ns) bytes; ``columns`` a HOST table of (byte offset, width 2 | 4)."""
    columns, ncol = _segy_table(columns, 2)
    check(lib().p3d_segy_encode_dev(int(device), section, int(ntr), int(ns), SEGY_LAYOUT[layout], int(fmt), template, _ptr(columns), ncol, values, records))


def segy_encode(section, layout, fmt, template, columns, values, device=0):
    """SEG-Y records uint8 [ntr][240 + 4 ns] of a host section, float32 [ntr][ns] (``layout`` 'trace') or [ns][ntr] ('slice'), in sample format 1
    (IBM) or 5 (IEEE): every header is ``template`` (240 bytes) overlaid with ``values[c][x]`` as a big-endian word of ``columns[c]`` = (byte
    offset, width 2 | 4) (p3d_segy_encode)."""
    section = np.ascontiguousarray(section, dtype=np.float32)
    if section.ndim != 2:
        raise ValueError("the section is [ntraces][nsamples] or [nsamples][ntraces]")
    ntr, ns = section.shape if SEGY_LAYOUT[layout] == 0 else section.shape[::-1]
    template = np.ascontiguousarray(template, dtype=np.uint8)
    if template.shape != (240,):
        raise ValueError("the header template holds 240 bytes")
    columns, ncol = _segy_table(columns, 2)
    values = np.ascontiguousarray(values, dtype=np.int32)
    if values.size != ncol * ntr:
        raise ValueError(f"{ncol} columns of {ntr} traces but {values.size} values")
    records = np.empty((ntr, 240 + 4 * max(ns, 0)), np.uint8)
    check(lib().p3d_segy_encode(int(device), _ptr(section), ntr, ns, SEGY_LAYOUT[layout], int(fmt), _ptr(template), _ptr(columns), ncol, _ptr(values),
                                _ptr(records)))
    return records


def segy_decode_dev(records, ntr, ns, fmt, fields, samples, words, device=0):
    """p3d_segy_decode_dev on device pointers: ``records`` ntr x (240 + ns x bytes(fmt)) bytes, ``samples`` float32 [ntr][ns], ``words`` int32
    [nfields][ntr]; ``fields`` a HOST table of (byte offset, width 2 | 4, signed)."""
    fields, nf = _segy_table(fields, 3)
    check(lib().p3d_segy_decode_dev(int(device), records, int(ntr), int(ns), int(fmt), _ptr(fields), nf, samples, words))


def segy_decode(records, ns, fmt, fields, device=0):
    """``(samples float32 [ntr][ns], words int32 [nfields][ntr])`` of host records uint8 [ntr][240 + ns x bytes(fmt)] in sample format 1, 2, 3, 5
    or 8; ``fields``: (byte offset, width 2 | 4, signed) of the header words to scrape (p3d_segy_decode)."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    ns, fmt = int(ns), int(fmt)
    reclen = 240 + max(ns, 0) * SEGY_SAMPLE_BYTES.get(fmt, 4)
    if records.ndim != 2 or records.shape[1] != reclen:
        raise ValueError(f"records are [ntraces][{reclen}] bytes for {ns} samples of format {fmt}")
    ntr = records.shape[0]
    fields, nf = _segy_table(fields, 3)
    samples, words = np.empty((ntr, max(ns, 0)), np.float32), np.empty((nf, ntr), np.int32)
    check(lib().p3d_segy_decode(int(device), _ptr(records), ntr, ns, fmt, _ptr(fields), nf, _ptr(samples), _ptr(words)))
    return samples, words


# ---- step 1: merging SEG-Y records (include/p3d.h, p3d_merge.hip) ---------------------------------------------------
def _merge_plan(src, lo_row, hi_row):
    """The three HOST tables of a merge plan as int32 [nout]."""
    src, lo_row, hi_row = (np.ascontiguousarray(t, dtype=np.int32).ravel() for t in (src, lo_row, hi_row))
    if not src.size == lo_row.size == hi_row.size:
        raise ValueError(f"plan tables of {src.size}, {lo_row.size} and {hi_row.size} rows")
    return src, lo_row, hi_row


def merge_keys_dev(records, n, reclen, tracl, fp_full, fp_sub, device=0):
    """p3d_merge_keys_dev on device pointers: ``records`` n x reclen bytes, ``tracl`` int32 [n], ``fp_full`` / ``fp_sub`` uint64 [n]."""
    check(lib().p3d_merge_keys_dev(int(device), records, int(n), int(reclen), tracl, fp_full, fp_sub))


def merge_keys(records, device=0):
    """``(tracl int32 [n], fp_full uint64 [n], fp_sub uint64 [n])`` of host records uint8 [n][reclen]: TRACE_SEQUENCE_LINE and the fingerprints of
    the 240 header bytes with and without bytes 5-8 (p3d_merge_keys)."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    if records.ndim != 2:
        raise ValueError("records are [nrecords][reclen] bytes")
    n, reclen = records.shape
    tracl, fp_full, fp_sub = np.empty(n, np.int32), np.empty(n, np.uint64), np.empty(n, np.uint64)
    check(lib().p3d_merge_keys(int(device), _ptr(records), n, reclen, _ptr(tracl), _ptr(fp_full), _ptr(fp_sub)))
    return tracl, fp_full, fp_sub


def merge_records_dev(records, nsrc, reclen, src, lo_row, hi_row, out, device=0):
    """p3d_merge_records_dev: ``records`` (nsrc x reclen bytes) and ``out`` (len(src) x reclen bytes) are device pointers, the plan ``src``,
    ``lo_row``, ``hi_row`` are HOST tables."""
    src, lo_row, hi_row = _merge_plan(src, lo_row, hi_row)
    check(lib().p3d_merge_records_dev(int(device), records, int(nsrc), int(reclen), src.size, _ptr(src), _ptr(lo_row), _ptr(hi_row), out))


def merge_records(records, src, lo_row, hi_row, device=0):
    """Output records uint8 [len(src)][reclen] of host records uint8 [nsrc][reclen]: row r is record ``src[r]`` with TRACE_SEQUENCE_FILE = r + 1,
    or for ``src[r]`` = -1 a gap trace whose header words are interpolated between rows ``lo_row[r]`` and ``hi_row[r]`` (p3d_merge_records)."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    if records.ndim != 2:
        raise ValueError("records are [nrecords][reclen] bytes")
    src, lo_row, hi_row = _merge_plan(src, lo_row, hi_row)
    out = np.empty((src.size, records.shape[1]), np.uint8)
    check(lib().p3d_merge_records(int(device), _ptr(records), records.shape[0], records.shape[1], src.size, _ptr(src), _ptr(lo_row), _ptr(hi_row), _ptr(out)))
    return out


# ---- step 2: reprojection of header coordinates (include/p3d.h, p3d_proj.hip) --------------------------------------
def _tmerc_prm(prm):
    prm = np.ascontiguousarray(prm, dtype=np.float64)
    if prm.shape != (7,):
        raise ValueError("projection parameters are (a, f, lon0_deg, lat0_deg, k0, x0, y0)")
    return prm


def proj_tmerc_dev(x, y, n, prm, inverse, out_x, out_y, device=0):
    """p3d_proj_tmerc_dev on device pointers to ``n`` float64 values each: forward (``inverse`` False: longitude / latitude in degrees ->
    easting / northing) or inverse transverse Mercator with ``prm`` = (a, f, lon0_deg, lat0_deg, k0, x0, y0).  ``out_x`` may be ``x`` and
    ``out_y`` may be ``y``."""
    prm = _tmerc_prm(prm)
    check(lib().p3d_proj_tmerc_dev(int(device), x, y, int(n), _ptr(prm), int(bool(inverse)), out_x, out_y))


def proj_tmerc(x, y, prm, inverse=False, device=0):
    """Forward or inverse transverse Mercator of host arrays (p3d_proj_tmerc).  Returns two float64 arrays of the inputs' shape."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError(f"x {x.shape} and y {y.shape} differ in shape")
    prm = _tmerc_prm(prm)
    ox, oy = np.empty_like(x), np.empty_like(y)
    check(lib().p3d_proj_tmerc(int(device), _ptr(x), _ptr(y), x.size, _ptr(prm), int(bool(inverse)), _ptr(ox), _ptr(oy)))
    return ox, oy


def proj_smooth_dev(padded, n, w, out, device=0):
    """p3d_proj_smooth_dev: ``padded`` (n + len(w) - 1 float64) and ``out`` (n float64) are device pointers, ``w`` a HOST array of weights;
    out = np.convolve(padded, w, 'valid')."""
    w = np.ascontiguousarray(w, dtype=np.float64).ravel()
    if w.size < 1:
        raise ValueError("an empty window")
    check(lib().p3d_proj_smooth_dev(int(device), padded, int(n), _ptr(w), w.size, out))


def proj_smooth(padded, w, device=0):
    """np.convolve(padded, w, 'valid') of a host signal on the device (len(padded) >= len(w) >= 1), in double."""
    padded, w = np.ascontiguousarray(padded, dtype=np.float64).ravel(), np.ascontiguousarray(w, dtype=np.float64).ravel()
    n = padded.size - w.size + 1
    if w.size < 1 or n < 1:
        raise ValueError(f"a signal of {padded.size} samples and a window of {w.size}")
    din, dout = DeviceArray((padded.size,), np.float64, device), DeviceArray((n,), np.float64, device)
    try:
        din.upload(padded)
        proj_smooth_dev(din.ptr, n, w, dout.ptr, device)
        return dout.download()
    finally:
        din.free()
        dout.free()


# ---- step 6: harmonic tide prediction (include/p3d.h, p3d_tide.hip) ------------------------------------------------
def _tide_small(grid, ids, nc):
    grid, ids = np.ascontiguousarray(grid, dtype=np.float64), np.ascontiguousarray(ids, dtype=np.int32)
    if grid.shape != (4,):
        raise ValueError("the grid numbers are (lon0, dlon, lat0, dlat)")
    if ids.shape != (nc,):
        raise ValueError(f"{nc} table planes but constituent ids of shape {ids.shape}")
    return grid, ids


def tide_predict_dev(lon, lat, t, n, hre, him, wet, nc, nxs, nys, grid, ids, out, device=0):
    """p3d_tide_predict_dev: ``lon``, ``lat``, ``t`` (n float64 each), the tables ``hre`` / ``him`` (int32 [nc][nxs][nys]) and ``wet`` (uint8
    [nxs][nys]) and the result ``out`` (n float64) are device pointers; ``grid`` = (lon0, dlon, lat0, dlat) and ``ids`` [nc] are HOST arrays."""
    grid, ids = _tide_small(grid, ids, int(nc))
    check(lib().p3d_tide_predict_dev(int(device), lon, lat, t, int(n), hre, him, wet, int(nc), int(nxs), int(nys), _ptr(grid), _ptr(ids), out))


def tide_predict(lon, lat, t, hre, him, wet, grid, ids, device=0):
    """Tide in metres at host points (p3d_tide_predict): ``lon`` / ``lat`` in degrees (longitudes on the subset's axis), ``t`` in seconds since
    1992-01-01T00:00:00, the subset tables ``hre`` / ``him`` int32 [nc][nxs][nys] in millimetres and ``wet`` uint8 [nxs][nys], ``grid`` =
    (lon0, dlon, lat0, dlat), ``ids`` [nc] constituent ids (positions in ``functions.tide_model.CONSTITUENTS``).  Returns float64 of the points' shape."""
    lon, lat, t = (np.ascontiguousarray(v, dtype=np.float64) for v in (lon, lat, t))
    if not lon.shape == lat.shape == t.shape:
        raise ValueError(f"lon {lon.shape}, lat {lat.shape} and t {t.shape} differ in shape")
    hre, him, wet = np.ascontiguousarray(hre, dtype=np.int32), np.ascontiguousarray(him, dtype=np.int32), np.ascontiguousarray(wet, dtype=np.uint8)
    if hre.ndim != 3 or him.shape != hre.shape or wet.shape != hre.shape[1:]:
        raise ValueError(f"tables are hre / him [nc][nxs][nys] and wet [nxs][nys], got {hre.shape}, {him.shape}, {wet.shape}")
    nc, nxs, nys = hre.shape
    grid, ids = _tide_small(grid, ids, nc)
    out = np.empty_like(lon)
    check(lib().p3d_tide_predict(int(device), _ptr(lon), _ptr(lat), _ptr(t), lon.size, _ptr(hre), _ptr(him), _ptr(wet), nc, nxs, nys, _ptr(grid),
                                 _ptr(ids), _ptr(out)))
    return out


# ---- step 7: mistie correction (include/p3d.h, p3d_mistie.hip) ---------------------------------------------------
MISTIE_LDS_SAMPLES = 8064    # P3D_MISTIE_LDS_SAMPLES of include/p3d.h
MISTIE_PATH = {"auto": 0, "lds": 1, "global": 2}
MISTIE_OK, MISTIE_EMPTY, MISTIE_LENGTHS, MISTIE_RANGE = 0, 1, 2, 3
MISTIE_HIT = np.dtype([("pair", np.int32), ("seg_i", np.int32), ("seg_j", np.int32), ("part", np.int32), ("x", np.float64), ("y", np.float64)])


def _mistie_lines(xy, line_off):
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    line_off = np.ascontiguousarray(line_off, dtype=np.int64)
    if line_off.ndim != 1 or line_off.size < 2 or line_off[0] != 0 or line_off[-1] != xy.shape[0] or np.any(np.diff(line_off) < 0):
        raise ValueError("line_off holds nlines + 1 ascending vertex offsets from 0 to the number of vertices")
    return xy, line_off


def _mistie_pairs(pairs, nlines):
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= nlines or np.any(pairs[:, 0] >= pairs[:, 1])):
        raise ValueError(f"line pairs are (i, j) with 0 <= i < j < {nlines}")
    return pairs


def mistie_cross_dev(xy, line_off, pairs, hits, capacity, device=0):
    """p3d_mistie_cross_dev: ``xy`` and ``hits`` (``capacity`` records of `MISTIE_HIT`) are device pointers, ``line_off`` / ``pairs`` host arrays.
    Returns the number of hits found (more than ``capacity``: only that many were stored); the records come in no defined order."""
    line_off = np.ascontiguousarray(line_off, dtype=np.int64)
    pairs = _mistie_pairs(pairs, line_off.size - 1)
    needed = C.c_size_t(0)
    check(lib().p3d_mistie_cross_dev(int(device), xy, _ptr(line_off), line_off.size - 1, _ptr(pairs), pairs.shape[0], hits, int(capacity), C.byref(needed)))
    return needed.value


def mistie_cross(xy, line_off, pairs, capacity=None, device=0):
    """Every point at which a segment of line i meets one of line j for the (i, j) of ``pairs`` (p3d_mistie_cross), as a `MISTIE_HIT` record array
    sorted by (pair, seg_i, seg_j, part), without the repeats of one point within a pair (a crossing through a shared vertex of consecutive
    segments is found once per segment).  ``capacity``: records of the first attempt (default: 4 per pair, at least 1024); when more are
    found the call is repeated ONCE with the number the first attempt reports."""
    xy, line_off = _mistie_lines(xy, line_off)
    pairs = _mistie_pairs(pairs, line_off.size - 1)
    cap = max(1024, 4 * pairs.shape[0]) if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("capacity must not be negative")
    needed = C.c_size_t(0)
    for _ in range(2):
        hits = np.zeros(max(cap, 1), MISTIE_HIT)
        check(lib().p3d_mistie_cross(int(device), _ptr(xy), _ptr(line_off), line_off.size - 1, _ptr(pairs), pairs.shape[0], _ptr(hits), cap, C.byref(needed)))
        if needed.value <= cap:
            break
        cap = needed.value
    else:
        raise P3DError(P3D_ERR_INVALID, f"the second attempt found {needed.value} hits, the first had reported {cap}")
    hits = hits[:needed.value]
    hits = hits[np.lexsort((hits["part"], hits["seg_j"], hits["seg_i"], hits["pair"]))]
    keep = np.ones(hits.size, bool)
    seen = set()
    for k, h in enumerate(hits):                                  # first occurrence of a point within its pair
        key = (int(h["pair"]), float(h["x"]), float(h["y"]))
        keep[k] = key not in seen
        seen.add(key)
    return hits[keep]


def mistie_nearest_dev(xy, line_off, points, lines, ncross, index, dist, device=0):
    """p3d_mistie_nearest_dev: device pointers but ``line_off`` (host); ``index`` int32 [ncross][2], ``dist`` float64 [ncross][2]."""
    line_off = np.ascontiguousarray(line_off, dtype=np.int64)
    check(lib().p3d_mistie_nearest_dev(int(device), xy, _ptr(line_off), line_off.size - 1, points, lines, int(ncross), index, dist))


def mistie_nearest(xy, line_off, points, lines, device=0):
    """For every crossing ``points[c]`` and both of its lines ``lines[c]``: (index int32 [k][2], distance float64 [k][2]) of the nearest vertex,
    the first minimum over the whole line (p3d_mistie_nearest)."""
    xy, line_off = _mistie_lines(xy, line_off)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    lines = np.ascontiguousarray(lines, dtype=np.int32).reshape(-1, 2)
    if lines.shape != points.shape:
        raise ValueError("one pair of lines per crossing")
    if lines.size and (lines.min() < 0 or lines.max() >= line_off.size - 1):
        raise ValueError(f"line numbers run from 0 to {line_off.size - 2}")
    index, dist = np.empty(lines.shape, np.int32), np.empty(lines.shape, np.float64)
    check(lib().p3d_mistie_nearest(int(device), _ptr(xy), _ptr(line_off), line_off.size - 1, _ptr(points), _ptr(lines), points.shape[0], _ptr(index),
                                   _ptr(dist)))
    return index, dist


def mistie_xcorr_dev(a, b, ncross, ns, ranges, max_len, shift, coeff, n, status, path="auto", work=None, device=0):
    """p3d_mistie_xcorr_dev on device pointers (``work``: [ncross][2][ns] floats for the global-memory form, None: allocated)."""
    check(lib().p3d_mistie_xcorr_dev(int(device), a, b, int(ncross), int(ns), ranges, int(max_len), MISTIE_PATH[path], work, shift, coeff, n, status))


def mistie_xcorr(a, b, ranges, path="auto", device=0):
    """Windowed cross-correlation of the trace pairs ``a[c]``, ``b[c]`` (float32 [ncross][ns]) over ``ranges[c] = (a first, a length, b first,
    b length)`` (p3d_mistie_xcorr).  Returns ``(shift int32, coeff float64, n int32, status int32)`` per crossing; see include/p3d.h."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.ndim != 2 or a.shape != b.shape or a.shape[1] < 1:
        raise ValueError("a and b are [ncross][nsamples], of one shape")
    ranges = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 4)
    if ranges.shape[0] != a.shape[0]:
        raise ValueError("one (a first, a length, b first, b length) per crossing")
    if path not in MISTIE_PATH:
        raise ValueError(f"path is one of {sorted(MISTIE_PATH)}")
    k = a.shape[0]
    shift, coeff, n, status = np.zeros(k, np.int32), np.zeros(k, np.float64), np.zeros(k, np.int32), np.zeros(k, np.int32)
    check(lib().p3d_mistie_xcorr(int(device), _ptr(a), _ptr(b), k, a.shape[1], _ptr(ranges), MISTIE_PATH[path], _ptr(shift), _ptr(coeff), _ptr(n),
                                 _ptr(status)))
    return shift, coeff, n, status


def _host_cube(x):
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("expected a cube (nslices, nil, nxl)")
    if np.iscomplexobj(x):
        return np.ascontiguousarray(x, dtype=np.complex64), P3D_C64
    return np.ascontiguousarray(x, dtype=np.float32), P3D_F32


def multi_stats(x, devices):
    """p3d_multi_stats: the statistics of every slice of a host cube, blocks of slices on the listed devices (one process)."""
    xc, dt = _host_cube(x)
    n, nil, nxl = xc.shape
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    st = np.empty((n, STATS_PER_SLICE), np.float64)
    check(lib().p3d_multi_stats(len(dev), _ptr(dev), nil, nxl, _ptr(xc), dt, n, _ptr(st)))
    return st


def multi_run(x, mask, tau, niter, devices, thresh_op="hard", version="regular", eps=0.0, alpha=1.0, active=None):
    """p3d_multi_run: the POCS loop on a host cube, blocks of slices on the listed devices (one process, one thread and one plan
    per entry); ``mask`` (nil, nxl) or, one per slice, (nslices, nil, nxl).  Returns (out, niter_done, sums)."""
    xc, dt = _host_cube(x)
    n, nil, nxl = xc.shape
    m = np.ascontiguousarray(mask, dtype=np.float32)
    if m.shape != (nil, nxl) and m.shape != xc.shape:
        raise ValueError(f"mask shape {m.shape} != {(nil, nxl)}")
    t = _tau_table(tau, (n, niter))
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    prm = Plan._params(niter, thresh_op, version, eps, alpha, False, mask_per_slice=m.ndim == 3)
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    out = np.empty_like(xc)
    done = np.zeros(n, np.int32)
    sums = np.zeros((niter + 1, n), np.float64)
    check(lib().p3d_multi_run(len(dev), _ptr(dev), nil, nxl, _ptr(xc), dt, _ptr(m), _ptr(t), None if act is None else _ptr(act),
                              C.byref(prm), _ptr(out), n, _ptr(done), _ptr(sums)))
    return out, done, sums


# ---- step 11: trace-wise pre-processing on device buffers (include/p3d.h, p3d_pre_*_dev) ----------------------------------------------
GAIN_FLAG = {"bias": 1, "tpow": 2, "epow": 4, "gpow": 8, "agc": 16, "clip": 32, "pclip": 64, "nclip": 128, "qclip": 256, "linear": 512,
             "pgc": 1024, "norm_rms": 2048, "scale": 4096, "norm": 8192}
GAIN_PRM = {"flags": 0, "bias": 1, "gpow": 2, "agc_win": 3, "agc_kind": 4, "agc_sqrt": 5, "clip": 6, "pclip": 7, "nclip": 8, "qclip": 9,
            "scale": 10}
GAIN_NPRM = 11
PRE_CHUNK_TRACES = None     # traces per device chunk of trace_ops (None: as many as half of the free device memory holds)


def _op_len(op, nt):
    """Trace length after one operation of :func:`trace_ops`."""
    kind = op[0]
    if kind == "upfirdn":
        return int(op[5])
    if kind == "spectral":
        return int(op[1])
    return nt


def _run_op(op, device, src, dst, work, nt, ntr, extras):
    kind = op[0]
    if kind == "reduce":
        ref = DeviceArray((ntr,), np.float32, device)
        check(lib().p3d_pre_reduce_dev(device, src, nt, ntr, int(op[1]), ref.ptr))
        check(lib().p3d_dev_memcpy(device, dst, src, 4 * nt * ntr, 2))
        extras.append(ref)
    elif kind == "balance":
        ref = DeviceArray((ntr,), np.float32, device)
        check(lib().p3d_pre_balance_dev(device, src, nt, ntr, int(op[1]), dst, ref.ptr))
        extras.append(ref)
    elif kind == "gain":
        prm = np.ascontiguousarray(op[1], dtype=np.float64)
        curves = None if op[2] is None else np.ascontiguousarray(op[2], dtype=np.float64)
        check(lib().p3d_pre_gain_dev(device, src, nt, ntr, _ptr(prm), None if curves is None else _ptr(curves), dst, work))
    elif kind == "agc":
        check(lib().p3d_agc_dev(device, src, nt, ntr, int(op[1]), AGC_KIND[op[2]], int(bool(op[3])), dst, None))
    elif kind == "filter":
        sos = np.ascontiguousarray(op[1], dtype=np.float64)
        zi = np.ascontiguousarray(op[2], dtype=np.float64)
        check(lib().p3d_pre_sosfiltfilt_dev(device, src, nt, ntr, sos.shape[0], _ptr(sos), _ptr(zi), int(op[3]), dst, work))
    elif kind == "upfirdn":
        h = np.ascontiguousarray(op[1], dtype=np.float64)
        check(lib().p3d_pre_upfirdn_dev(device, src, nt, ntr, _ptr(h), h.size, int(op[2]), int(op[3]), int(op[4]), int(op[5]), dst))
    elif kind == "spectral":
        srci = np.ascontiguousarray(op[2], dtype=np.int32)
        fac = np.ascontiguousarray(op[3], dtype=np.float32)
        check(lib().p3d_pre_spectral_dev(device, src, nt, ntr, int(op[1]), _ptr(srci), _ptr(fac), int(bool(op[4])), float(op[5]), float(op[6]),
                                         dst, work))
    else:
        raise ValueError(f"unknown trace operation {kind!r}")


def trace_ops(x, ops, device=0, chunk_traces=None):
    """Run a chain of step-11 operations along axis 0 of a float32 array [nt][traces...] on the GPU.

    The traces go to the device in chunks (``chunk_traces``, else ``PRE_CHUNK_TRACES``, else as many as half of the free device memory
    holds); every operation of the chain runs on the chunk's device buffers, and the chunk comes back once.  ``ops`` are tuples:
    ``('balance', kind)`` (0 rms, 1 max; its reference amplitudes are returned), ``('reduce', kind)`` (the same amplitudes, data
    unchanged; kind 2: the rms without the 0 -> 1 guard), ``('gain', prm, curves)``, ``('agc', win, kind,
    squared)``, ``('filter', sos, zi, padlen)``, ``('upfirdn', h, up, down, pre_remove, nout)``, ``('spectral', num, src, fac, modulus,
    s1, s2)`` (include/p3d.h).  Returns ``(y, refs)``: y float32 [nt_out][traces...], refs one float32 array [traces...] per balance."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim < 1 or x.size == 0:
        raise ValueError("expected a non-empty array with time on axis 0")
    nt = x.shape[0]
    tshape = x.shape[1:]
    ntr = x.size // nt
    x2 = x.reshape(nt, ntr)
    lens = [nt]
    for op in ops:
        lens.append(_op_len(op, lens[-1]))
    ntmax = max(lens)
    # the filter's extension: float32, or double for a cascade of more than 8 sections (include/p3d.h)
    ext = max([(8 if np.shape(op[1])[0] > 8 else 4) * (ntmax + 2 * int(op[3])) for op in ops if op[0] == "filter"] or [0])
    # per trace: two float buffers, the work buffer (float / filter extension / two complex64 lines)
    work_per_trace = max(4 * ntmax, ext, 8 * 2 * ntmax)
    per_trace = 2 * 4 * ntmax + work_per_trace
    chunk = chunk_traces or PRE_CHUNK_TRACES
    if not chunk:
        free, _ = device_mem_info(device)
        chunk = max(1, (free // 2) // per_trace)
    chunk = int(min(chunk, ntr, 2 ** 31 - 1))   # the entry points take at most 2^31 - 1 traces per call
    y = np.empty((lens[-1], ntr), np.float32)
    nbal = sum(1 for op in ops if op[0] in ("balance", "reduce"))
    refs = [np.empty(ntr, np.float32) for _ in range(nbal)]
    bufs = [DeviceArray((ntmax * chunk,), np.float32, device) for _ in range(2)]
    work = DeviceArray((work_per_trace * chunk // 4,), np.float32, device)
    try:
        for j0 in range(0, ntr, chunk):
            n = min(chunk, ntr - j0)
            piece = np.ascontiguousarray(x2[:, j0:j0 + n])
            check(lib().p3d_dev_memcpy(device, bufs[0].ptr, _ptr(piece), piece.nbytes, 0))
            cur, extras = 0, []
            for op, ln in zip(ops, lens[:-1]):
                _run_op(op, device, bufs[cur].ptr, bufs[1 - cur].ptr, work.ptr, ln, n, extras)
                cur = 1 - cur
            out = np.empty((lens[-1], n), np.float32)
            check(lib().p3d_dev_memcpy(device, _ptr(out), bufs[cur].ptr, out.nbytes, 1))
            y[:, j0:j0 + n] = out
            for r, e in zip(refs, extras):
                r[j0:j0 + n] = e.download()
                e.free()
    finally:
        for b in bufs + [work]:
            b.free()
    return y.reshape((lens[-1],) + tshape), [r.reshape(tshape) for r in refs]


def apply_trace_op(x, axis, op, device=0):
    """One operation of :func:`trace_ops` along ``axis`` of ``x`` (moved to the front on the host and back); float32 result."""
    x = np.asarray(x, dtype=np.float32)
    axis = axis % x.ndim
    xt = np.moveaxis(x, axis, 0) if axis != 0 else x
    y, refs = trace_ops(xt, [op], device=device)
    y = np.moveaxis(y, 0, axis) if axis != 0 else y
    return (y, refs) if op[0] in ("balance", "reduce") else y
