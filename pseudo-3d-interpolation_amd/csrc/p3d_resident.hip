// p3d_resident.hip -- the whole POCS job of a SMALL slice in one kernel: one workgroup per slice, the slice in registers, every
// transform through LDS, all K iterations without touching HBM.
//
// The reference runs POCS_algorithm once per (iline, xline) slice (pseudo_3D_interpolation/cube_POCS_interpolation_3D.py:314-340,
// functions/POCS.py:549-632); for slices of 32 x 32 ... 128 x 128 points (BASELINE configs[0]: 64 x 64 x 128) the two-pass kernels
// of p3d_kernels.hpp are launch bound (two launches + bookkeeping per iteration for 32 KiB of data per slice).  A slice of
// N1 x N2 <= 16384 points is 16 points per thread of an N1 N2 / 16-thread workgroup, so here
//
//     x_obs, mask bits -> registers (once)                                   POCS.py:549
//     K x { row FFT -> [LDS] -> column FFT -> threshold -> inverse column FFT -> [LDS] -> inverse row FFT
//           -> x = x (1 - alpha mask) + alpha x_obs -> sum |x| -> cost -> early exit }          POCS.py:560-632
//     result -> HBM (once)
//
// HBM traffic per slice: (8 + 8) B/point per JOB instead of per iteration.  Same templates (line_fft, Shrink), same twiddle tables,
// same order of operations and the same reduction order of the cost sums as the two-pass path: results, sums and iteration counts
// are bit-identical to it (tests/test_gpu_parity.py::test_resident_small_slices_equal_the_two_pass_path).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_fft.hpp"
#include "p3d_resident.hpp"
#include "p3d_resident_job.hpp"
#include "p3d_shrink.hpp"

namespace p3d {

template <int N1, int N2>
static hipError_t launch_shape(const ResidentArgs& a, hipStream_t st)
{
    constexpr size_t lds = resident_lds_bytes<N1, N2>();
    constexpr int T = N1 * N2 / 16;
#define P3D_RES(OP)                                                                                                         \
    do {                                                                                                                    \
        if (lds > 64 * 1024) {                                                                                              \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(resident_kernel<N1, N2, OP>),            \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                 \
            if (e != hipSuccess) return e;                                                                                  \
        }                                                                                                                   \
        resident_kernel<N1, N2, OP><<<a.nslices, T, lds, st>>>(a);                                                          \
    } while (0)
    switch (a.op) {
        case 0: P3D_RES(0); break;
        case 1: P3D_RES(1); break;
        case 2: P3D_RES(2); break;
        default: return hipErrorInvalidValue;
    }
#undef P3D_RES
    return hipGetLastError();
}

bool resident_supported(int nil, int nxl)
{
    auto ok = [](int n) { return n == 32 || n == 64 || n == 128; };
    return ok(nil) && ok(nxl);
}

hipError_t resident_launch(int nil, int nxl, const ResidentArgs& a, hipStream_t st)
{
#define P3D_SHAPE(A, B) if (nil == A && nxl == B) return launch_shape<A, B>(a, st)
    P3D_SHAPE(32, 32); P3D_SHAPE(32, 64); P3D_SHAPE(32, 128);
    P3D_SHAPE(64, 32); P3D_SHAPE(64, 64); P3D_SHAPE(64, 128);
    P3D_SHAPE(128, 32); P3D_SHAPE(128, 64); P3D_SHAPE(128, 128);
#undef P3D_SHAPE
    return hipErrorNotSupported;
}

}  // namespace p3d
