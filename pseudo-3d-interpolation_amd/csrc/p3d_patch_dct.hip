// p3d_patch_dct.hip -- the instantiations of the single-kernel DCT loop of the windowed jobs (p3d_resident_dct_job.hpp) and their launcher: the eight
// window shapes of resident_patch_launch (p3d_patch.hip), hard / soft / garrote.  A unit of its own: patch.o and resident.o keep their code.
#include <hip/hip_runtime.h>

#include "p3d_resident_dct_job.hpp"

namespace p3d {

template <int N1, int N2>
static hipError_t launch_dct_shape(const ResidentDctArgs& a, hipStream_t st)
{
    constexpr size_t lds = resident_dct_lds_bytes<N1, N2>();
    constexpr int T = N1 * N2 / 16;
    // (the attribute is per device and is set at every launch, not latched in a flag: two devices may run the same shape)
#define P3D_RES(OP)                                                                                                        \
    do {                                                                                                                   \
        if (lds > 64 * 1024) {                                                                                             \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(resident_dct_kernel<N1, N2, OP>),       \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                \
            if (e != hipSuccess) return e;                                                                                 \
        }                                                                                                                  \
        resident_dct_kernel<N1, N2, OP><<<a.r.nslices, T, lds, st>>>(a);                                                   \
    } while (0)
    switch (a.r.op) {
        case 0: P3D_RES(0); break;
        case 1: P3D_RES(1); break;
        case 2: P3D_RES(2); break;
        default: return hipErrorInvalidValue;
    }
#undef P3D_RES
    return hipGetLastError();
}

hipError_t resident_dct_patch_launch(int nil, int nxl, const ResidentDctArgs& a, hipStream_t st)
{
    if (a.r.mask_period < 1 || !a.r.bits || !a.fac || a.r.nslices < 1) return hipErrorInvalidValue;
#define P3D_SHAPE(A, B) if (nil == A && nxl == B) return launch_dct_shape<A, B>(a, st)
    P3D_SHAPE(32, 32); P3D_SHAPE(32, 64); P3D_SHAPE(32, 128);
    P3D_SHAPE(64, 32); P3D_SHAPE(64, 64); P3D_SHAPE(64, 128);
    P3D_SHAPE(128, 32); P3D_SHAPE(128, 64);
#undef P3D_SHAPE
    return hipErrorNotSupported;
}

}  // namespace p3d
