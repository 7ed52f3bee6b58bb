// p3d_sortnet.hpp -- the register sorting network shared by the exact medians of step 10 (p3d_binning.hip) and step 8 (p3d_despike.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace p3d {

// ascending bitonic network over N (a power of two) registers: every index is a compile-time constant, so nothing is spilled to scratch
template <int N>
__device__ inline void bitonic(float (&v)[N])
{
#pragma unroll
    for (int k = 2; k <= N; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = v[i], b = v[l];
                    const float lo = fminf(a, b), hi = fmaxf(a, b);
                    const bool up = (i & k) == 0;
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
}

}  // namespace p3d
