// p3d_vol64_index.hpp -- the pure index arithmetic of the double-precision axis-0 pass (p3d_vol64.hip): the factorisation of n0, the tile width, the LDS
// size and the position -> coefficient map of the unpermuted transform.  No HIP call and no device state: the
// kernel and the host share these functions, and tests/csrc/test_vol64_index_host.cpp runs them on the CPU.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define P3D_VOL64_HD __host__ __device__ inline
#else
#define P3D_VOL64_HD inline
#endif

namespace p3d {
namespace vol64 {

constexpr int MAX_N0 = 1024;
constexpr int MAX_STAGES = 10;       // 2^10
constexpr int THREADS = 256;
constexpr int STAT = 5;              // doubles per workgroup of the statistics pass: peak (Re, Im), max |X|, min |X|, sum |X|^2
constexpr int ELEM_BYTES = 16;       // complex128
constexpr size_t LDS_LIMIT = 163840; // what one workgroup may declare

// radices of a 7-smooth n (4s first, then 2, 3, 5, 7); n = 1: one stage of radix 1.  Returns the stage count, or -1
inline int factor(int n, int* radix)
{
    if (n < 1 || n > MAX_N0) return -1;
    int ns = 0;
    if (n == 1) { radix[0] = 1; return 1; }
    while (n % 4 == 0) { radix[ns++] = 4; n /= 4; }
    const int rest[4] = {2, 3, 5, 7};
    for (int r : rest)
        while (n % r == 0) { radix[ns++] = r; n /= r; }
    return n == 1 ? ns : -1;
}

// tile width: the largest of 32, 16, 8 positions (rows of 512, 256, 128 B) whose tile stays within 32 KiB -- four workgroups then share a compute unit's
// LDS --, never below 8 (a 128-B row)
inline int width(int n0)
{
    int w = 32;
    while (w > 8 && (size_t)ELEM_BYTES * (size_t)n0 * w > 32768) w >>= 1;
    return w;
}

// dynamic LDS of vol64_z_kernel: the tile [n0][width] and the n0 roots behind it, at least the scratch of the statistics reduction
inline size_t lds_bytes(int n0, int width)
{
    const size_t tile = (size_t)ELEM_BYTES * ((size_t)n0 * width + n0), scratch = sizeof(double) * STAT * THREADS;
    return tile > scratch ? tile : scratch;
}

// position p of the transformed column holds coefficient k: p = k_1 n0/r_1 + k_2 n0/(r_1 r_2) + ..., k = k_1 + r_1 k_2 + r_1 r_2 k_3 + ...
P3D_VOL64_HD int coef_of_pos(int n0, int nstage, const int* radix, int p)
{
    int k = 0, mult = 1, M = n0;
    for (int s = 0; s < nstage; ++s) {
        const int r = radix[s], L = M / r, d = p / L;
        p -= d * L;
        k += d * mult;
        mult *= r;
        M = L;
    }
    return k;
}

}  // namespace vol64
}  // namespace p3d
