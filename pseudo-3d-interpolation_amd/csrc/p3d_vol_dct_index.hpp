// p3d_vol_dct_index.hpp -- the pure index arithmetic of the axis-0 cosine pass (p3d_vol_dct.hip): the factorisation of n0, the tile width, the LDS size,
// the position <-> coefficient maps of the unpermuted transform and the partner position of the DCT's group step (p3d_dct_tables.hpp).  No HIP call and
// no device state: the kernel and the host share these functions, and tests/csrc/test_vol_dct_index_host.cpp runs them on the CPU.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define P3D_VOLDCT_HD __host__ __device__ inline
#else
#define P3D_VOLDCT_HD inline
#endif

namespace p3d {
namespace voldct {

constexpr int MAX_N0 = 1024;
constexpr int MAX_STAGES = 10;       // 2^10
constexpr int THREADS = 256;
constexpr int STAT = 5;              // doubles per workgroup of the statistics pass: peak (Re, Im), max |X|^2, min |X|^2, sum |X|^2
constexpr int ELEM_BYTES = 8;        // complex64
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

// tile width: 64 positions (rows of 512 B) while the tile stays within 32 KiB -- four workgroups then share a compute unit's LDS --, never below 16 (128 B)
inline int width(int n0)
{
    int w = 64;
    while (w > 16 && (size_t)ELEM_BYTES * (size_t)n0 * w > 32768) w >>= 1;
    return w;
}

// bytes of the position table behind the roots: one 16-bit entry per coefficient, rounded up to whole complex64 elements
inline size_t pos_table_bytes(int n0) { return (((size_t)n0 * 2 + ELEM_BYTES - 1) / ELEM_BYTES) * ELEM_BYTES; }

// dynamic LDS of voldct_z_kernel: the tile [n0][width], the n0 roots and the position table behind it, at least the scratch of the statistics reduction
inline size_t lds_bytes(int n0, int width)
{
    const size_t tile = (size_t)ELEM_BYTES * ((size_t)n0 * width + n0) + pos_table_bytes(n0);
    const size_t scratch = (sizeof(double) + 4 * sizeof(float)) * THREADS;
    return tile > scratch ? tile : scratch;
}

// position p of the transformed column holds coefficient k: p = k_1 n0/r_1 + k_2 n0/(r_1 r_2) + ..., k = k_1 + r_1 k_2 + r_1 r_2 k_3 + ...
P3D_VOLDCT_HD int coef_of_pos(int n0, int nstage, const int* radix, int p)
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

// ... and its inverse: where coefficient k stands
P3D_VOLDCT_HD int pos_of_coef(int n0, int nstage, const int* radix, int k)
{
    int p = 0, M = n0;
    for (int s = 0; s < nstage; ++s) {
        const int r = radix[s], L = M / r, d = k % r;
        k /= r;
        p += d * L;
        M = L;
    }
    return p;
}

// the position of the group partner (n0 - k) mod n0 of the coefficient at position p
P3D_VOLDCT_HD int partner_pos(int n0, int nstage, const int* radix, int p)
{
    const int k = coef_of_pos(n0, nstage, radix, p);
    return pos_of_coef(n0, nstage, radix, k == 0 ? 0 : n0 - k);
}

// sample z of a column goes to row perm(n0, z) (p3d_dct_tables.hpp: even samples ascending, odd samples descending); row p holds sample unperm(n0, p)
P3D_VOLDCT_HD int unperm(int n, int p) { return p < (n + 1) / 2 ? 2 * p : 2 * (n - 1 - p) + 1; }

}  // namespace voldct
}  // namespace p3d
