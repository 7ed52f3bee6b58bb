// p3d_tile_screen.hpp -- the column pass's empty-tile screen: what one thread contributes to the bound, the threshold the bound is set against
// and the decision.  Host and device (tests/csrc/test_tile_screen_host.cpp runs the same functions against a double-precision transform).
//
// A column of N = A*B points, X[k_a + A*k_b] = sum_b W_N^(b*k) S_b[k_a] with S_b = DFT_A over q of x[b + B*q] (what the first, in-register
// pass of the forward transform leaves in thread b's registers), so for every k
//        |X[k]|  <=  sum_b |S_b[k mod A]|  <=  sum_b max_ka (|Re S_b[k_a]| + |Im S_b[k_a]|)  =:  U.
// If U is below the threshold, no coefficient of the column survives it, and a tile all of whose columns are like that is the all-zero tile the
// pass would have found after two more passes, a threshold and a workgroup vote.
#pragma once

#include "p3d_fft.hpp"

namespace p3d {

// Both sides of the comparison give way by 2^-10.  What that has to cover, in units of U: the kernel's S_b carry a rounding error of about
// 10 eps * sum_q |x[b + B*q]| <= 40 eps * max_ka |S_b[k_a]| (Parseval over the A = 16 outputs: max |S| >= sum |x| / 4), the float sum of the B = 64
// non-negative terms 6 eps, and the coefficients the kernel itself would go on to compute differ from the exact X[k] by a few dozen eps * sum_n |x[n]|
// <= 4 U of the same kind -- together below 2^-14, against 2^-9.  The decisions of the threshold operators near their limits (the rounding of |X|^2,
// of 1 / |X|, the tie rule of the hard threshold) move by a few eps of tau and fall inside the same margin.
constexpr float SCREEN_UP = 1.0009765625f;     // 1 + 2^-10
constexpr float SCREEN_DOWN = 0.9990234375f;   // 1 - 2^-10

// max over a thread's PPT values of |re| + |im| (>= the modulus).  Taken on the bit patterns (non-negative floats order like unsigned integers), so
// that a NaN or an infinity among them comes out on top instead of being dropped the way fmaxf drops a NaN: the sum is then not below any threshold
// and the tile takes the full path, which keeps such a coefficient.
template <int PPT>
P3D_HD float screen_term(const c32 (&v)[PPT])
{
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const float t = __builtin_fabsf(v[q].x) + __builtin_fabsf(v[q].y);
        unsigned b;
        __builtin_memcpy(&b, &t, 4);
        b &= 0x7fffffffu;
        m = b > m ? b : m;
    }
    float r;
    __builtin_memcpy(&r, &m, 4);
    return r;
}

// The modulus below which operator `op` (0 hard, 1 soft, 2 garrote) zeroes a coefficient, up to the margin; 0 or NaN: none is known.  Hard compares |X|
// with Re tau (lexicographically, the tie is inside the margin), soft keeps X when Re(1 - tau / |X|) > 0, garrote when Re(1 - tau^2 / |X|^2) > 0, i.e.
// when |X|^2 > Re(tau)^2 - Im(tau)^2 -- a smaller limit than Re tau as soon as the threshold has an imaginary part.
P3D_HD float screen_threshold(c32 tau, int op)
{
    if (op != 2) return tau.x;
    const float t2 = tau.x * tau.x - tau.y * tau.y;   // (the garrote's own expression)
    return t2 > 0.0f ? __builtin_sqrtf(t2) : 0.0f;
}

// U above this answers nothing: the operators square the modulus (|X|^2 = re^2 + im^2 in float), and a coefficient beyond ~1.8e19 overflows there -- against
// a threshold that is larger still (or infinite) the full path then KEEPS it (inf < inf is false) although its modulus is below the threshold.  With
// U <= 1e18 every |X| <= U (1 + 2^-14) squares to less than 1.1e36, far from the overflow, and the full path zeroes what the bound says it zeroes.
constexpr float SCREEN_U_MAX = 1.0e18f;

// column sum U against the threshold: true = every coefficient of the column is zeroed.  Written so that a NaN on either side answers false.
P3D_HD bool screen_proves_empty(float u, float thr)
{
    return thr > 0.0f && u <= SCREEN_U_MAX && u * SCREEN_UP < thr * SCREEN_DOWN;
}

}  // namespace p3d
