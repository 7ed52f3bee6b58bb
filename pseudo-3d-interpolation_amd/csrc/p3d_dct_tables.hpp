// p3d_dct_tables.hpp -- index maps and coefficient tables of the DCT-II / DCT-III pair built on the complex FFT (p3d_dct.hip).
// Host and device; no HIP header needed, so a plain C++ program can check it (tests/csrc/test_dct_tables_host.cpp).
//
// Per axis of length N (scipy.fft.dctn / idctn, type 2, norm 'backward' or 'ortho'):
//   reorder   v[perm(i)] = z[i],  perm(2n) = n,  perm(2n + 1) = N - 1 - n
//   V = FFT_N(v)
//   combine   X[k] = fwd[k] * V[k] + conj(fwd[k]) * V[partner(k)],   fwd[k] = s_k * exp(-i pi k / 2N)
//   split     V[k] = inv[k] * (X[k] - i X[partner(k)])  for k > 0,   V[0] = inv[0] * X[0],   inv[k] = exp(+i pi k / 2N) / (2 s_k)
// with s_k = 1 ('backward') or s_0 = sqrt(1/4N), s_k = sqrt(1/2N) ('ortho').  k and partner(k) = (N - k) mod N form a group that both
// directions close over; k = 0 and (N even) k = N/2 are their own partners.  The owners of the groups are k = 0 ... N/2.
#pragma once
#include <cmath>

#include "p3d_fft.hpp"

namespace p3d {
namespace dct {

constexpr int NORM_BACKWARD = 0;   // P3D_DCT_BACKWARD
constexpr int NORM_ORTHO = 1;      // P3D_DCT_ORTHO

P3D_HD int perm(int n, int i) { return (i & 1) ? n - 1 - (i >> 1) : (i >> 1); }
P3D_HD int partner(int n, int k) { return k == 0 ? 0 : n - k; }
P3D_HD int owners(int n) { return n / 2 + 1; }

inline double scale(int n, int k, int norm)
{
    if (norm != NORM_ORTHO) return 1.0;
    return k == 0 ? std::sqrt(1.0 / (4.0 * n)) : std::sqrt(1.0 / (2.0 * n));
}

// fwd[n], inv[n]: evaluated in double, rounded once to the storage type C (c32 for the float32 kernels; a complex of doubles keeps them as they are)
template <class C>
inline void build_tables(int n, int norm, C* fwd, C* inv)
{
    using R = decltype(C::x);
    for (int k = 0; k < n; ++k) {
        const double ang = 3.14159265358979323846264338327950288 * double(k) / (2.0 * double(n));
        const double s = scale(n, k, norm), c = std::cos(ang), sn = std::sin(ang);
        fwd[k] = C{R(s * c), R(-s * sn)};
        inv[k] = C{R(c / (2.0 * s)), R(sn / (2.0 * s))};
    }
}

}  // namespace dct
}  // namespace p3d
