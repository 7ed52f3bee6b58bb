// p3d_segy_codec.hpp -- the word-level conversions of the SEG-Y codec (p3d_segy.hip), in integer arithmetic on the bit patterns, for the host and
// the device alike: tests/csrc/test_segy_codec_host.cpp compiles this file with a plain C++ compiler.
//
// An IBM System/360 single is  (-1)^s * 0.m * 16^(e - 64):  s 1 bit, e 7 bits, m 24 bits (6 hex digits, no hidden bit).  Both functions reproduce
// functions/segy.py bit for bit; that file computes in float64, where every value below is exact, so its only rounding is the one named here.
//
//   ieee2ibm   A finite non-zero float32 is M * 2^(k - 24) with 2^23 <= M < 2^24 (subnormals are shifted up first).  k = 4 e16 - r with
//              r = 0 ... 3 puts the value on a power of 16; the IBM mantissa is M >> r, rounded to nearest, ties to even (np.rint).  With r = 0 the
//              mantissa is M itself, with r >= 1 it is at most 2^23, so the rounding never carries out of the 24 bits; and e16 + 64 runs from 27
//              (2^-149) to 96 (FLT_MAX), so no float32 leaves the IBM range: there is no carry, saturation or flush to code.
//              +-0 and NaN give 0 (the host's `a > 0` holds for neither); +-Inf gives the largest magnitude, 0x7FFFFFFF / 0xFFFFFFFF (the host
//              function is undefined there).
//   ibm2ieee   m * 2^(4 (e - 64) - 24), cast to float32 as NumPy casts a double: exact while the result is a normal float32 (m has 24 bits), rounded
//              to nearest-even where it is a subnormal, +-inf beyond FLT_MAX, and a zero mantissa keeps the sign (-0.0).  Any m, normalised or not.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3D_SEGY_HD __host__ __device__ inline
#else
#define P3D_SEGY_HD inline
#endif

namespace p3d_segy {

// leading zeros of a non-zero 32-bit word
P3D_SEGY_HD int clz32(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)v);
#else
    return __builtin_clz(v);
#endif
}

P3D_SEGY_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

P3D_SEGY_HD uint32_t ieee2ibm(uint32_t f)
{
    const uint32_t sign = f & 0x80000000u, be = (f >> 23) & 0xFFu;
    uint32_t M = f & 0x007FFFFFu;
    if (be == 0xFFu) return M ? 0u : sign | 0x7FFFFFFFu;           // NaN, +-Inf
    int k;                                                         // |x| = M * 2^(k - 24), 2^23 <= M < 2^24
    if (be) {
        M |= 0x00800000u;
        k = (int)be - 126;
    } else {
        if (!M) return 0u;
        const int lz = clz32(M) - 8;
        M <<= lz;
        k = -125 - lz;
    }
    const int e16 = (k + 3) >> 2, r = 4 * e16 - k;                 // arithmetic shift: the ceiling of k / 4 for negative k too
    const uint32_t q = M >> r, rem = M & ((1u << r) - 1u), half = (1u << r) >> 1;
    const uint32_t mant = q + (uint32_t)(r && (rem > half || (rem == half && (q & 1u))));
    return sign | ((uint32_t)(e16 + 64) << 24) | mant;
}

P3D_SEGY_HD uint32_t ibm2ieee(uint32_t w)
{
    const uint32_t sign = w & 0x80000000u, m = w & 0x00FFFFFFu;
    if (!m) return sign;
    const int lz = clz32(m) - 8;
    const uint32_t M = m << lz;                                    // bit 23 set
    const int be = 4 * ((int)((w >> 24) & 0x7Fu) - 64) - 1 - lz + 127;   // biased exponent of M * 2^(4 (e - 64) - 24 - lz)
    if (be >= 255) return sign | 0x7F800000u;
    if (be >= 1) return sign | ((uint32_t)be << 23) | (M & 0x007FFFFFu);
    const int s = 1 - be;                                          // subnormal: M >> s in units of 2^-149, to nearest-even
    if (s > 25) return sign;
    const uint32_t q = M >> s, rem = M & ((1u << s) - 1u), half = 1u << (s - 1);
    return sign | (q + (uint32_t)(rem > half || (rem == half && (q & 1u))));
}

}  // namespace p3d_segy
