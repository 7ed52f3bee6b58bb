// p3d_select64.hpp -- order statistics of double-precision spectra (p3d_select64.hip): np.percentile of |X| per slice for the percentile
// operators of the double-precision FFT loop, and the lexicographically sorted spectrum for the 'data-driven' threshold model.
// The three helpers that are plain C++ -- the order-preserving key of a double, NumPy's interpolation of two order statistics -- are
// defined here for host and device alike (tests/csrc/test_select64_host.cpp drives them on the CPU).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace p3d {
namespace sel64 {

// double -> uint64 whose unsigned order is the order of the doubles (-0.0 is made +0.0 first: NumPy compares them equal), and back
__host__ __device__ inline uint64_t ord64(double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double unord64(uint64_t k)
{
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
// a non-negative double (a modulus) orders like its bit pattern
__host__ __device__ inline uint64_t mod_key(double m) { return __builtin_bit_cast(uint64_t, m); }
__host__ __device__ inline double mod_value(uint64_t k) { return __builtin_bit_cast(double, k); }

// numpy.lib._function_base_impl._lerp: a + (b - a) t, and b - (b - a) (1 - t) for t >= 0.5 (separate roundings: this unit is compiled
// without contraction into fused multiply-adds)
__host__ __device__ inline double lerp64(double a, double b, double t)
{
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// ---- percentile select -------------------------------------------------------------------------------------------------------------
// The state of one select, PCT_WORDS 64-bit words per slice:
//   [0] rank still to find among the keys that share the prefix   [1] the prefix: key bits found so far
//   [2] in: 1 if the upper order statistic is the successor of the lower one (0: the same element)   out: 1 if a successor pass is needed
//   [3] the upper order statistic's key (the successor pass takes a minimum into it)
constexpr int PCT_WORDS = 4;
constexpr int PCT_BINS = 8192;   // 13 bits per level: 13 + 13 + 13 + 13 + 11 = the 63 bits below the sign

// tau[s * niter + iter] = (np.percentile(|spectrum[s]|, .), 0) for every slice with done[s] == 0 (done == NULL: every slice).
// spectrum [nslices][per] complex128; sel [nslices][PCT_WORDS] as above (consumed); frac [nslices] the weight of the upper order
// statistic; hist [nslices][PCT_BINS] all zero (left all zero); mod [nslices][per] scratch for the moduli.  Enqueues on st.
hipError_t percentile64(const void* spectrum, size_t per, int nslices, uint64_t* sel, const double* frac, unsigned* hist, uint64_t* mod, void* tau,
                        int niter, int iter, const int* done, hipStream_t st);

// ---- lexicographic sort ------------------------------------------------------------------------------------------------------------
// spectrum [nslices][per] complex128 is REPLACED by its 128-bit order keys, sorted per slice in descending order (`other`: a second
// buffer of that size, scratch); peaks_dev [nslices][2] the lexicographic maximum of every slice.  `hist`: 16 * tiles * nslices words,
// tiles = sort64_tiles(per).  Enqueues on st.
int sort64_tiles(size_t per);
hipError_t lex_sort_desc64(void* spectrum, void* other, size_t per, int nslices, unsigned* hist, double* peaks_dev, hipStream_t st);

// bounds_dev [nslices][4] = tau_min (re, im), tau_max (re, im) -> count_dev [nslices] = Nv = #{tau_min < X < tau_max},
// tau_dev [nslices][niter][2] = the picks of POCS.py:359-362 (untouched where Nv = 0)
hipError_t data_driven_pick64(const void* sorted, size_t per, int nslices, int niter, const double* bounds_dev, double* tau_dev, long long* count_dev,
                              hipStream_t st);

}  // namespace sel64
}  // namespace p3d
