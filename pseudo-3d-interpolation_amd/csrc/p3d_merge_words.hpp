// p3d_merge_words.hpp -- the words of the 240-byte SEG-Y rev-1 trace header as step 1 (p3d_merge.hip) sees them, for the host and the device alike:
// tests/csrc/test_merge_words_host.cpp compiles this file with a plain C++ compiler.
//
// The header is 91 big-endian signed words of 2 or 4 bytes that tile the 240 bytes without a hole (RUNS below: runs of equal width, in order).
// Every word starts at an even byte, but not every 4-byte word at a multiple of 4 (the one at bytes 219-222, counted from 1 as in the standard, does not), so words are read and written
// byte by byte.
//
//   word_at(j)        offset and width of word j = 0 ... 90
//   word_of_byte(i)   the word that holds byte i = 0 ... 239
//   load_be / store_be   a word as a sign-extended int32 / the low 16 or 32 bits of an int32 as a word
//   interp_word       the header word of a gap trace in output row r between the surviving rows a < r < b with words va and vb: what
//                     pandas.DataFrame.interpolate('linear').astype('int32') gives, i.e. np.interp's  slope = (vb - va) / (b - a);
//                     v = slope * (r - a) + va  in IEEE double, in this order and with no fused multiply-add (build with -ffp-contract=off), then
//                     a C cast to int32 (toward zero).  The result lies between va and vb (rounding is monotone), so the cast never overflows.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3D_MERGE_HD __host__ __device__ inline
#define P3D_MERGE_UNROLL _Pragma("unroll")
#else
#define P3D_MERGE_HD inline
#define P3D_MERGE_UNROLL
#endif

namespace p3d_merge {

constexpr int HDR_BYTES = 240;
constexpr int NWORDS = 91;
constexpr int NRUNS = 16;
constexpr int RUN_COUNT[NRUNS] = {7, 4, 8, 2, 4, 46, 5, 2, 1, 5, 1, 1, 1, 1, 1, 2};
constexpr int RUN_WIDTH[NRUNS] = {4, 2, 4, 2, 4, 2, 4, 2, 4, 2, 4, 2, 4, 2, 2, 4};

constexpr int words_before(int run)
{
    int n = 0;
    for (int k = 0; k < run; ++k) n += RUN_COUNT[k];
    return n;
}
constexpr int bytes_before(int run)
{
    int n = 0;
    for (int k = 0; k < run; ++k) n += RUN_COUNT[k] * RUN_WIDTH[k];
    return n;
}
static_assert(words_before(NRUNS) == NWORDS, "the trace header has 91 words");
static_assert(bytes_before(NRUNS) == HDR_BYTES, "the 91 words cover the 240 bytes");

// the loops below run over compile-time constants only: unrolled, they are chains of compares against immediates (no table in memory)
P3D_MERGE_HD void word_at(int j, int& off, int& width)
{
    off = 0;
    width = 0;
    P3D_MERGE_UNROLL
    for (int k = 0; k < NRUNS; ++k) {
        const int first = words_before(k), start = bytes_before(k);
        if (j >= first && j < first + RUN_COUNT[k]) {
            off = start + (j - first) * RUN_WIDTH[k];
            width = RUN_WIDTH[k];
        }
    }
}

P3D_MERGE_HD void word_of_byte(int i, int& off, int& width)
{
    off = 0;
    width = 0;
    P3D_MERGE_UNROLL
    for (int k = 0; k < NRUNS; ++k) {
        const int start = bytes_before(k), len = RUN_COUNT[k] * RUN_WIDTH[k];
        if (i >= start && i < start + len) {
            off = start + ((i - start) & ~(RUN_WIDTH[k] - 1));      // widths are powers of two and a run starts at one of its words
            width = RUN_WIDTH[k];
        }
    }
}

P3D_MERGE_HD int32_t load_be(const unsigned char* p, int width)
{
    const uint32_t hi = ((uint32_t)p[0] << 8) | p[1];
    if (width == 2) return (int32_t)(int16_t)(uint16_t)hi;
    return (int32_t)((hi << 16) | ((uint32_t)p[2] << 8) | p[3]);
}

P3D_MERGE_HD void store_be(unsigned char* p, int width, int32_t v)
{
    const uint32_t u = (uint32_t)v;
    if (width == 2) {
        p[0] = (unsigned char)(u >> 8);
        p[1] = (unsigned char)u;
    } else {
        p[0] = (unsigned char)(u >> 24);
        p[1] = (unsigned char)(u >> 16);
        p[2] = (unsigned char)(u >> 8);
        p[3] = (unsigned char)u;
    }
}

P3D_MERGE_HD int32_t interp_word(int32_t va, int32_t vb, int a, int b, int r)
{
    const double slope = ((double)vb - (double)va) / ((double)b - (double)a);
    const double v = slope * ((double)r - (double)a) + (double)va;
    return (int32_t)v;
}

}  // namespace p3d_merge
