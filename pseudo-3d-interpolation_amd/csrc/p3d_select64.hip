// p3d_select64.hip -- order statistics of a slice's DOUBLE-PRECISION spectrum, on the device: what the percentile operators and the
// 'data-driven' threshold model of the double-precision FFT loop (p3d_f64.hip) need.  The float32 loop has both in p3d_generic.hip
// (gen_launch_pct_*) and p3d_select.hip; these are their counterparts on 64-bit moduli and 128-bit lexicographic keys.
//
// 1. np.percentile(|X|, perc) per slice and iteration (POCS.py:43-58): an EXACT radix select on the bit pattern of the non-negative double
//    |X| (it orders like an unsigned integer).  No sampling, no float32 pre-pass.  Passes over a slice of P points, per iteration:
//      pct64_mod_kernel    reads the spectrum (16 P bytes), writes the moduli (8 P bytes), counts the top 13 bits
//      pct64_hist_kernel   x 4: reads the moduli (8 P bytes each), counts the next 13 (last: 11) bits of the keys that share the prefix
//      pct64_scan_kernel   after every count: the bin that holds the rank; the last one also knows how many keys EQUAL the order statistic
//      pct64_succ_kernel   the upper order statistic is the successor of the lower one: the same key if the rank stays inside the run of
//                          equal keys (or the position is an integer), else the smallest key above -- one more read of the moduli (8 P bytes),
//                          skipped per slice on the device where it is not needed
//      pct64_tau_kernel    NumPy's interpolation of the two, with a double weight, into the loop's device-side tau
//    = 56 P bytes (64 P with the successor pass) per iteration.  Counting goes through a histogram in LDS (32 KiB per workgroup, LDS atomics:
//    lanes of a wavefront that hit the same bin are serialised by the LDS, at most 64 deep; a spectrum's moduli share a few exponents, so the
//    first level is the slow one), flushed to memory with one atomic per non-empty bin and workgroup.
// 2. the spectrum sorted in NumPy's complex order (real part, then imaginary part; -0.0 == +0.0) for POCS.py:356-362: (re, im) -> a 128-bit
//    key whose unsigned order is that order, sorted per slice by the segmented least-significant-digit radix sort of p3d_select.hip with a
//    two-word key: thirty-two 4-bit passes of histogram / scan / stable scatter.  Once per job, off the iteration loop: clarity over speed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_select64.hpp"

namespace p3d {
namespace sel64 {

namespace {

// ---- percentile select ---------------------------------------------------------------------------------------------------------------------
constexpr int PCT_LEVELS = 5, PCT_T = 256;
__host__ __device__ constexpr int pct_shift(int level) { return level == 4 ? 0 : 50 - 13 * level; }
__host__ __device__ constexpr int pct_bits(int level) { return level == 4 ? 11 : 13; }

__device__ __forceinline__ void pct_flush(const unsigned* h, unsigned* hist)
{
    for (int i = threadIdx.x; i < PCT_BINS; i += blockDim.x)
        if (h[i] != 0u) atomicAdd(&hist[i], h[i]);
}

// level 0: the moduli of the spectrum -> mod, the top 13 bits of their keys (sign, exponent, first mantissa bit) counted
__global__ __launch_bounds__(PCT_T) void pct64_mod_kernel(const double2* w, uint64_t* mod, size_t per, unsigned* hist, const int* done)
{
    __shared__ unsigned h[PCT_BINS];
    const int s = blockIdx.y;
    if (done && done[s] != 0) return;
    for (int i = threadIdx.x; i < PCT_BINS; i += blockDim.x) h[i] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
        const double2 v = w[(size_t)s * per + i];
        const uint64_t key = mod_key(hypot(v.x, v.y));   // np.absolute; the modulus the threshold operators compare (shrink64)
        mod[(size_t)s * per + i] = key;
        atomicAdd(&h[(unsigned)(key >> pct_shift(0)) & (PCT_BINS - 1)], 1u);
    }
    __syncthreads();
    pct_flush(h, hist + (size_t)s * PCT_BINS);
}

// levels 1 .. 4: the keys that share the prefix found so far, counted by their next digit
__global__ __launch_bounds__(PCT_T) void pct64_hist_kernel(const uint64_t* mod, size_t per, const uint64_t* sel, unsigned* hist, int level, const int* done)
{
    __shared__ unsigned h[PCT_BINS];
    const int s = blockIdx.y;
    if (done && done[s] != 0) return;
    const int shift = pct_shift(level), bits = pct_bits(level);
    const uint64_t prefix = sel[(size_t)s * PCT_WORDS + 1], pmask = ~0ull << (shift + bits);
    for (int i = threadIdx.x; i < PCT_BINS; i += blockDim.x) h[i] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t key = mod[(size_t)s * per + i];
        if ((key & pmask) == prefix) atomicAdd(&h[(unsigned)(key >> shift) & ((1u << bits) - 1u)], 1u);
    }
    __syncthreads();
    pct_flush(h, hist + (size_t)s * PCT_BINS);
}

// one workgroup per slice: thread t adds bins [32 t, 32 t + 32), thread 0 walks the 256 sums and then the 32 bins of the one that holds the rank;
// the histogram is cleared for the next level
__global__ __launch_bounds__(PCT_T) void pct64_scan_kernel(uint64_t* sel, unsigned* hist, int level, const int* done)
{
    __shared__ unsigned part[PCT_T];
    const int s = blockIdx.x, t = threadIdx.x;
    if (done && done[s] != 0) return;
    constexpr int PER_T = PCT_BINS / PCT_T;
    unsigned* h = hist + (size_t)s * PCT_BINS;
    unsigned mine = 0;
    for (int i = 0; i < PER_T; ++i) mine += h[t * PER_T + i];
    part[t] = mine;
    __syncthreads();
    if (t == 0) {
        uint64_t* me = sel + (size_t)s * PCT_WORDS;
        const unsigned rank = (unsigned)me[0];
        unsigned run = 0;
        int c = 0;
        while (c < PCT_T - 1 && rank >= run + part[c]) run += part[c++];   // (a rank beyond the total -- ranks are < per -- ends in the last bin)
        int b = c * PER_T;
        const int end = b + PER_T - 1;
        while (b < end && rank >= run + h[b]) run += h[b++];
        const uint64_t key = me[1] | ((uint64_t)b << pct_shift(level));
        me[0] = rank - run;
        me[1] = key;
        if (level == PCT_LEVELS - 1) {
            // the key is complete and h[b] keys equal it: the next element of the sorted slice is the same key while the rank stays inside that run
            const bool same = me[2] == 0 || rank - run + 1u < h[b];
            me[2] = same ? 0ull : 1ull;
            me[3] = same ? key : ~0ull;
        }
    }
    __syncthreads();
    for (int i = t; i < PCT_BINS; i += PCT_T) h[i] = 0u;
}

// the smallest key above the lower order statistic, where the scan asked for it
__global__ __launch_bounds__(PCT_T) void pct64_succ_kernel(const uint64_t* mod, size_t per, uint64_t* sel, const int* done)
{
    __shared__ unsigned long long red[PCT_T / 64];
    const int s = blockIdx.y;
    if (done && done[s] != 0) return;
    uint64_t* me = sel + (size_t)s * PCT_WORDS;
    if (me[2] == 0) return;   // (written by the scan kernel before this launch; nobody writes it here)
    const uint64_t lo = me[1];
    unsigned long long best = ~0ull;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t key = mod[(size_t)s * per + i];
        if (key > lo && key < best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(best, o, 64);
        best = other < best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PCT_T / 64; ++w) best = red[w] < best ? red[w] : best;
        if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(me + 3), best);
    }
}

__global__ void pct64_tau_kernel(const uint64_t* sel, const double* frac, double2* tau, int niter, int iter, int nslices, const int* done)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslices || (done && done[s] != 0)) return;
    const double a = mod_value(sel[(size_t)s * PCT_WORDS + 1]), b = mod_value(sel[(size_t)s * PCT_WORDS + 3]);
    tau[(size_t)s * niter + iter] = double2{lerp64(a, b, frac[s]), 0.0};
}

// ---- segmented radix sort of 128-bit keys, descending, one segment per slice --------------------------------------------------------------
// As p3d_select.hip: 4 bits per pass (bucket = 15 - digit: the largest digit first), tiles of 4096 keys (256 threads x 16 consecutive keys: a
// thread's keys, then the threads, then the tiles are in index order, so ranks counted that way keep the pass stable).  Passes 0 .. 15 take the
// imaginary word, 16 .. 31 the real word.
struct __attribute__((aligned(16))) Key128 {
    uint64_t re, im;
};
constexpr int SORT_T = 256, SORT_K = 16, SORT_TILE = SORT_T * SORT_K, SORT_PASSES = 32;
__device__ __forceinline__ unsigned sort_bucket(Key128 k, int pass)
{
    const uint64_t word = pass < 16 ? k.im : k.re;
    return 15u - (unsigned)((word >> (4 * (pass & 15))) & 15ull);
}
// (a.re, a.im) > (b.re, b.im), or >=
__device__ __forceinline__ bool key_above(Key128 a, Key128 b, bool strict)
{
    if (a.re != b.re) return a.re > b.re;
    return strict ? a.im > b.im : a.im >= b.im;
}

__global__ void lex_keys64_kernel(Key128* inout, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const double2 v = reinterpret_cast<const double2*>(inout)[i];
        inout[i] = Key128{ord64(v.x), ord64(v.y)};
    }
}

// hist[(slice * 16 + bucket) * tiles + tile] = keys of the tile in the bucket
__global__ __launch_bounds__(SORT_T) void sort64_hist_kernel(const Key128* src, unsigned* hist, size_t per, int tiles, int pass)
{
    __shared__ unsigned cnt[16];
    const int tile = blockIdx.x, slice = blockIdx.y;
    if (threadIdx.x < 16) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const Key128* s = src + (size_t)slice * per;
    const size_t lo = (size_t)tile * SORT_TILE;
    for (int j = 0; j < SORT_K; ++j) {
        const size_t i = lo + (size_t)j * SORT_T + threadIdx.x;   // (any order will do for counting: coalesced)
        if (i < per) atomicAdd(&cnt[sort_bucket(s[i], pass)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16) hist[((size_t)slice * 16 + threadIdx.x) * tiles + tile] = cnt[threadIdx.x];
}
// exclusive prefix of a slice's counts in (bucket, tile) order, in place: where the tile's keys of that bucket start in the sorted slice
__global__ void sort64_scan_kernel(unsigned* hist, int tiles)
{
    __shared__ unsigned total[16];
    const int slice = blockIdx.x, b = threadIdx.x;   // 16 threads
    unsigned* h = hist + ((size_t)slice * 16 + b) * tiles;
    unsigned t = 0;
    for (int i = 0; i < tiles; ++i) t += h[i];
    total[b] = t;
    __syncthreads();
    unsigned run = 0;
    for (int q = 0; q < b; ++q) run += total[q];
    for (int i = 0; i < tiles; ++i) { const unsigned c = h[i]; h[i] = run; run += c; }
}
__global__ __launch_bounds__(SORT_T) void sort64_scatter_kernel(const Key128* src, Key128* dst, const unsigned* offs, size_t per, int tiles, int pass)
{
    __shared__ unsigned cnt[16][SORT_T];   // [bucket][thread]: keys of the thread in the bucket, then their exclusive prefix over the threads
    const int tile = blockIdx.x, slice = blockIdx.y, t = threadIdx.x;
    const Key128* s = src + (size_t)slice * per;
    Key128* d = dst + (size_t)slice * per;
    const size_t i0 = (size_t)tile * SORT_TILE + (size_t)t * SORT_K;   // a thread's 16 CONSECUTIVE keys
#pragma unroll
    for (int b = 0; b < 16; ++b) cnt[b][t] = 0u;
    Key128 key[SORT_K];
    unsigned rank[SORT_K];
#pragma unroll
    for (int j = 0; j < SORT_K; ++j) {
        key[j] = i0 + j < per ? s[i0 + j] : Key128{0ull, 0ull};
        if (i0 + j < per) {
            const unsigned b = sort_bucket(key[j], pass);
            rank[j] = cnt[b][t];          // keys of this thread, of this bucket, before this one (the thread owns its column: no race)
            cnt[b][t] = rank[j] + 1u;
        } else {
            rank[j] = 0u;
        }
    }
    __syncthreads();
    if (t < 16) {   // thread b: exclusive prefix of its bucket's row over the 256 threads
        unsigned run = 0;
        for (int i = 0; i < SORT_T; ++i) { const unsigned c = cnt[t][i]; cnt[t][i] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SORT_K; ++j) {
        if (i0 + j < per) {
            const unsigned b = sort_bucket(key[j], pass);
            d[offs[((size_t)slice * 16 + b) * tiles + tile] + cnt[b][t] + rank[j]] = key[j];
        }
    }
}

__global__ void peaks64_kernel(const Key128* sorted, size_t per, int nslices, double* peaks)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslices) return;
    const Key128 k = sorted[(size_t)s * per];   // descending: the lexicographic maximum (x_fwd.max(), POCS.py:288)
    peaks[2 * s] = unord64(k.re);
    peaks[2 * s + 1] = unord64(k.im);
}

// number of keys of the descending array d[0 .. n) that are > k (strict) or >= k
__device__ size_t count_above(const Key128* d, size_t n, Key128 k, bool strict)
{
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key_above(d[mid], k, strict)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one block per slice: bounds [s][4] = tau_min (re, im), tau_max (re, im)
__global__ void pick64_kernel(const Key128* sorted, size_t per, int niter, const double* bounds, double* tau, long long* count)
{
    const int s = blockIdx.x;
    const Key128* d = sorted + (size_t)s * per;
    __shared__ size_t first, nv;
    if (threadIdx.x == 0) {
        const Key128 klo{ord64(bounds[4 * s]), ord64(bounds[4 * s + 1])}, khi{ord64(bounds[4 * s + 2]), ord64(bounds[4 * s + 3])};
        const size_t i0 = count_above(d, per, khi, false);   // x < tau_max starts here
        const size_t i1 = count_above(d, per, klo, true);    // x > tau_min ends here
        first = i0;
        nv = i1 > i0 ? i1 - i0 : 0;
        count[s] = (long long)nv;
    }
    __syncthreads();
    if (nv == 0) return;
    for (int i = threadIdx.x; i < niter; i += blockDim.x) {
        // ceil(i (Nv - 1) / (niter - 1)) in integers (POCS.py:361-362 take it in float64: the same integer)
        const size_t j = i == 0 || niter < 2 ? 0 : ((size_t)i * (nv - 1) + (size_t)(niter - 2)) / (size_t)(niter - 1);
        const Key128 k = d[first + j];
        tau[((size_t)s * niter + i) * 2] = unord64(k.re);
        tau[((size_t)s * niter + i) * 2 + 1] = unord64(k.im);
    }
}

unsigned pct_blocks(size_t per)
{
    const size_t want = (per + 4095) / 4096;   // ~16 samples per thread
    return (unsigned)(want < 1 ? 1 : (want > 256 ? 256 : want));
}

}  // namespace

hipError_t percentile64(const void* spectrum, size_t per, int nslices, uint64_t* sel, const double* frac, unsigned* hist, uint64_t* mod, void* tau,
                        int niter, int iter, const int* done, hipStream_t st)
{
    if (per > 0xffffffffull || nslices < 1) return hipErrorInvalidValue;   // (ranks and counts are 32-bit)
    const dim3 grid(pct_blocks(per), (unsigned)nslices);
    pct64_mod_kernel<<<grid, PCT_T, 0, st>>>(reinterpret_cast<const double2*>(spectrum), mod, per, hist, done);
    pct64_scan_kernel<<<nslices, PCT_T, 0, st>>>(sel, hist, 0, done);
    for (int level = 1; level < PCT_LEVELS; ++level) {
        pct64_hist_kernel<<<grid, PCT_T, 0, st>>>(mod, per, sel, hist, level, done);
        pct64_scan_kernel<<<nslices, PCT_T, 0, st>>>(sel, hist, level, done);
    }
    pct64_succ_kernel<<<grid, PCT_T, 0, st>>>(mod, per, sel, done);
    pct64_tau_kernel<<<(nslices + 63) / 64, 64, 0, st>>>(sel, frac, reinterpret_cast<double2*>(tau), niter, iter, nslices, done);
    return hipGetLastError();
}

int sort64_tiles(size_t per) { return (int)((per + SORT_TILE - 1) / SORT_TILE); }

hipError_t lex_sort_desc64(void* spectrum, void* other, size_t per, int nslices, unsigned* hist, double* peaks_dev, hipStream_t st)
{
    if (per > 0xffffffffull || nslices < 1) return hipErrorInvalidValue;
    Key128* keys = reinterpret_cast<Key128*>(spectrum);
    Key128* pong = reinterpret_cast<Key128*>(other);
    lex_keys64_kernel<<<4096, 256, 0, st>>>(keys, per * (size_t)nslices);
    const int tiles = sort64_tiles(per);
    const dim3 grid((unsigned)tiles, (unsigned)nslices);
    for (int pass = 0; pass < SORT_PASSES; ++pass) {   // an even number of passes: the sorted keys end where they started
        const Key128* src = (pass & 1) ? pong : keys;
        Key128* dst = (pass & 1) ? keys : pong;
        sort64_hist_kernel<<<grid, SORT_T, 0, st>>>(src, hist, per, tiles, pass);
        sort64_scan_kernel<<<nslices, 16, 0, st>>>(hist, tiles);
        sort64_scatter_kernel<<<grid, SORT_T, 0, st>>>(src, dst, hist, per, tiles, pass);
    }
    peaks64_kernel<<<(nslices + 255) / 256, 256, 0, st>>>(keys, per, nslices, peaks_dev);
    return hipGetLastError();
}

hipError_t data_driven_pick64(const void* sorted, size_t per, int nslices, int niter, const double* bounds_dev, double* tau_dev, long long* count_dev,
                              hipStream_t st)
{
    pick64_kernel<<<nslices, 128, 0, st>>>(reinterpret_cast<const Key128*>(sorted), per, niter, bounds_dev, tau_dev, count_dev);
    return hipGetLastError();
}

}  // namespace sel64
}  // namespace p3d
