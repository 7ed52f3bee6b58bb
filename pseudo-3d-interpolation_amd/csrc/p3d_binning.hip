// p3d_binning.hip -- trace stacking of step 10 (the reference's inlines_from_seismic, cube_binning_3D.py:922-1240): every bin of the
// (iline, xline) grid stacks the traces that fall into it, after aligning them on the global twt axis, and the cube is written slice-major.
//
// Input layout (CSR, prepared by the host): the traces are sorted into bin order, bin b = il * nxl + xl owns traces
// bin_start[b] .. bin_start[b + 1] (empty bins included).  Trace t has its samples at samples[trace_off[t] .. + trace_len[t]); its sample i
// lands on output sample j = i + shift[t], and it contributes 0 wherever 0 <= j - shift[t] < trace_len[t] does not hold (the reference's
// pad_trace: zero padding that COUNTS in the mean and the median).  Output: out[nt][nil][nxl] float32, empty bins 0.
//   average: sum over the bin's k padded traces in double, / k, rounded once;
//   median:  per sample the exact median of the k padded values; for even k the float32 (a + b) / 2 of the two middle values
//            (np.median of a float32 stack, bit for bit);
//   nearest: the first trace of the bin (the host keeps only the nearest one), a shifted copy;
//   IDW:     sum w[t] x[t] in double with the host's normalised weights, rounded once.
// No atomics: every output element is computed by one lane and written once, so the result is bitwise repeatable.
//
// Shape: one 256-thread workgroup per (64 consecutive xlines of one inline) x (128 samples).  Gather phase: wave w takes bins w, w + 4, ...
// of the tile; its 64 lanes hold 2 samples each (j0 + lane, j0 + 64 + lane), so every trace piece is read as contiguous 256-B rows, once.
// The wave's results go to an LDS tile [64 xlines][128 + 1 samples]; the write phase then stores rows of 64 consecutive xlines per sample
// (coalesced along xline).  Median: k <= 16 sorts k values (+inf padded) per sample in registers with a bitonic network of 8 or 16; larger k
// selects the order statistics by a 32-pass radix descent over the float's ordered bit pattern (k reads per pass, nothing held per value):
// no per-lane array is indexed at run time, so no scratch memory for any k.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"
#include "p3d_sortnet.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

enum { BIN_AVERAGE = 0, BIN_MEDIAN = 1, BIN_NEAREST = 2, BIN_IDW = 3 };

constexpr int TX = 64;            // xlines per tile (one wave-row of the write phase)
constexpr int SPL = 2;            // samples per lane in the gather phase
constexpr int TS = 64 * SPL;      // samples per tile
constexpr int NW = 4;             // waves per workgroup

struct BinArgs {
    const float* samples;
    const long long* trace_off;
    const int* trace_len;
    const int* shift;
    const double* weight;
    const long long* bin_start;   // absolute trace indices; trace t of the buffers is bin_start value - tbase
    long long tbase, sbase;       // chunked runs: first trace / first sample of the uploaded span
    long long nt, nxl, nil;       // nil: inlines of this launch (the slab); bins il * nxl + xl of the slab
    long long il0;                // first inline of the slab in bin_start
    float* out;                   // [nt][nil][nxl]
    unsigned ntiles_x, ntiles_t;
};

__device__ inline float tap(const BinArgs& a, long long off, int len, int sh, long long j)
{
    const long long i = j - sh;
    return (j < a.nt && i >= 0 && i < len) ? a.samples[off + i] : 0.0f;
}

__device__ inline unsigned fkey(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float funkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// median of the k values of sample j (k <= N), +inf padded and sorted in registers; runtime ranks picked by compare, not by index
template <int N>
__device__ inline float median_small(const BinArgs& a, long long t0, int k, long long j)
{
    float v[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        v[q] = INFINITY;
        if (q < k) v[q] = tap(a, a.trace_off[t0 + q] - a.sbase, a.trace_len[t0 + q], a.shift[t0 + q], j);
    }
    p3d::bitonic<N>(v);
    const int m2 = k >> 1, m1 = (k - 1) >> 1;
    float lo = 0.0f, hi = 0.0f;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        if (q == m1) lo = v[q];
        if (q == m2) hi = v[q];
    }
    return (k & 1) ? hi : (lo + hi) / 2.0f;
}

// any k: rank m1 = (k - 1) / 2 by a radix descent on the ordered keys, rank m2 = k / 2 from one or two more passes
__device__ inline float median_large(const BinArgs& a, long long t0, long long k, long long j)
{
    const long long m1 = (k - 1) >> 1, m2 = k >> 1;
    unsigned prefix = 0u, mask = 0u;
    long long rem = m1;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned b = 1u << bit;
        long long cnt = 0;
        for (long long t = t0; t < t0 + k; ++t) {
            const unsigned key = fkey(tap(a, a.trace_off[t] - a.sbase, a.trace_len[t], a.shift[t], j));
            cnt += ((key & mask) == prefix && (key & b) == 0u);
        }
        if (rem >= cnt) {
            prefix |= b;
            rem -= cnt;
        }
        mask |= b;
    }
    const float lo = funkey(prefix);
    if (m1 == m2) return lo;
    long long le = 0;
    unsigned next = 0xffffffffu;
    for (long long t = t0; t < t0 + k; ++t) {
        const unsigned key = fkey(tap(a, a.trace_off[t] - a.sbase, a.trace_len[t], a.shift[t], j));
        le += key <= prefix;
        if (key > prefix && key < next) next = key;
    }
    const float hi = le > m2 ? lo : funkey(next);
    return (lo + hi) / 2.0f;
}

template <int METHOD>
__global__ void __launch_bounds__(256) bin_stack_kernel(BinArgs a)
{
    __shared__ float tile[TX][TS + 1];
    const unsigned blk = blockIdx.x;
    const unsigned tx = blk % a.ntiles_x;
    const unsigned rest = blk / a.ntiles_x;
    const long long il = rest % (unsigned)a.nil;
    const long long j0 = (long long)(rest / (unsigned)a.nil) * TS;
    const long long xl0 = (long long)tx * TX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (int xb = wave; xb < TX; xb += NW) {
        const long long xl = xl0 + xb;
        float res[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) res[s] = 0.0f;
        if (xl < a.nxl) {
            const long long b = (a.il0 + il) * a.nxl + xl;
            const long long t0 = a.bin_start[b] - a.tbase, t1 = a.bin_start[b + 1] - a.tbase;
            const long long k = t1 - t0;
            if (k > 0) {
                if (METHOD == BIN_MEDIAN) {
#pragma unroll
                    for (int s = 0; s < SPL; ++s) {
                        const long long j = j0 + lane + 64 * s;
                        if (j >= a.nt) continue;
                        if (k <= 8) res[s] = median_small<8>(a, t0, (int)k, j);
                        else if (k <= 16) res[s] = median_small<16>(a, t0, (int)k, j);
                        else res[s] = median_large(a, t0, k, j);
                    }
                } else {
                    double acc[SPL];
#pragma unroll
                    for (int s = 0; s < SPL; ++s) acc[s] = 0.0;
                    const long long tend = METHOD == BIN_NEAREST ? t0 + 1 : t1;
                    long long t = t0;
                    for (; t + 1 < tend; t += 2) {          // two traces in flight
                        const long long o0 = a.trace_off[t] - a.sbase, o1 = a.trace_off[t + 1] - a.sbase;
                        const int n0 = a.trace_len[t], n1 = a.trace_len[t + 1], h0 = a.shift[t], h1 = a.shift[t + 1];
                        float x0[SPL], x1[SPL];
#pragma unroll
                        for (int s = 0; s < SPL; ++s) {
                            x0[s] = tap(a, o0, n0, h0, j0 + lane + 64 * s);
                            x1[s] = tap(a, o1, n1, h1, j0 + lane + 64 * s);
                        }
                        if (METHOD == BIN_IDW) {
                            const double w0 = a.weight[t], w1 = a.weight[t + 1];
#pragma unroll
                            for (int s = 0; s < SPL; ++s) {
                                acc[s] += w0 * (double)x0[s];
                                acc[s] += w1 * (double)x1[s];
                            }
                        } else {
#pragma unroll
                            for (int s = 0; s < SPL; ++s) {
                                acc[s] += (double)x0[s];
                                acc[s] += (double)x1[s];
                            }
                        }
                    }
                    if (t < tend) {
                        const long long o0 = a.trace_off[t] - a.sbase;
                        const int n0 = a.trace_len[t], h0 = a.shift[t];
                        const double w0 = METHOD == BIN_IDW ? a.weight[t] : 1.0;
#pragma unroll
                        for (int s = 0; s < SPL; ++s) acc[s] += w0 * (double)tap(a, o0, n0, h0, j0 + lane + 64 * s);
                    }
#pragma unroll
                    for (int s = 0; s < SPL; ++s) res[s] = METHOD == BIN_AVERAGE ? (float)(acc[s] / (double)k) : (float)acc[s];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < SPL; ++s) tile[xb][lane + 64 * s] = res[s];
    }
    __syncthreads();

    const long long slab = a.nil * a.nxl;
    for (int e = threadIdx.x; e < TX * TS; e += 256) {
        const int x = e % TX, s = e / TX;
        const long long j = j0 + s, xl = xl0 + x;
        if (j < a.nt && xl < a.nxl) a.out[j * slab + il * a.nxl + xl] = tile[x][s];
    }
}

int launch(const BinArgs& a0, int method, hipStream_t stream)
{
    BinArgs a = a0;
    a.ntiles_x = (unsigned)((a.nxl + TX - 1) / TX);
    a.ntiles_t = (unsigned)((a.nt + TS - 1) / TS);
    const unsigned long long blocks = (unsigned long long)a.ntiles_x * (unsigned long long)a.nil * a.ntiles_t;
    if (blocks == 0) return P3D_OK;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "cube of %lld x %lld x %lld needs %llu workgroups", a.nt, a.nil, a.nxl, blocks);
    switch (method) {
    case BIN_AVERAGE: bin_stack_kernel<BIN_AVERAGE><<<(unsigned)blocks, 256, 0, stream>>>(a); break;
    case BIN_MEDIAN: bin_stack_kernel<BIN_MEDIAN><<<(unsigned)blocks, 256, 0, stream>>>(a); break;
    case BIN_NEAREST: bin_stack_kernel<BIN_NEAREST><<<(unsigned)blocks, 256, 0, stream>>>(a); break;
    default: bin_stack_kernel<BIN_IDW><<<(unsigned)blocks, 256, 0, stream>>>(a); break;
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int check_common(int nt, int nil, int nxl, int method)
{
    if (nt < 1 || nil < 1 || nxl < 1) return fail(P3D_ERR_INVALID, "bad cube shape (nt %d, nil %d, nxl %d)", nt, nil, nxl);
    if (method < BIN_AVERAGE || method > BIN_IDW) return fail(P3D_ERR_INVALID, "unknown stacking method %d", method);
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_bin_stack(int device, const float* samples, const long long* trace_off, const int* trace_len, const int* shift, const double* weight,
                  size_t ntraces, const long long* bin_start, int nil, int nxl, int nt, int method, size_t max_bytes, float* out)
{
    if (!out || !bin_start || (ntraces > 0 && (!samples || !trace_off || !trace_len || !shift))) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = check_common(nt, nil, nxl, method)) return rc;
    if (method == BIN_IDW && ntraces > 0 && !weight) return fail(P3D_ERR_INVALID, "IDW needs weights");
    const long long nbins = (long long)nil * nxl;
    if (bin_start[0] != 0 || bin_start[nbins] != (long long)ntraces) return fail(P3D_ERR_INVALID, "bin_start must run from 0 to ntraces");
    for (long long b = 0; b < nbins; ++b)
        if (bin_start[b + 1] < bin_start[b]) return fail(P3D_ERR_INVALID, "bin_start decreases at bin %lld", b);
    for (size_t t = 0; t < ntraces; ++t)
        if (trace_len[t] < 0 || trace_off[t] < 0) return fail(P3D_ERR_INVALID, "trace %zu: negative offset or length", t);
    if (int rc = use_device(device)) return rc;

    size_t free_b = 0, total_b = 0;
    P3D_TRY(hipMemGetInfo(&free_b, &total_b));
    size_t cap = free_b / 2;
    if (max_bytes > 0 && max_bytes < cap) cap = max_bytes;

    // device bytes of inlines [i0, i1): the cube slab, the span of their samples, the per-trace tables and bin_start
    const size_t per_trace = sizeof(long long) + 2 * sizeof(int) + (weight ? sizeof(double) : 0);
    auto span_of = [&](long long i0, long long i1, long long& s0, long long& s1) {
        s0 = 0;
        s1 = 0;
        bool any = false;
        for (long long t = bin_start[i0 * nxl]; t < bin_start[i1 * nxl]; ++t) {
            if (trace_len[t] == 0) continue;
            const long long a = trace_off[t], b = a + trace_len[t];
            if (!any || a < s0) s0 = a;
            if (!any || b > s1) s1 = b;
            any = true;
        }
    };
    auto bytes_of = [&](long long i0, long long i1) {
        long long s0, s1;
        span_of(i0, i1, s0, s1);
        const long long ntr = bin_start[i1 * nxl] - bin_start[i0 * nxl];
        return (size_t)nt * (size_t)(i1 - i0) * nxl * sizeof(float) + (size_t)(s1 - s0) * sizeof(float) + (size_t)ntr * per_trace +
               (size_t)((i1 - i0) * nxl + 1) * sizeof(long long);
    };

    // chunks of whole inlines, each within the cap: grow while the next inline still fits (traces in bin order keep the span tight)
    std::vector<long long> cuts{0};
    while (cuts.back() < nil) {
        const long long i0 = cuts.back();
        if (bytes_of(i0, i0 + 1) > cap)
            return fail(P3D_ERR_UNSUPPORTED, "inline %lld needs %zu device bytes, more than the %zu available", i0, bytes_of(i0, i0 + 1), cap);
        long long lo = i0 + 1, hi = nil;                    // largest i1 in [lo, hi] with bytes_of(i0, i1) <= cap (monotone in i1)
        while (lo < hi) {
            const long long mid = lo + (hi - lo + 1) / 2;
            if (bytes_of(i0, mid) <= cap) lo = mid;
            else hi = mid - 1;
        }
        cuts.push_back(lo);
    }

    size_t max_cube = 0, max_span = 0, max_tr = 0, max_bins = 0;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        long long s0, s1;
        span_of(cuts[c], cuts[c + 1], s0, s1);
        const size_t n = cuts[c + 1] - cuts[c];
        max_cube = std::max(max_cube, (size_t)nt * n * nxl);
        max_span = std::max(max_span, (size_t)(s1 - s0));
        max_tr = std::max(max_tr, (size_t)(bin_start[cuts[c + 1] * nxl] - bin_start[cuts[c] * nxl]));
        max_bins = std::max(max_bins, n * nxl + 1);
    }
    DevBuf dcube, dsmp, doff, dlen, dsh, dw, dbs;
    P3D_TRY(hipMalloc(&dcube.p, max_cube * sizeof(float)));
    P3D_TRY(hipMalloc(&dbs.p, max_bins * sizeof(long long)));
    if (max_tr > 0) {
        P3D_TRY(hipMalloc(&dsmp.p, std::max<size_t>(max_span, 1) * sizeof(float)));
        P3D_TRY(hipMalloc(&doff.p, max_tr * sizeof(long long)));
        P3D_TRY(hipMalloc(&dlen.p, max_tr * sizeof(int)));
        P3D_TRY(hipMalloc(&dsh.p, max_tr * sizeof(int)));
        if (weight) P3D_TRY(hipMalloc(&dw.p, max_tr * sizeof(double)));
    }

    const size_t row = (size_t)nil * nxl * sizeof(float);
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const long long i0 = cuts[c], i1 = cuts[c + 1], n = i1 - i0;
        long long s0, s1;
        span_of(i0, i1, s0, s1);
        const long long tb = bin_start[i0 * nxl], ntr = bin_start[i1 * nxl] - tb;
        P3D_TRY(hipMemcpy(dbs.p, bin_start + i0 * nxl, (size_t)(n * nxl + 1) * sizeof(long long), hipMemcpyHostToDevice));
        if (ntr > 0) {
            if (s1 > s0) P3D_TRY(hipMemcpy(dsmp.p, samples + s0, (size_t)(s1 - s0) * sizeof(float), hipMemcpyHostToDevice));
            P3D_TRY(hipMemcpy(doff.p, trace_off + tb, (size_t)ntr * sizeof(long long), hipMemcpyHostToDevice));
            P3D_TRY(hipMemcpy(dlen.p, trace_len + tb, (size_t)ntr * sizeof(int), hipMemcpyHostToDevice));
            P3D_TRY(hipMemcpy(dsh.p, shift + tb, (size_t)ntr * sizeof(int), hipMemcpyHostToDevice));
            if (weight) P3D_TRY(hipMemcpy(dw.p, weight + tb, (size_t)ntr * sizeof(double), hipMemcpyHostToDevice));
        }
        // offsets of zero-length traces may lie outside the span: they are never dereferenced (tap() checks the length first)
        BinArgs a{(const float*)dsmp.p, (const long long*)doff.p, (const int*)dlen.p, (const int*)dsh.p, (const double*)dw.p,
                  (const long long*)dbs.p, tb, s0, nt, nxl, n, 0, (float*)dcube.p, 0, 0};
        if (int rc = launch(a, method, 0)) return rc;
        const size_t w = (size_t)n * nxl * sizeof(float);
        P3D_TRY(hipMemcpy2D(out + (size_t)i0 * nxl, row, dcube.p, w, w, (size_t)nt, hipMemcpyDeviceToHost));
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_bin_stack_dev(int device, const float* samples_dev, const long long* trace_off_dev, const int* trace_len_dev, const int* shift_dev,
                      const double* weight_dev, const long long* bin_start_dev, int nil, int nxl, int nt, int method, float* out_dev)
{
    if (!out_dev || !bin_start_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = check_common(nt, nil, nxl, method)) return rc;
    if (method == BIN_IDW && !weight_dev) return fail(P3D_ERR_INVALID, "IDW needs weights");
    if (int rc = use_device(device)) return rc;
    BinArgs a{samples_dev, trace_off_dev, trace_len_dev, shift_dev, weight_dev, bin_start_dev, 0, 0, nt, nxl, nil, 0, out_dev, 0, 0};
    if (int rc = launch(a, method, 0)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // extern "C"
