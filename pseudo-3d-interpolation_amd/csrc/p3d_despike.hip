// p3d_despike.hip -- step 8 of the workflow (the reference's despike_2D, despiking_2D_segy.py): single-trace noise bursts are found by comparing
// every sample with the background amplitude of w adjacent traces, and replaced from the neighbouring traces.
//
// The section stays in the file's own layout, trace-major [ntr][ns] float32.  Lanes run along samples (coalesced), the window slides across traces.
//
// Detection (despike_detect_kernel<W, MODE>): for row t the window value is m[t][j] = f(|a[t][j .. j + W - 1]|), f = mean / median / rms, and sample
// (t, x) is a candidate if |a[t][x]| > threshold * m[t][j] for ANY window that contains it, i.e. against the smallest of them.  A thread owns one
// sample index t and walks a tile of traces plus a halo of W - 1 traces on either side, with the last W absolute values and the last W window
// values in registers (shifted by constant index, never indexed at run time: no scratch).  mean / rms accumulate in float32 in NumPy's order
// (np_sum: sequential below 8 terms, eight partial sums combined pairwise from 8 on), the median is the middle of a register sorting network (W is
// odd, so it is an element of the data).  Windows never cross a split boundary (Tile::seg_lo / seg_hi).  The wave's 64 decisions are one ballot word
// of the packed mask [ntr][ceil(ns / 64)]; rows that neither view of the reference examines are masked out.  despike_count_kernel then counts each
// trace's candidates inside the rows of the main and of the additional view (one wave per trace, integer popcounts; no atomics anywhere).
//
// Replacement (despike_replace_kernel): one workgroup per spike record (trace, lo, hi, first, last, c0, c1): rows lo .. hi of the trace are rewritten
// from columns c0 .. c1.  The host launches one batch per level, spikes of one batch neither read nor write what another of the batch writes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"
#include "p3d_sortnet.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

enum { DSP_MEAN = 0, DSP_MEDIAN = 1, DSP_RMS = 2 };
enum { OUT_SCALED = 0, OUT_MODE = 1, OUT_THRESHOLD = 2, OUT_ZEROS = 3, OUT_MEDIAN = 4 };

constexpr int MAXW = P3D_DESPIKE_MAX_TRACES;   // widest window (odd)
constexpr int TT = 128;                        // traces per detection tile
constexpr int BS = 256;                        // threads (= samples) per workgroup
constexpr int SPIKE_INTS = 8;                  // ints per spike record

struct Tile {
    int seg_lo, seg_hi;   // the split that owns the tile: windows live in [seg_lo, seg_hi)
    int x0, x1;           // traces decided by the tile
};

struct Spike {
    int x, lo, hi, first, last, c0, c1, pad;
};

// np.add.reduce of N float32 terms in NumPy's order: 0 + a0 + a1 + ... below 8 terms; from 8 on, eight running sums over blocks of 8, combined
// pairwise, then the remainder added in order
template <int N>
__device__ inline float np_sum(const float (&v)[N])
{
    if constexpr (N < 8) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) s += v[i];
        return s;
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = v[j];
        constexpr int NB = N - N % 8;
#pragma unroll
        for (int i = 8; i < NB; i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += v[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = NB; i < N; ++i) res += v[i];
        return 0.0f + res;
    }
}

// the same for a run-time count n <= 32 (the clipped neighbour window of the replacement); v[k >= n] is not read
__device__ inline float np_sum_n(const float (&v)[32], int n)
{
    if (n < 8) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < n) s += v[k];
        return s;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = v[j];
    const int nb = n - n % 8;
#pragma unroll
    for (int b = 8; b < 32; b += 8)
        if (b < nb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += v[b + j];
        }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int k = 8; k < 32; ++k)
        if (k >= nb && k < n) res += v[k];
    return 0.0f + res;
}

constexpr int pow2_at_least(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

template <int W, int MODE>
__device__ inline float window_value(const float (&ring)[W])
{
    if constexpr (MODE == DSP_MEAN) {
        return np_sum<W>(ring) / (float)W;
    } else if constexpr (MODE == DSP_RMS) {
        float sq[W];
#pragma unroll
        for (int i = 0; i < W; ++i) sq[i] = ring[i] * ring[i];
        return sqrtf(np_sum<W>(sq) / (float)W);
    } else {
        constexpr int N = pow2_at_least(W);
        float v[N];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = i < W ? ring[i] : INFINITY;
        p3d::bitonic<N>(v);
        return v[W / 2];
    }
}

template <int W, int MODE>
__global__ void __launch_bounds__(BS) despike_detect_kernel(const float* __restrict__ a, const Tile* __restrict__ tiles, unsigned nsb, int ns, float thr,
                                                            int main_end, int add_start, unsigned long long* __restrict__ mask, int nw64)
{
    const Tile tl = tiles[blockIdx.x / nsb];
    const int t = (int)(blockIdx.x % nsb) * BS + (int)threadIdx.x;
    const bool live = t < ns;
    const bool examined = live && (t < main_end || t >= add_start);
    float ring[W], mr[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        ring[i] = 0.0f;
        mr[i] = INFINITY;
    }
    const int pstart = max(tl.seg_lo, tl.x0 - (W - 1));
    const int pend = tl.x1 + (W - 1);   // traces beyond the split are virtual: they close the windows of the last W - 1 real ones
    for (int p = pstart; p < pend; ++p) {
        const bool real = p < tl.seg_hi;
        float v = 0.0f;
        if (live && real) v = fabsf(a[(size_t)p * ns + t]);
#pragma unroll
        for (int i = 0; i + 1 < W; ++i) ring[i] = ring[i + 1];
        ring[W - 1] = v;
        const int j = p - (W - 1);      // the window that trace p completes, and the trace decided now
        float m = INFINITY;
        if (real && j >= tl.seg_lo) m = window_value<W, MODE>(ring);
#pragma unroll
        for (int i = 0; i + 1 < W; ++i) mr[i] = mr[i + 1];
        mr[W - 1] = m;
        if (j >= tl.x0) {
            float mm = mr[0];           // windows j - W + 1 ... j: the ones that contain trace j (+inf where there is none)
#pragma unroll
            for (int i = 1; i < W; ++i) mm = fminf(mm, mr[i]);
            const bool cand = examined && ring[0] > thr * mm;
            const unsigned long long word = __ballot(cand);
            if ((threadIdx.x & 63) == 0 && live) mask[(size_t)j * nw64 + (t >> 6)] = word;
        }
    }
}

// counts[x] / counts[ntr + x]: candidates of trace x in the rows of the main view (t < main_end) / of the additional view (t >= add_start)
__global__ void __launch_bounds__(64) despike_count_kernel(const unsigned long long* __restrict__ mask, int nw64, int ntr, int main_end, int add_start,
                                                           int* __restrict__ counts)
{
    const int x = blockIdx.x;
    int cm = 0, ca = 0;
    for (int k = threadIdx.x; k < nw64; k += 64) {
        const unsigned long long word = mask[(size_t)x * nw64 + k];
        const long long t0 = (long long)k * 64;
        unsigned long long in_main = 0ull, in_add = 0ull;
        if (main_end >= t0 + 64) in_main = ~0ull;
        else if (main_end > t0) in_main = (1ull << (main_end - t0)) - 1ull;
        if (add_start <= t0) in_add = ~0ull;
        else if (add_start < t0 + 64) in_add = ~((1ull << (add_start - t0)) - 1ull);
        cm += __popcll(word & in_main);
        ca += __popcll(word & in_add);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        cm += __shfl_xor(cm, d);
        ca += __shfl_xor(ca, d);
    }
    if (threadIdx.x == 0) {
        counts[x] = cm;
        counts[ntr + x] = ca;
    }
}

// np.median of the n values v[0 .. n): the middle of the sorted values, for even n the float32 mean of the two middle ones
__device__ inline float median_n(float (&v)[32], int n)
{
#pragma unroll
    for (int k = 0; k < 32; ++k)
        if (k >= n) v[k] = INFINITY;
    p3d::bitonic<32>(v);
    const int m1 = (n - 1) >> 1, m2 = n >> 1;
    float lo = 0.0f, hi = 0.0f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        if (k == m1) lo = v[k];
        if (k == m2) hi = v[k];
    }
    return (n & 1) ? hi : (0.0f + lo + hi) / 2.0f;
}

// f over the n values of v (mean / median / rms), as NumPy computes it in float32
__device__ inline float mode_value(float (&v)[32], int n, int mode)
{
    if (mode == DSP_MEAN) return np_sum_n(v, n) / (float)n;
    if (mode == DSP_RMS) {
#pragma unroll
        for (int k = 0; k < 32; ++k) v[k] = v[k] * v[k];
        return sqrtf(np_sum_n(v, n) / (float)n);
    }
    return median_n(v, n);
}

__global__ void __launch_bounds__(BS) despike_replace_kernel(float* __restrict__ a, const Spike* __restrict__ spikes, int ns, int mode, int out, float thr)
{
    __shared__ float red[BS / 64];
    const Spike s = spikes[blockIdx.x];
    const int L = s.hi - s.lo, n = s.c1 - s.c0;
    float* own = a + (size_t)s.x * ns + s.lo;
    float mx = -INFINITY;
    if (out == OUT_SCALED) {   // the trace's (signed) maximum over the padded rows, before any of them is rewritten
        for (int i = threadIdx.x; i < L; i += BS) mx = fmaxf(mx, own[i]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
    for (int i = threadIdx.x; i < L; i += BS) {
        float res = 0.0f;
        if (out != OUT_ZEROS) {
            float v[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                v[k] = 0.0f;
                if (k < n) v[k] = a[(size_t)(s.c0 + k) * ns + s.lo + i];
            }
            if (out == OUT_MEDIAN) {
                res = median_n(v, n);
            } else if (out == OUT_SCALED) {
                const float mine = own[i];
#pragma unroll
                for (int k = 0; k < 32; ++k) v[k] = fabsf(v[k]);
                const float val = mine / (mx / mode_value(v, n, mode));
                double taper = 1.0;   // np.blackman(L)[i], in double
                if (L > 1) {
                    const double pi = 3.141592653589793, nn = (double)(1 - L + 2 * i), den = (double)(L - 1);
                    taper = 0.42 + 0.5 * cos(pi * nn / den) + 0.08 * cos(2.0 * pi * nn / den);
                }
                res = (float)((double)val * taper);
            } else {
                res = mode_value(v, n, mode);
                if (out == OUT_THRESHOLD) res = res * thr;
            }
        }
        own[i] = res;
    }
}

int check_window(int ntr, int ns, int w, int mode)
{
    if (ntr < 1 || ns < 1) return fail(P3D_ERR_INVALID, "bad section shape (%d traces, %d samples)", ntr, ns);
    if (mode < DSP_MEAN || mode > DSP_RMS) return fail(P3D_ERR_INVALID, "unknown amplitude mode %d", mode);
    if (w < 3 || w % 2 == 0) return fail(P3D_ERR_INVALID, "the trace window must be an odd number of at least 3 traces, got %d", w);
    if (w > MAXW) return fail(P3D_ERR_UNSUPPORTED, "trace windows of up to %d traces are supported, got %d", MAXW, w);
    return P3D_OK;
}

template <int W>
void launch_detect_w(int mode, unsigned blocks, hipStream_t st, const float* a, const Tile* tiles, unsigned nsb, int ns, float thr, int main_end, int add_start,
                     unsigned long long* mask, int nw64)
{
    switch (mode) {
    case DSP_MEAN: despike_detect_kernel<W, DSP_MEAN><<<blocks, BS, 0, st>>>(a, tiles, nsb, ns, thr, main_end, add_start, mask, nw64); break;
    case DSP_MEDIAN: despike_detect_kernel<W, DSP_MEDIAN><<<blocks, BS, 0, st>>>(a, tiles, nsb, ns, thr, main_end, add_start, mask, nw64); break;
    default: despike_detect_kernel<W, DSP_RMS><<<blocks, BS, 0, st>>>(a, tiles, nsb, ns, thr, main_end, add_start, mask, nw64); break;
    }
}

// section_dev [ntr][ns], mask_dev [ntr][nw64], counts_dev [2][ntr]: device; splits: host, nsplits + 1 ascending boundaries from 0 to ntr
int detect_dev(const float* section_dev, int ntr, int ns, int w, int mode, float thr, int main_end, int add_start, const int* splits, int nsplits,
               unsigned long long* mask_dev, int* counts_dev)
{
    if (int rc = check_window(ntr, ns, w, mode)) return rc;
    if (!section_dev || !mask_dev || !counts_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (main_end < 0 || main_end > ns || add_start < 0) return fail(P3D_ERR_INVALID, "view rows outside the section (main_end %d, add_start %d)", main_end, add_start);
    const int one[2] = {0, ntr};
    if (!splits || nsplits < 1) {
        splits = one;
        nsplits = 1;
    }
    if (splits[0] != 0 || splits[nsplits] != ntr) return fail(P3D_ERR_INVALID, "split boundaries must run from 0 to the number of traces");
    std::vector<Tile> tiles;
    for (int s = 0; s < nsplits; ++s) {
        if (splits[s + 1] <= splits[s]) return fail(P3D_ERR_INVALID, "split boundaries must ascend");
        for (int x0 = splits[s]; x0 < splits[s + 1]; x0 += TT) tiles.push_back(Tile{splits[s], splits[s + 1], x0, std::min(x0 + TT, splits[s + 1])});
    }
    const unsigned nsb = (unsigned)((ns + BS - 1) / BS);
    const unsigned long long blocks = (unsigned long long)tiles.size() * nsb;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "section too large for one launch (%llu workgroups)", blocks);
    const int nw64 = (ns + 63) / 64;
    DevBuf dt;
    P3D_TRY(hipMalloc(&dt.p, tiles.size() * sizeof(Tile)));
    P3D_TRY(hipMemcpy(dt.p, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice));
    const Tile* tp = (const Tile*)dt.p;
    const unsigned nb = (unsigned)blocks;
#define DSP_CASE(W) case W: launch_detect_w<W>(mode, nb, 0, section_dev, tp, nsb, ns, thr, main_end, add_start, mask_dev, nw64); break;
    switch (w) {
        DSP_CASE(3) DSP_CASE(5) DSP_CASE(7) DSP_CASE(9) DSP_CASE(11) DSP_CASE(13) DSP_CASE(15) DSP_CASE(17) DSP_CASE(19) DSP_CASE(21) DSP_CASE(23)
        DSP_CASE(25) DSP_CASE(27) DSP_CASE(29) DSP_CASE(31)
    default: return fail(P3D_ERR_UNSUPPORTED, "no kernel for a window of %d traces", w);
    }
#undef DSP_CASE
    P3D_TRY(hipGetLastError());
    despike_count_kernel<<<(unsigned)ntr, 64, 0, 0>>>(mask_dev, nw64, ntr, main_end, add_start, counts_dev);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());   // the tile table is freed on return
    return P3D_OK;
}

int check_spikes(const int* spikes, size_t nspikes, const int* level_start, int nlevels, int ntr, int ns)
{
    if (nlevels < 0 || (nspikes > 0 && (!spikes || !level_start || nlevels < 1))) return fail(P3D_ERR_INVALID, "spike records without levels");
    if (nlevels > 0 && (level_start[0] != 0 || (size_t)level_start[nlevels] != nspikes)) return fail(P3D_ERR_INVALID, "level offsets must run from 0 to the number of spikes");
    for (int l = 0; l < nlevels; ++l)
        if (level_start[l + 1] < level_start[l]) return fail(P3D_ERR_INVALID, "level offsets must not descend");
    for (size_t i = 0; i < nspikes; ++i) {
        const int* r = spikes + i * SPIKE_INTS;
        const bool ok = r[5] >= 0 && r[5] <= r[0] && r[0] < r[6] && r[6] <= ntr && r[6] - r[5] <= MAXW && r[1] >= 0 && r[1] < r[2] && r[2] <= ns;
        if (!ok) return fail(P3D_ERR_INVALID, "spike record %zu outside the section (trace %d, rows %d:%d, columns %d:%d)", i, r[0], r[1], r[2], r[5], r[6]);
    }
    return P3D_OK;
}

int replace_dev(float* section_dev, int ntr, int ns, const int* spikes, size_t nspikes, const int* level_start, int nlevels, int mode, int out, float thr)
{
    if (ntr < 1 || ns < 1 || !section_dev) return fail(P3D_ERR_INVALID, "bad section");
    if (mode < DSP_MEAN || mode > DSP_RMS) return fail(P3D_ERR_INVALID, "unknown amplitude mode %d", mode);
    if (out < OUT_SCALED || out > OUT_MEDIAN) return fail(P3D_ERR_INVALID, "unknown output amplitude option %d", out);
    if (int rc = check_spikes(spikes, nspikes, level_start, nlevels, ntr, ns)) return rc;
    if (nspikes == 0) return P3D_OK;
    DevBuf ds;
    P3D_TRY(hipMalloc(&ds.p, nspikes * sizeof(Spike)));
    P3D_TRY(hipMemcpy(ds.p, spikes, nspikes * sizeof(Spike), hipMemcpyHostToDevice));
    for (int l = 0; l < nlevels; ++l) {   // one batch per level, in stream order
        const int n = level_start[l + 1] - level_start[l];
        if (n == 0) continue;
        despike_replace_kernel<<<(unsigned)n, BS, 0, 0>>>(section_dev, (const Spike*)ds.p + level_start[l], ns, mode, out, thr);
        P3D_TRY(hipGetLastError());
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_despike_detect_dev(int device, const float* section_dev, int ntr, int ns, int w, int mode, float threshold, int main_end, int add_start,
                           const int* splits, int nsplits, unsigned long long* mask_dev, int* counts_dev)
{
    if (int rc = check_window(ntr, ns, w, mode)) return rc;
    if (int rc = use_device(device)) return rc;
    return detect_dev(section_dev, ntr, ns, w, mode, threshold, main_end, add_start, splits, nsplits, mask_dev, counts_dev);
}

int p3d_despike_detect(int device, const float* section, int ntr, int ns, int w, int mode, float threshold, int main_end, int add_start, const int* splits,
                       int nsplits, unsigned long long* mask, int* counts)
{
    if (int rc = check_window(ntr, ns, w, mode)) return rc;
    if (!section || !mask || !counts) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nw64 = (size_t)(ns + 63) / 64, nsec = (size_t)ntr * ns * sizeof(float), nmask = (size_t)ntr * nw64 * sizeof(unsigned long long);
    DevBuf da, dm, dc;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&dm.p, nmask));
    P3D_TRY(hipMalloc(&dc.p, 2 * (size_t)ntr * sizeof(int)));
    P3D_TRY(hipMemcpy(da.p, section, nsec, hipMemcpyHostToDevice));
    if (int rc = detect_dev((const float*)da.p, ntr, ns, w, mode, threshold, main_end, add_start, splits, nsplits, (unsigned long long*)dm.p, (int*)dc.p)) return rc;
    P3D_TRY(hipMemcpy(mask, dm.p, nmask, hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(counts, dc.p, 2 * (size_t)ntr * sizeof(int), hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_despike_replace_dev(int device, float* section_dev, int ntr, int ns, const int* spikes, size_t nspikes, const int* level_start, int nlevels, int mode,
                            int out, float threshold)
{
    if (int rc = use_device(device)) return rc;
    return replace_dev(section_dev, ntr, ns, spikes, nspikes, level_start, nlevels, mode, out, threshold);
}

int p3d_despike_replace(int device, float* section, int ntr, int ns, const int* spikes, size_t nspikes, const int* level_start, int nlevels, int mode, int out,
                        float threshold)
{
    if (ntr < 1 || ns < 1 || !section) return fail(P3D_ERR_INVALID, "bad section");
    if (int rc = check_spikes(spikes, nspikes, level_start, nlevels, ntr, ns)) return rc;
    if (nspikes == 0) return P3D_OK;
    if (int rc = use_device(device)) return rc;
    const size_t nsec = (size_t)ntr * ns * sizeof(float);
    DevBuf da;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMemcpy(da.p, section, nsec, hipMemcpyHostToDevice));
    if (int rc = replace_dev((float*)da.p, ntr, ns, spikes, nspikes, level_start, nlevels, mode, out, threshold)) return rc;
    P3D_TRY(hipMemcpy(section, da.p, nsec, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
