// p3d_static.hip -- step 5 of the workflow (the reference's static_correction_segy.py): the seafloor is found in every trace of a 2-D section
// (STA/LTA energy ratio, first crossing of a global threshold, a pick among the n largest amplitudes of a window around the filtered crossing) and
// the traces are shifted by their static.
//
// The section stays in the file's own layout, trace-major [ntr][ns] float32.  In the three detection kernels one wavefront owns one trace and walks
// it in chunks of 256 samples, every lane with one 16-byte load: the walk starts at the 16-byte boundary at or below the first sample of the
// trace's valid slice (whatever ns and the slice start are), samples outside the slice count as zeros.
//
//   static_scan_kernel     first non-zero sample of the trace (-1: a zero trace); stops at the first chunk that holds one.
//   static_stalta_kernel   the running sum c[i] of a^2 in DOUBLE (a wave scan per chunk; the squares of float32 values are exact in double), kept
//                          in an LDS ring that reaches nlta samples back, so sta = (c[i] - c[i - nsta]) / nsta and lta = (c[i] - c[i - nlta]) / nlta
//                          are formed the way the reference forms them and the ratio is never stored.  PASS 0: the maximum of the ratio over rows
//                          nlta ... 2 nlta - 1 (it reads no further); PASS 1: the first row whose ratio exceeds the threshold (it stops there).
//                          Both passes run the same arithmetic on the same chunks, so the row that set the threshold does not exceed it.
//   static_peak_kernel     the window base - win ... base + win clipped to the slice, 64 K samples in K registers per lane; a sample is among the
//                          n largest if fewer than n others beat it (larger, or equal at a lower position); the wave's ballots are the bitmap of
//                          the chosen positions, from which every lane derives the reference's leading group, then an arg-max over that group.
//   static_shift_kernel    out[x][t] = in[x][t - s[x]] or 0; a thread owns four consecutive floats of the flat section (16-byte store, 16-byte
//                          load where the source is aligned too).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int WAVE = 64;
constexpr int CHUNK = 4 * WAVE;                 // samples per step of a wave
constexpr int MAXWIN = P3D_STATIC_MAX_WIN;
constexpr int MAXNLTA = P3D_STATIC_MAX_NLTA;
constexpr int SHIFT_BS = 256;

// the valid slice of trace x: samples [g0, g0 + n) of the flat section
struct Slice {
    long long g0;
    int n;
};

__device__ inline Slice trace_slice(int x, int ns, const int* __restrict__ first, int padded, int nvalid)
{
    int start = 0, n = ns;
    if (padded) {
        start = max(first[x], 0);
        n = max(min(nvalid, ns - start), 0);
    }
    return Slice{(long long)x * ns + start, n};
}

// the four floats at flat index g (a multiple of 4) ... g + 3, zeros outside [lo, hi)
__device__ inline float4 load4(const float* __restrict__ a, long long g, long long lo, long long hi, long long total)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (g + 3 < lo || g >= hi) return v;
    if (g + 3 < total) {
        v = *reinterpret_cast<const float4*>(a + g);
    } else {
        if (g < total) v.x = a[g];
        if (g + 1 < total) v.y = a[g + 1];
        if (g + 2 < total) v.z = a[g + 2];
    }
    if (g < lo || g >= hi) v.x = 0.0f;
    if (g + 1 < lo || g + 1 >= hi) v.y = 0.0f;
    if (g + 2 < lo || g + 2 >= hi) v.z = 0.0f;
    if (g + 3 < lo || g + 3 >= hi) v.w = 0.0f;
    return v;
}

__device__ inline int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

__global__ void __launch_bounds__(WAVE) static_scan_kernel(const float* __restrict__ a, int ns, long long total, int* __restrict__ first)
{
    const int x = blockIdx.x, lane = threadIdx.x;
    const long long g0 = (long long)x * ns, base = g0 & ~3ll, hi = g0 + ns;
    int found = INT_MAX;
    for (long long c = base; c < hi; c += CHUNK) {
        const long long g = c + 4 * lane;
        const float4 v = load4(a, g, g0, hi, total);
        int k = INT_MAX;
        if (v.w != 0.0f) k = 3;
        if (v.z != 0.0f) k = 2;
        if (v.y != 0.0f) k = 1;
        if (v.x != 0.0f) k = 0;
        if (k != INT_MAX) k += (int)(g - g0);
        found = wave_min(k);
        if (found != INT_MAX) break;
    }
    if (lane == 0) first[x] = found == INT_MAX ? -1 : found;
}

// PASS 0: peak[x] = max of the ratio over rows nlta ... 2 nlta - 1; PASS 1: cross[x] = first row with ratio > thr (0 when there is none)
template <int PASS>
__global__ void __launch_bounds__(WAVE) static_stalta_kernel(const float* __restrict__ a, int ns, long long total, const int* __restrict__ first, int padded,
                                                             int nvalid, int nsta, int nlta, int ring_mask, double thr, double* __restrict__ peak,
                                                             int* __restrict__ cross)
{
    extern __shared__ double ring[];   // c at virtual position j: ring[j & ring_mask], the last nlta + 2 CHUNK positions are alive
    const int x = blockIdx.x, lane = threadIdx.x;
    if (first[x] < 0) {                // a zero trace: left out of the detection
        if (lane == 0) {
            if (PASS == 0) peak[x] = 0.0;
            else cross[x] = 0;
        }
        return;
    }
    const Slice sl = trace_slice(x, ns, first, padded, nvalid);
    const long long base = sl.g0 & ~3ll, hi = sl.g0 + sl.n;
    const int head = (int)(sl.g0 - base);                      // virtual position j = i + head
    const int rows = PASS == 0 ? min(sl.n, 2 * nlta) : sl.n;   // rows that matter
    double carry = 0.0, best = 0.0;
    int hit = INT_MAX;
    for (int j0 = 0; j0 < rows + head; j0 += CHUNK) {
        const int j = j0 + 4 * lane;
        const float4 v = load4(a, base + j, sl.g0, hi, total);
        double s[4] = {(double)v.x * (double)v.x, (double)v.y * (double)v.y, (double)v.z * (double)v.z, (double)v.w * (double)v.w};
        s[1] += s[0];
        s[2] += s[1];
        s[3] += s[2];
        double incl = s[3];                                    // inclusive scan of the lanes' totals
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const double up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const double left = __shfl_up(incl, 1);
        const double before = lane == 0 ? carry : carry + left;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] += before;
            ring[(j + k) & ring_mask] = s[k];
        }
        carry = __shfl(incl, WAVE - 1) + carry;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = j + k - head;
            if (i < 0 || i >= rows) continue;
            if (PASS == 0 && i < nlta) continue;
            double sta = s[k], lta = s[k];
            if (i >= nsta) sta -= ring[(j + k - nsta) & ring_mask];
            if (i >= nlta) lta -= ring[(j + k - nlta) & ring_mask];
            sta /= (double)nsta;
            lta /= (double)nlta;
            if (i < nlta - 1) sta = 0.0;
            const double ratio = lta != 0.0 ? sta / lta : 0.0;
            if (PASS == 0) best = fmax(best, ratio);
            else if (ratio > thr) hit = min(hit, i);
        }
        if (PASS == 1) {
            hit = wave_min(hit);
            if (hit != INT_MAX) break;
        }
    }
    if (PASS == 0) {
        // the ratio is >= 0 (sums of squares), so 0 is the neutral element; a trace without rows nlta ... yields 0
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) best = fmax(best, __shfl_xor(best, d));
        if (lane == 0) peak[x] = best;
    } else if (lane == 0) {
        cross[x] = hit == INT_MAX ? 0 : hit;
    }
}

// K: registers per lane, the window holds up to 64 K samples
template <int K>
__global__ void __launch_bounds__(WAVE) static_peak_kernel(const float* __restrict__ a, int ns, const int* __restrict__ first, int padded, int nvalid,
                                                           const int* __restrict__ base_idx, int win, int nlargest, int* __restrict__ out)
{
    __shared__ float w[WAVE * K];
    __shared__ unsigned long long chosen[K];
    const int x = blockIdx.x, lane = threadIdx.x;
    if (first[x] < 0) {
        if (lane == 0) out[x] = -1;
        return;
    }
    const Slice sl = trace_slice(x, ns, first, padded, nvalid);
    const int b = max(min(base_idx[x], sl.n + win), -win - 1);
    const int lo = max(b - win, 0), hi = min(b + win, sl.n - 1);   // clipped to the slice (the reference raises there)
    const int L = hi - lo + 1;
    if (L <= 0 || L > WAVE * K) {                                  // refused on the host; never a read outside the section here
        if (lane == 0) out[x] = -1;
        return;
    }
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int p = lane + WAVE * k;
        v[k] = p < L ? a[sl.g0 + lo + p] : -INFINITY;
        w[p] = v[k];
    }
    __syncthreads();
    int rank[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rank[k] = 0;
    for (int q = 0; q < L; ++q) {
        const float u = w[q];                                      // one address for the wave: a broadcast
#pragma unroll
        for (int k = 0; k < K; ++k) rank[k] += (u > v[k] || (u == v[k] && q < lane + WAVE * k)) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long word = __ballot(lane + WAVE * k < L && rank[k] < nlargest);
        if (lane == 0) chosen[k] = word;
    }
    __syncthreads();
    // the chosen positions in ascending order p[0] < p[1] < ...; i = the first index with p[i + 1] - p[i] > 1.  The reference keeps p[:i]
    // (p[:1] when i = 0, all of them when there is no such gap): positions [p0, q)
    int p0 = -1, count = 0;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        const unsigned long long word = chosen[k];
        count += __popcll(word);
        if (word) p0 = WAVE * k + __ffsll((long long)word) - 1;
    }
    p0 = max(p0, 0);
    int e = p0;
    while (e < L && ((chosen[e >> 6] >> (e & 63)) & 1ull)) ++e;   // first position after the leading run
    const int q = count > e - p0 ? max(e - 1, p0 + 1) : e;
    float bv = -INFINITY;
    int bp = INT_MAX;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int p = lane + WAVE * k;
        if (p >= p0 && p < q && (v[k] > bv || bp == INT_MAX)) {   // ascending p: a later equal value does not replace
            bv = v[k];
            bp = p;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int op = __shfl_xor(bp, d);
        if (op != INT_MAX && (bp == INT_MAX || ov > bv || (ov == bv && op < bp))) {
            bv = ov;
            bp = op;
        }
    }
    if (lane == 0) out[x] = lo + bp;
}

__device__ inline float shifted(const float* __restrict__ in, const int* __restrict__ shift, int ns, long long g)
{
    const long long x = g / ns;
    const long long t = g - x * ns - (long long)shift[x];
    return t >= 0 && t < ns ? in[x * ns + t] : 0.0f;
}

__global__ void __launch_bounds__(SHIFT_BS) static_shift_kernel(const float* __restrict__ in, const int* __restrict__ shift, int ns, long long total,
                                                                float* __restrict__ out)
{
    const long long g = ((long long)blockIdx.x * SHIFT_BS + threadIdx.x) * 4;
    if (g >= total) return;
    const long long x = g / ns;
    const int t = (int)(g - x * ns);
    if (g + 3 < total && t + 3 < ns) {                             // four samples of one trace
        const long long src = (long long)t - (long long)shift[x];
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (src >= 0 && src + 3 < ns) {
            const float* p = in + x * ns + src;
            if (((x * ns + src) & 3) == 0) {
                r = *reinterpret_cast<const float4*>(p);
            } else {
                r = make_float4(p[0], p[1], p[2], p[3]);
            }
        } else if (src > -4 && src < ns) {
            const float* p = in + x * ns;
            if (src >= 0) r.x = p[src];
            if (src + 1 >= 0 && src + 1 < ns) r.y = p[src + 1];
            if (src + 2 >= 0 && src + 2 < ns) r.z = p[src + 2];
            if (src + 3 >= 0 && src + 3 < ns) r.w = p[src + 3];
        }
        *reinterpret_cast<float4*>(out + g) = r;
    } else {
        for (int k = 0; k < 4 && g + k < total; ++k) out[g + k] = shifted(in, shift, ns, g + k);
    }
}

int check_section(int ntr, int ns)
{
    if (ntr < 1 || ns < 1) return fail(P3D_ERR_INVALID, "bad section shape (%d traces, %d samples)", ntr, ns);
    return P3D_OK;
}

int check_slice(int ns, int padded, int nvalid)
{
    if (padded && (nvalid < 1 || nvalid > ns)) return fail(P3D_ERR_INVALID, "%d valid samples do not fit traces of %d samples", nvalid, ns);
    return P3D_OK;
}

int check_stalta(int ntr, int ns, int padded, int nvalid, int nsta, int nlta)
{
    if (int rc = check_section(ntr, ns)) return rc;
    if (int rc = check_slice(ns, padded, nvalid)) return rc;
    if (nsta < 1 || nlta < 1) return fail(P3D_ERR_INVALID, "the STA / LTA windows must be at least 1 sample long (nsta %d, nlta %d)", nsta, nlta);
    if (nsta > nlta) return fail(P3D_ERR_INVALID, "the short window (%d samples) is longer than the long one (%d)", nsta, nlta);
    if (nlta > MAXNLTA) return fail(P3D_ERR_UNSUPPORTED, "long windows of up to %d samples are supported, got %d", MAXNLTA, nlta);
    return P3D_OK;
}

int check_peak(int ntr, int ns, int padded, int nvalid, int win, int n)
{
    if (int rc = check_section(ntr, ns)) return rc;
    if (int rc = check_slice(ns, padded, nvalid)) return rc;
    if (win < 1) return fail(P3D_ERR_INVALID, "the search window must reach at least 1 sample to either side, got %d", win);
    if (win > MAXWIN) return fail(P3D_ERR_UNSUPPORTED, "search windows of up to +- %d samples are supported, got %d", MAXWIN, win);
    if (n < 1) return fail(P3D_ERR_INVALID, "at least 1 amplitude must be selected, got %d", n);
    if (n > 2 * win + 1) return fail(P3D_ERR_UNSUPPORTED, "a window of %d samples cannot give %d amplitudes", 2 * win + 1, n);
    return P3D_OK;
}

int ring_size(int nlta)
{
    int r = 1024;
    while (r < nlta + 2 * CHUNK) r <<= 1;
    return r;
}

int scan_dev(const float* a, int ntr, int ns, int* first)
{
    if (!a || !first) return fail(P3D_ERR_INVALID, "NULL buffer");
    static_scan_kernel<<<(unsigned)ntr, WAVE, 0, 0>>>(a, ns, (long long)ntr * ns, first);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int stalta_dev(int pass, const float* a, int ntr, int ns, const int* first, int padded, int nvalid, int nsta, int nlta, double thr, double* peak, int* cross)
{
    if (!a || !first || (pass == 0 ? !peak : !cross)) return fail(P3D_ERR_INVALID, "NULL buffer");
    const int r = ring_size(nlta);
    const size_t lds = (size_t)r * sizeof(double);
    const long long total = (long long)ntr * ns;
    if (pass == 0) static_stalta_kernel<0><<<(unsigned)ntr, WAVE, lds, 0>>>(a, ns, total, first, padded, nvalid, nsta, nlta, r - 1, thr, peak, cross);
    else static_stalta_kernel<1><<<(unsigned)ntr, WAVE, lds, 0>>>(a, ns, total, first, padded, nvalid, nsta, nlta, r - 1, thr, peak, cross);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int peak_dev(const float* a, int ntr, int ns, const int* first, int padded, int nvalid, const int* base, int win, int n, int* out)
{
    if (!a || !first || !base || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    const int L = 2 * win + 1;
    if (L <= 64) static_peak_kernel<1><<<(unsigned)ntr, WAVE, 0, 0>>>(a, ns, first, padded, nvalid, base, win, n, out);
    else if (L <= 128) static_peak_kernel<2><<<(unsigned)ntr, WAVE, 0, 0>>>(a, ns, first, padded, nvalid, base, win, n, out);
    else if (L <= 256) static_peak_kernel<4><<<(unsigned)ntr, WAVE, 0, 0>>>(a, ns, first, padded, nvalid, base, win, n, out);
    else static_peak_kernel<8><<<(unsigned)ntr, WAVE, 0, 0>>>(a, ns, first, padded, nvalid, base, win, n, out);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int shift_dev(const float* in, int ntr, int ns, const int* shift, float* out)
{
    if (!in || !shift || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (in == out) return fail(P3D_ERR_INVALID, "the shift needs separate input and output buffers");
    const long long total = (long long)ntr * ns, quads = (total + 3) / 4, blocks = (quads + SHIFT_BS - 1) / SHIFT_BS;
    if (blocks > 0x7fffffffll) return fail(P3D_ERR_UNSUPPORTED, "section too large for one launch (%lld workgroups)", blocks);
    static_shift_kernel<<<(unsigned)blocks, SHIFT_BS, 0, 0>>>(in, shift, ns, total, out);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_static_scan_dev(int device, const float* section_dev, int ntr, int ns, int* first_dev)
{
    if (int rc = check_section(ntr, ns)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = scan_dev(section_dev, ntr, ns, first_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_static_stalta_max_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, int nsta, int nlta,
                              double* peak_dev)
{
    if (int rc = check_stalta(ntr, ns, padded, nvalid, nsta, nlta)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = stalta_dev(0, section_dev, ntr, ns, first_dev, padded, nvalid, nsta, nlta, 0.0, peak_dev, nullptr)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_static_stalta_cross_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, int nsta, int nlta,
                                double threshold, int* cross_dev)
{
    if (int rc = check_stalta(ntr, ns, padded, nvalid, nsta, nlta)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = stalta_dev(1, section_dev, ntr, ns, first_dev, padded, nvalid, nsta, nlta, threshold, nullptr, cross_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_static_peak_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, const int* base_dev, int win,
                        int n, int* peak_idx_dev)
{
    if (int rc = check_peak(ntr, ns, padded, nvalid, win, n)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = peak_dev(section_dev, ntr, ns, first_dev, padded, nvalid, base_dev, win, n, peak_idx_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_static_shift_dev(int device, const float* in_dev, int ntr, int ns, const int* shift_on_dev, float* out_dev)
{
    if (int rc = check_section(ntr, ns)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = shift_dev(in_dev, ntr, ns, shift_on_dev, out_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_static_detect(int device, const float* section, int ntr, int ns, int padded, int nvalid, int nsta, int nlta, double* threshold, int* first,
                      int* cross)
{
    if (int rc = check_stalta(ntr, ns, padded, nvalid, nsta, nlta)) return rc;
    if (!section || !threshold || !first || !cross) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nsec = (size_t)ntr * ns * sizeof(float);
    DevBuf da, df, dp, dc;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&df.p, (size_t)ntr * sizeof(int)));
    P3D_TRY(hipMalloc(&dp.p, (size_t)ntr * sizeof(double)));
    P3D_TRY(hipMalloc(&dc.p, (size_t)ntr * sizeof(int)));
    P3D_TRY(hipMemcpy(da.p, section, nsec, hipMemcpyHostToDevice));
    if (int rc = scan_dev((const float*)da.p, ntr, ns, (int*)df.p)) return rc;
    P3D_TRY(hipMemcpy(first, df.p, (size_t)ntr * sizeof(int), hipMemcpyDeviceToHost));
    if (std::isnan(*threshold)) {   // the reference's default: the largest ratio of rows nlta ... 2 nlta - 1 over the live traces
        std::vector<double> peak(ntr);
        if (int rc = stalta_dev(0, (const float*)da.p, ntr, ns, (const int*)df.p, padded, nvalid, nsta, nlta, 0.0, (double*)dp.p, nullptr)) return rc;
        P3D_TRY(hipMemcpy(peak.data(), dp.p, (size_t)ntr * sizeof(double), hipMemcpyDeviceToHost));
        double thr = 0.0;
        for (int x = 0; x < ntr; ++x)
            if (first[x] >= 0) thr = std::max(thr, peak[x]);
        *threshold = thr;
    }
    if (int rc = stalta_dev(1, (const float*)da.p, ntr, ns, (const int*)df.p, padded, nvalid, nsta, nlta, *threshold, nullptr, (int*)dc.p)) return rc;
    P3D_TRY(hipMemcpy(cross, dc.p, (size_t)ntr * sizeof(int), hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_static_peak(int device, const float* section, int ntr, int ns, const int* first, int padded, int nvalid, const int* base, int win, int n,
                    int* peak_idx)
{
    if (int rc = check_peak(ntr, ns, padded, nvalid, win, n)) return rc;
    if (!section || !first || !base || !peak_idx) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nsec = (size_t)ntr * ns * sizeof(float), nint = (size_t)ntr * sizeof(int);
    DevBuf da, df, db, dout;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&df.p, nint));
    P3D_TRY(hipMalloc(&db.p, nint));
    P3D_TRY(hipMalloc(&dout.p, nint));
    P3D_TRY(hipMemcpy(da.p, section, nsec, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(df.p, first, nint, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(db.p, base, nint, hipMemcpyHostToDevice));
    if (int rc = peak_dev((const float*)da.p, ntr, ns, (const int*)df.p, padded, nvalid, (const int*)db.p, win, n, (int*)dout.p)) return rc;
    P3D_TRY(hipMemcpy(peak_idx, dout.p, nint, hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_static_shift(int device, const float* section, int ntr, int ns, const int* shift, float* out)
{
    if (int rc = check_section(ntr, ns)) return rc;
    if (!section || !shift || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nsec = (size_t)ntr * ns * sizeof(float), nint = (size_t)ntr * sizeof(int);
    DevBuf da, ds, dout;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&ds.p, nint));
    P3D_TRY(hipMalloc(&dout.p, nsec));
    P3D_TRY(hipMemcpy(da.p, section, nsec, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(ds.p, shift, nint, hipMemcpyHostToDevice));
    if (int rc = shift_dev((const float*)da.p, ntr, ns, (const int*)ds.p, (float*)dout.p)) return rc;
    P3D_TRY(hipMemcpy(out, dout.p, nsec, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
