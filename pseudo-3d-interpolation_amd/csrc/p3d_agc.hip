// p3d_agc.hip -- automatic gain control of step 15 (the reference's AGC, functions/signal.py:325-409, applied along the time axis).
// Semantics, restated for a trace x[0 .. nt) with win odd (an even win is made odd by the caller) and h = win / 2:
//   the trace is zero-padded by h samples at both ends; g[t] aggregates the win samples x[t-h .. t+h], pads included:
//     rms:    sqrt(mean(x^2)) -- x^2 rounded to float32 first, as NumPy squares a float32 array
//     mean:   mean(x)
//     median: the element of rank h of the window (win is odd: NumPy's median is that element exactly)
//   g == 0 -> 1; y = x * (1 / g) (a float32 reciprocal and a multiply, like `x *= 1 / g`); squared: y = sign(y) * y^2.
// Layout: time-slow [nt][ntraces] (the slice-major (twt, iline, xline) cube), one lane per trace: every time step is a coalesced row.
//   rms / mean: a running window sum in double precision (add the entering sample, subtract the leaving one) plus a count of the
//               non-zero samples in the window, so a window of zeros gives exactly g = 0 (-> 1) whatever rounding the sum carried.
//               The rounding of the running sum is absolute (about 2^-53 of the largest sum it held), so when the sum falls below 2^-20 of
//               the largest magnitude it held since the last resync, the lane sums its window again directly (one coalesced row per window
//               sample): the relative error stays below nt * 2^-33 however small a window's energy is next to the trace's loudest part.
//   median:     an incremental rank.  The lane keeps the current median m and the counts lt = #{w < m}, eq = #{w == m}; a step removes
//               one sample and adds one, which moves lt and lt + eq by at most one, so at most one move to the next smaller (or larger)
//               distinct window value restores lt <= h < lt + eq.  A move is one scan of the window (one coalesced row per window sample,
//               mostly from L2).  The lane starts from a window of pads only (m = 0, eq = win) h + 1 steps before t = 0, so the first
//               window needs no special case.  No per-lane array: no scratch memory, any odd win (also > nt).
#include <hip/hip_runtime.h>

#include <cmath>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

enum { AGC_RMS = 0, AGC_MEAN = 1, AGC_MEDIAN = 2 };

__device__ __forceinline__ float apply_gain(float v, float g, int squared)
{
    if (g == 0.0f) g = 1.0f;
    const float r = 1.0f / g;
    float y = v * r;
    if (squared) {
        const float s = y > 0.0f ? 1.0f : (y < 0.0f ? -1.0f : y);   // np.sign (0 -> 0, NaN -> NaN)
        y = s * (y * y);
    }
    return y;
}

// rms (kind 0) / mean (kind 1): running window sum in double precision
__global__ void __launch_bounds__(256) agc_sum_kernel(const float* __restrict__ x, float* __restrict__ out, float* __restrict__ gain, long long nt,
                                                      long long ntr, int h, int win, int kind, int squared)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntr) return;
    const float* xj = x + j;
    const bool rms = kind == AGC_RMS;
    double sum = 0.0;
    long long nz = 0;
    // the window of t = 0: samples 0 .. min(h, nt - 1)
    const long long first = (long long)h < nt - 1 ? (long long)h : nt - 1;
    for (long long t = 0; t <= first; ++t) {
        const float v = xj[t * ntr];
        const float q = rms ? v * v : v;
        sum += (double)q;
        nz += v != 0.0f;
    }
    const double inv_win = 1.0 / (double)win;
    double big = fabs(sum);     // largest |sum| since the last direct summation
#pragma unroll 4
    for (long long t = 0; t < nt; ++t) {
        const double mag = fabs(sum);
        if (mag < big * 0x1p-20) {         // cancellation: sum the window of t again
            const long long t0 = t - h < 0 ? 0 : t - h, t1 = t + h >= nt ? nt - 1 : t + h;
            double direct = 0.0;
            for (long long u = t0; u <= t1; ++u) {
                const float v = xj[u * ntr];
                direct += (double)(rms ? v * v : v);
            }
            sum = direct;
            big = fabs(direct);
        } else if (mag > big) {
            big = mag;
        }
        float g = 0.0f;
        if (nz != 0) {
            const float m = (float)(sum * inv_win);
            g = rms ? sqrtf(m) : m;
        }
        const float v = xj[t * ntr];
        out[t * ntr + j] = apply_gain(v, g, squared);
        if (gain) gain[t * ntr + j] = g == 0.0f ? 1.0f : g;
        // slide: sample t - h leaves, sample t + h + 1 enters
        const long long tin = t + h + 1, tout = t - h;
        if (tin < nt) {
            const float a = xj[tin * ntr];
            sum += (double)(rms ? a * a : a);
            nz += a != 0.0f;
        }
        if (tout >= 0) {
            const float b = xj[tout * ntr];
            sum -= (double)(rms ? b * b : b);
            nz -= b != 0.0f;
        }
    }
}

// median: incremental rank (see the header comment)
__global__ void __launch_bounds__(256) agc_median_kernel(const float* __restrict__ x, float* __restrict__ out, float* __restrict__ gain, long long nt,
                                                         long long ntr, int h, int squared)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntr) return;
    const float* xj = x + j;
    const long long win = 2LL * h + 1;
    float m = 0.0f;             // window of pads only: centre c = -h - 1, samples -2h - 1 .. -1
    long long lt = 0, eq = win;
    for (long long c = -h; c < nt; ++c) {
        // slide the centre from c - 1 to c: sample c - h - 1 leaves, sample c + h enters (0 outside the trace)
        const long long tout = c - h - 1, tin = c + h;
        const float a = (tout >= 0 && tout < nt) ? xj[tout * ntr] : 0.0f;
        const float b = (tin >= 0 && tin < nt) ? xj[tin * ntr] : 0.0f;
        if (a < m) --lt; else if (a == m) --eq;
        if (b < m) ++lt; else if (b == m) ++eq;
        // the window of centre c: positions lo .. hi, of which npad lie outside the trace
        const long long lo = c - h, hi = c + h;
        const long long t0 = lo < 0 ? 0 : lo, t1 = hi >= nt ? nt - 1 : hi;
        const long long npad = win - (t1 >= t0 ? t1 - t0 + 1 : 0);
        if ((long long)h < lt) {            // the median is the largest window value below m
            float best = -INFINITY;
            long long cnt = 0;
            if (npad > 0 && 0.0f < m) { best = 0.0f; cnt = npad; }
            for (long long t = t0; t <= t1; ++t) {
                const float w = xj[t * ntr];
                if (w < m) {
                    if (w > best) { best = w; cnt = 1; }
                    else if (w == best) ++cnt;
                }
            }
            m = best;
            lt -= cnt;
            eq = cnt;
        } else if ((long long)h >= lt + eq) {   // ... the smallest window value above m
            float best = INFINITY;
            long long cnt = 0;
            if (npad > 0 && 0.0f > m) { best = 0.0f; cnt = npad; }
            for (long long t = t0; t <= t1; ++t) {
                const float w = xj[t * ntr];
                if (w > m) {
                    if (w < best) { best = w; cnt = 1; }
                    else if (w == best) ++cnt;
                }
            }
            m = best;
            lt += eq;
            eq = cnt;
        }
        if (c >= 0) {
            const float v = xj[c * ntr];
            out[c * ntr + j] = apply_gain(v, m, squared);
            if (gain) gain[c * ntr + j] = m == 0.0f ? 1.0f : m;
        }
    }
}

}  // namespace

extern "C" {

int p3d_agc(int device, const float* x, size_t nt, size_t ntraces, int win, int kind, int squared, float* out, float* gain)
{
    if (!x || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (nt < 1 || ntraces < 1) return fail(P3D_ERR_INVALID, "bad shape (nt %zu, ntraces %zu)", nt, ntraces);
    if (win < 1) return fail(P3D_ERR_INVALID, "window of %d samples", win);
    if (kind != AGC_RMS && kind != AGC_MEAN && kind != AGC_MEDIAN) return fail(P3D_ERR_INVALID, "unknown AGC kind %d", kind);
    if (win % 2 == 0) ++win;
    const int h = win / 2;
    if (int rc = use_device(device)) return rc;

    // traces per chunk: input, output (and gain) of a chunk within half of the free device memory
    size_t free_b = 0, total_b = 0;
    P3D_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t per_trace = nt * sizeof(float) * (gain ? 3 : 2);
    size_t chunk = (free_b / 2) / per_trace;
    if (chunk > ntraces) chunk = ntraces;
    if (chunk >= 256 && chunk < ntraces) chunk -= chunk % 256;
    if (chunk < 1) return fail(P3D_ERR_UNSUPPORTED, "a trace of %zu samples does not fit in device memory", nt);

    DevBuf din, dout, dgain;
    P3D_TRY(hipMalloc(&din.p, sizeof(float) * nt * chunk));
    P3D_TRY(hipMalloc(&dout.p, sizeof(float) * nt * chunk));
    if (gain) P3D_TRY(hipMalloc(&dgain.p, sizeof(float) * nt * chunk));
    const size_t pitch = ntraces * sizeof(float);
    for (size_t j0 = 0; j0 < ntraces; j0 += chunk) {
        const size_t n = ntraces - j0 < chunk ? ntraces - j0 : chunk;   // traces of this chunk: [nt][n] on the device
        const size_t w = n * sizeof(float);
        P3D_TRY(hipMemcpy2D(din.p, w, x + j0, pitch, w, nt, hipMemcpyHostToDevice));
        const unsigned blocks = (unsigned)((n + 255) / 256);
        if (kind == AGC_MEDIAN)
            agc_median_kernel<<<blocks, 256>>>((const float*)din.p, (float*)dout.p, (float*)dgain.p, (long long)nt, (long long)n, h, squared);
        else
            agc_sum_kernel<<<blocks, 256>>>((const float*)din.p, (float*)dout.p, (float*)dgain.p, (long long)nt, (long long)n, h, win, kind, squared);
        P3D_TRY(hipGetLastError());
        P3D_TRY(hipMemcpy2D(out + j0, pitch, dout.p, w, w, nt, hipMemcpyDeviceToHost));
        if (gain) P3D_TRY(hipMemcpy2D(gain + j0, pitch, dgain.p, w, w, nt, hipMemcpyDeviceToHost));
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_agc_dev(int device, const float* x, size_t nt, size_t ntraces, int win, int kind, int squared, float* out, float* gain)
{
    if (!x || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (x == out) return fail(P3D_ERR_INVALID, "x and out must be different buffers");
    if (nt < 1 || ntraces < 1) return fail(P3D_ERR_INVALID, "bad shape (nt %zu, ntraces %zu)", nt, ntraces);
    if (win < 1) return fail(P3D_ERR_INVALID, "window of %d samples", win);
    if (kind != AGC_RMS && kind != AGC_MEAN && kind != AGC_MEDIAN) return fail(P3D_ERR_INVALID, "unknown AGC kind %d", kind);
    if (win % 2 == 0) ++win;
    const int h = win / 2;
    if (int rc = use_device(device)) return rc;
    const unsigned blocks = (unsigned)((ntraces + 255) / 256);
    if (kind == AGC_MEDIAN)
        agc_median_kernel<<<blocks, 256>>>(x, out, gain, (long long)nt, (long long)ntraces, h, squared);
    else
        agc_sum_kernel<<<blocks, 256>>>(x, out, gain, (long long)nt, (long long)ntraces, h, win, kind, squared);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // extern "C"
