// p3d_delrt.hip -- steps 3 and 4 of the workflow (the reference's delrt_correction_segy.py and delrt_padding_segy.py): the device part of the check of
// a DelayRecordingTime at the places where the recording window jumps, and the zero padding that puts all traces of a profile on one time axis.
//
// The section stays in the file's own layout, trace-major [ntr][ns] float32.  Both kernels only copy and compare (max, arg-max), so their results
// are bit-identical to NumPy's.  NaN samples are outside the contract: `>` never holds for them, so a NaN is skipped where NumPy would return it.
//
//   delrt_pad_kernel      out[x][t] = in[x][t - top[x]] for top[x] <= t < top[x] + ns_in, else 0; out is [ntr][ns_out], ns_out >= ns_in.  The access
//                         pattern of static_shift_kernel (which cannot serve: its output trace is as long as its input trace): a thread owns four
//                         consecutive floats of the flat output (16-byte store), 16-byte load where the source is aligned too, scalar loads
//                         otherwise; the tail of the section and the quads that straddle two traces go element by element.
//   delrt_window_kernel   one workgroup (4 wavefronts) per delay change c.  All four waves walk trace ref[c] in chunks of 1024 samples (16-byte loads
//                         from the 16-byte boundary at or below the trace start) for its maximum and the FIRST index that holds it (np.argmax): every
//                         lane keeps its own first maximum, the wave and then the workgroup reduce with the lower index winning a tie.  Then wave w
//                         takes the traces ref[c] - n_traces + j, j = w, w + 4, ... <= 2 n_traces, and walks rows [max(peak - n_samples / 2, 0),
//                         min(peak + n_samples / 2 + 1, ns)) of each in chunks of 256 samples for the plain maximum.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int WAVE = 64;
constexpr int PAD_BS = 256;
constexpr int WIN_WAVES = 4;
constexpr int WIN_BS = WIN_WAVES * WAVE;

__device__ inline float padded(const float* __restrict__ in, const int* __restrict__ top, int ns_in, int ns_out, long long g)
{
    const long long x = g / ns_out;
    const long long t = g - x * ns_out - (long long)top[x];
    return t >= 0 && t < ns_in ? in[x * ns_in + t] : 0.0f;
}

__global__ void __launch_bounds__(PAD_BS) delrt_pad_kernel(const float* __restrict__ in, const int* __restrict__ top, int ns_in, int ns_out, long long total,
                                                           float* __restrict__ out)
{
    const long long g = ((long long)blockIdx.x * PAD_BS + threadIdx.x) * 4;
    if (g >= total) return;
    const long long x = g / ns_out;
    const int t = (int)(g - x * ns_out);
    if (g + 3 < total && t + 3 < ns_out) {                         // four samples of one output trace
        const long long src = (long long)t - (long long)top[x];
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (src >= 0 && src + 3 < ns_in) {
            const float* p = in + x * ns_in + src;
            if (((x * ns_in + src) & 3) == 0) {
                r = *reinterpret_cast<const float4*>(p);
            } else {
                r = make_float4(p[0], p[1], p[2], p[3]);
            }
        } else if (src > -4 && src < ns_in) {
            const float* p = in + x * ns_in;
            if (src >= 0) r.x = p[src];
            if (src + 1 >= 0 && src + 1 < ns_in) r.y = p[src + 1];
            if (src + 2 >= 0 && src + 2 < ns_in) r.z = p[src + 2];
            if (src + 3 >= 0 && src + 3 < ns_in) r.w = p[src + 3];
        }
        *reinterpret_cast<float4*>(out + g) = r;
    } else {
        for (int k = 0; k < 4 && g + k < total; ++k) out[g + k] = padded(in, top, ns_in, ns_out, g + k);
    }
}

// the four floats at flat index g (a multiple of 4) ... g + 3 of the section; lanes outside [lo, hi) are marked in `inside`
__device__ inline float4 load4(const float* __restrict__ a, long long g, long long lo, long long hi, long long total, bool inside[4])
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) inside[k] = g + k >= lo && g + k < hi;
    if (g + 3 < lo || g >= hi) return v;
    if (g + 3 < total) {
        v = *reinterpret_cast<const float4*>(a + g);
    } else {
        if (g < total) v.x = a[g];
        if (g + 1 < total) v.y = a[g + 1];
        if (g + 2 < total) v.z = a[g + 2];
    }
    return v;
}

// (value, index) with the larger value, the lower index among equal values
__device__ inline void take(float& bv, int& bi, float v, int i)
{
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

__global__ void __launch_bounds__(WIN_BS) delrt_window_kernel(const float* __restrict__ a, int ntr, int ns, const int* __restrict__ ref, int n_traces,
                                                              int n_samples, int* __restrict__ peak_idx, float* __restrict__ peak_val,
                                                              float* __restrict__ maxima)
{
    __shared__ float wave_val[WIN_WAVES];
    __shared__ int wave_idx[WIN_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int width = 2 * n_traces + 1;
    const long long total = (long long)ntr * ns;
    const int r = ref[c];
    if (r - n_traces < 0 || r + n_traces >= ntr) {                 // refused on the host; never a read outside the section here
        if (tid == 0) {
            peak_idx[c] = -1;
            peak_val[c] = -INFINITY;
        }
        for (int j = tid; j < width; j += WIN_BS) maxima[(long long)c * width + j] = -INFINITY;
        return;
    }

    // the reference trace: its maximum and the first index that holds it
    float bv = -INFINITY;
    int bi = INT_MAX;
    {
        const long long g0 = (long long)r * ns, base = g0 & ~3ll, hi = g0 + ns;
        for (long long q = base + 4 * tid; q < hi; q += 4 * WIN_BS) {
            bool in[4];
            const float4 v = load4(a, q, g0, hi, total, in);
            const int i = (int)(q - g0);
            if (in[0]) take(bv, bi, v.x, i);
            if (in[1]) take(bv, bi, v.y, i + 1);
            if (in[2]) take(bv, bi, v.z, i + 2);
            if (in[3]) take(bv, bi, v.w, i + 3);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        take(bv, bi, ov, oi);
    }
    if (lane == 0) {
        wave_val[wave] = bv;
        wave_idx[wave] = bi;
    }
    __syncthreads();
    bv = wave_val[0];
    bi = wave_idx[0];
#pragma unroll
    for (int w = 1; w < WIN_WAVES; ++w) take(bv, bi, wave_val[w], wave_idx[w]);
    if (bi == INT_MAX) bi = 0;                                     // a trace of NaNs (outside the contract): the window stays inside the trace
    if (tid == 0) {
        peak_idx[c] = bi;
        peak_val[c] = bv;
    }

    // the window around the peak row in every trace of the subset
    const int half = n_samples / 2;
    const int lo = max(bi - half, 0), hi_row = min(bi + half + 1, ns);
    for (int j = wave; j < width; j += WIN_WAVES) {
        const long long t0 = (long long)(r - n_traces + j) * ns;
        const long long g0 = t0 + lo, hi = t0 + hi_row, base = g0 & ~3ll;
        float m = -INFINITY;
        for (long long q = base + 4 * lane; q < hi; q += 4 * WAVE) {
            bool in[4];
            const float4 v = load4(a, q, g0, hi, total, in);
            if (in[0] && v.x > m) m = v.x;
            if (in[1] && v.y > m) m = v.y;
            if (in[2] && v.z > m) m = v.z;
            if (in[3] && v.w > m) m = v.w;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float o = __shfl_xor(m, d);
            if (o > m) m = o;
        }
        if (lane == 0) maxima[(long long)c * width + j] = m;
    }
}

int check_pad_shape(int ntr, int ns_in, int ns_out)
{
    if (ntr < 1 || ns_in < 1) return fail(P3D_ERR_INVALID, "bad section shape (%d traces, %d samples)", ntr, ns_in);
    if (ns_out < ns_in) return fail(P3D_ERR_INVALID, "padded traces of %d samples cannot hold traces of %d samples", ns_out, ns_in);
    return P3D_OK;
}

int check_top(const int* top, int ntr, int ns_in, int ns_out)
{
    for (int x = 0; x < ntr; ++x) {
        if (top[x] < 0) return fail(P3D_ERR_INVALID, "trace %d: %d samples of top padding", x, top[x]);
        if ((long long)top[x] + ns_in > ns_out)
            return fail(P3D_ERR_INVALID, "trace %d: %d samples of top padding and %d samples do not fit padded traces of %d samples", x, top[x], ns_in, ns_out);
    }
    return P3D_OK;
}

int pad_dev(const float* in, int ntr, int ns_in, int ns_out, const int* top, float* out)
{
    if (!in || !top || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (in == out) return fail(P3D_ERR_INVALID, "the padding needs separate input and output buffers");
    if (((uintptr_t)in | (uintptr_t)out) & 15) return fail(P3D_ERR_INVALID, "the sections must start at 16-byte boundaries");
    const long long total = (long long)ntr * ns_out, quads = (total + 3) / 4, blocks = (quads + PAD_BS - 1) / PAD_BS;
    if (blocks > 0x7fffffffll) return fail(P3D_ERR_UNSUPPORTED, "section too large for one launch (%lld workgroups)", blocks);
    delrt_pad_kernel<<<(unsigned)blocks, PAD_BS, 0, 0>>>(in, top, ns_in, ns_out, total, out);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int check_windows(int ntr, int ns, int m, int n_traces, int n_samples)
{
    if (ntr < 1 || ns < 1) return fail(P3D_ERR_INVALID, "bad section shape (%d traces, %d samples)", ntr, ns);
    if (m < 0) return fail(P3D_ERR_INVALID, "%d delay changes", m);
    if (n_traces < 1) return fail(P3D_ERR_INVALID, "the comparison window needs at least 1 trace to either side, got %d", n_traces);
    if (n_samples < 1) return fail(P3D_ERR_INVALID, "the comparison window needs at least 1 sample, got %d", n_samples);
    if (2ll * n_traces + 1 > ntr) return fail(P3D_ERR_INVALID, "a window of %lld traces does not fit a section of %d traces", 2ll * n_traces + 1, ntr);
    return P3D_OK;
}

// ref: HOST; the section and the three results: DEVICE
int windows_dev(const float* a, int ntr, int ns, const int* ref, int m, int n_traces, int n_samples, int* peak_idx, float* peak_val, float* maxima)
{
    if (m == 0) return P3D_OK;
    if (!a || !ref || !peak_idx || !peak_val || !maxima) return fail(P3D_ERR_INVALID, "NULL buffer");
    if ((uintptr_t)a & 15) return fail(P3D_ERR_INVALID, "the section must start at a 16-byte boundary");
    for (int c = 0; c < m; ++c)
        if (ref[c] < n_traces || ref[c] > ntr - 1 - n_traces)
            return fail(P3D_ERR_INVALID, "change %d: trace %d has fewer than %d neighbours to either side in a section of %d traces", c, ref[c], n_traces, ntr);
    DevBuf dref;
    P3D_TRY(hipMalloc(&dref.p, (size_t)m * sizeof(int)));
    P3D_TRY(hipMemcpy(dref.p, ref, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    delrt_window_kernel<<<(unsigned)m, WIN_BS, 0, 0>>>(a, ntr, ns, (const int*)dref.p, n_traces, n_samples, peak_idx, peak_val, maxima);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());                               // dref is freed on return
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_delrt_pad_dev(int device, const float* in_dev, int ntr, int ns_in, int ns_out, const int* top_dev, float* out_dev)
{
    if (int rc = check_pad_shape(ntr, ns_in, ns_out)) return rc;
    if (!in_dev || !top_dev || !out_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    std::vector<int> top(ntr);                                     // one int per trace comes back for the check: nothing is launched on a bad table
    P3D_TRY(hipMemcpy(top.data(), top_dev, (size_t)ntr * sizeof(int), hipMemcpyDeviceToHost));
    if (int rc = check_top(top.data(), ntr, ns_in, ns_out)) return rc;
    if (int rc = pad_dev(in_dev, ntr, ns_in, ns_out, top_dev, out_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_delrt_pad(int device, const float* section, int ntr, int ns_in, int ns_out, const int* top, float* out)
{
    if (int rc = check_pad_shape(ntr, ns_in, ns_out)) return rc;
    if (!section || !top || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = check_top(top, ntr, ns_in, ns_out)) return rc;
    if (int rc = use_device(device)) return rc;
    const size_t nin = (size_t)ntr * ns_in * sizeof(float), nout = (size_t)ntr * ns_out * sizeof(float), nint = (size_t)ntr * sizeof(int);
    DevBuf da, dt, dout;
    P3D_TRY(hipMalloc(&da.p, nin));
    P3D_TRY(hipMalloc(&dt.p, nint));
    P3D_TRY(hipMalloc(&dout.p, nout));
    P3D_TRY(hipMemcpy(da.p, section, nin, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dt.p, top, nint, hipMemcpyHostToDevice));
    if (int rc = pad_dev((const float*)da.p, ntr, ns_in, ns_out, (const int*)dt.p, (float*)dout.p)) return rc;
    P3D_TRY(hipMemcpy(out, dout.p, nout, hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_delrt_windows_dev(int device, const float* section_dev, int ntr, int ns, const int* ref, int m, int n_traces, int n_samples, int* peak_idx_dev,
                          float* peak_val_dev, float* maxima_dev)
{
    if (int rc = check_windows(ntr, ns, m, n_traces, n_samples)) return rc;
    if (int rc = use_device(device)) return rc;
    return windows_dev(section_dev, ntr, ns, ref, m, n_traces, n_samples, peak_idx_dev, peak_val_dev, maxima_dev);
}

int p3d_delrt_windows(int device, const float* subsets, int m, int ns, int n_traces, int n_samples, int* peak_idx, float* peak_val, float* maxima)
{
    if (m == 0) return P3D_OK;
    if (n_traces < 1) return fail(P3D_ERR_INVALID, "the comparison window needs at least 1 trace to either side, got %d", n_traces);
    const long long width = 2ll * n_traces + 1;
    if (m < 0 || width * m > INT_MAX) return fail(P3D_ERR_INVALID, "%d delay changes of %lld traces each", m, width);
    const int ntr = (int)(width * m);
    if (int rc = check_windows(ntr, ns, m, n_traces, n_samples)) return rc;
    if (!subsets || !peak_idx || !peak_val || !maxima) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    std::vector<int> ref(m);
    for (int c = 0; c < m; ++c) ref[c] = c * (int)width + n_traces;   // the packed subsets are a section of their own
    const size_t nsec = (size_t)ntr * ns * sizeof(float), nmax = (size_t)ntr * sizeof(float);
    DevBuf da, di, dv, dm;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&di.p, (size_t)m * sizeof(int)));
    P3D_TRY(hipMalloc(&dv.p, (size_t)m * sizeof(float)));
    P3D_TRY(hipMalloc(&dm.p, nmax));
    P3D_TRY(hipMemcpy(da.p, subsets, nsec, hipMemcpyHostToDevice));
    if (int rc = windows_dev((const float*)da.p, ntr, ns, ref.data(), m, n_traces, n_samples, (int*)di.p, (float*)dv.p, (float*)dm.p)) return rc;
    P3D_TRY(hipMemcpy(peak_idx, di.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(peak_val, dv.p, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(maxima, dm.p, nmax, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
