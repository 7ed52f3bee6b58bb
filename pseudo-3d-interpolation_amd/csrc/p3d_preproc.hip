// p3d_preproc.hip -- trace-wise operations of step 11 (cube pre-processing): trace balancing, time-variant gain, zero-phase
// Butterworth filtering (sosfiltfilt), polyphase resampling (upfirdn), FFT resampling and the trace envelope.
// Layout: every buffer is a DEVICE float32 matrix [nt][ntraces] (time-slow, the slice-major (twt, iline, xline) cube), so lane j of
// a wavefront reads trace j and every time step is a coalesced row.  Coefficient tables (gain curves, filter sections, FIR taps,
// spectral factors) are small host arrays designed in NumPy (functions/filter.py, functions/signal.py) and uploaded per call.
// Callers that hold cubes larger than the device memory split them into chunks of traces (every operation is per trace).
//
//   gain (pre_gain_kernel): one elementwise pass over a contiguous range of the stages below, in the reference's order
//        (functions/signal.py gain): bias, tpow, epow, gpow | AGC | clip, pclip, nclip | qclip, linear, pgc | norm_rms, scale.
//        A '|' is where a per-trace quantity must be known first: the AGC (p3d_agc_dev), the quantile of |x| (pre_quantile_kernel)
//        or the rms (pre_reduce_kernel); the host splits the pass there.  float32 arithmetic as NumPy does it on a float32 array:
//        the tpow / epow / linear curves are float64 (a float64 product rounded to float32), pgc is float32.
//   balance: pre_reduce_kernel (rms or max |x| per trace, 0 -> 1) and the division stage of pre_gain_kernel (12 B/pt).
//   sosfiltfilt (sos_*_kernel<NS>): scipy's odd extension (formed in float32, as scipy forms it on a float32 array), the forward
//        cascade from zi * ext[0], the backward cascade from zi * y[-1], transposed direct form II in DOUBLE precision; the
//        sections' state lives in registers (the section loop is unrolled for NS <= 8).  Longer cascades run in groups of 8
//        sections, one pass per group (exact: sosfilt_zi already carries the gain of the earlier sections); the signal between
//        the groups stays in DOUBLE (a float32 hand-off after every group cost 1.7e-5 rel-L2 at 17 band-pass sections).
//   upfirdn (pre_upfirdn_kernel): one thread per (output sample, trace), taps in double, the window of scipy's resample_poly.
//   spectral (resample / envelope): real -> complex, the any-length line FFT (axis0_fft, p3d_api.hip), a bin remap with factors,
//        the inverse FFT at the output length, real part (resample) or modulus (envelope).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"
#include "p3d_internal.hpp"

using p3d::c32;
using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int FFT_MAX_N = 10240;   // GEN_MAX_N of p3d_generic.hpp: the longest line of the any-length FFT

int check_shape(size_t nt, size_t ntr)
{
    if (nt < 1 || ntr < 1) return fail(P3D_ERR_INVALID, "bad shape (nt %zu, ntraces %zu)", nt, ntr);
    if (ntr > 2147483647u) return fail(P3D_ERR_INVALID, "too many traces for one call: split the cube");
    return P3D_OK;
}

// a caller's work buffer: aligned for its element, and long enough as far as the runtime can tell.  Best effort: the room is counted
// to the end of the allocation that holds the pointer (for a view into a pooled block: to the end of that block), and a pointer the
// runtime does not know is taken on trust
int check_work(const void* work, size_t need, size_t align)
{
    if ((uintptr_t)work % align) return fail(P3D_ERR_INVALID, "work buffer not aligned to %zu bytes", align);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)work) != hipSuccess) {
        (void)hipGetLastError();   // not an allocation of this runtime (a view of another allocator's pool): nothing to compare with
        return P3D_OK;
    }
    const size_t room = size - (size_t)((const char*)work - (const char*)base);
    if (room < need) return fail(P3D_ERR_INVALID, "work buffer too small: %zu bytes needed, %zu there", need, room);
    return P3D_OK;
}

constexpr int TPB = 256;
constexpr unsigned MAX_GRID_Y = 65535;

dim3 grid2(size_t ntr, size_t rows)
{
    return dim3((unsigned)((ntr + TPB - 1) / TPB), (unsigned)(rows < MAX_GRID_Y ? rows : MAX_GRID_Y));
}

// ---- gain ------------------------------------------------------------------------------------------------------------------------
enum Stage { S_BIAS = 0, S_TPOW, S_EPOW, S_GPOW, S_CLIP, S_PCLIP, S_NCLIP, S_QCLIP, S_LINEAR, S_PGC, S_DIV, S_SCALE, S_COUNT };

struct GainArgs {
    unsigned mask;          // stages to apply (bit s = Stage s), restricted by the host to one contiguous range of the order
    float bias, gpow, clip, pclip, nclip, scale;
    int norm;               // scale stage divides by `scale` (the reference's data * 1 / scale)
    const double* tpow;     // [nt] float64 curves
    const double* epow;
    const double* linear;
    const float* pgc;       // [nt] float32 curve
    const double* qthr;     // [ntr] per-trace quantile of |x|
    const float* div;       // [ntr] per-trace divisor (rms for norm_rms, the reference amplitude for balancing), 0 already -> 1
};

__device__ __forceinline__ float fsign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }   // np.sign

__global__ void __launch_bounds__(TPB) pre_gain_kernel(const float* __restrict__ x, float* __restrict__ out, long long nt, long long ntr, GainArgs a)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    for (long long t = blockIdx.y; t < nt; t += gridDim.y) {
        const long long i = t * ntr + j;
        float v = x[i];
        const unsigned m = a.mask;
        if (m & (1u << S_BIAS)) v = v + a.bias;
        if (m & (1u << S_TPOW)) v = (float)((double)v * a.tpow[t]);
        if (m & (1u << S_EPOW)) v = (float)((double)v * a.epow[t]);
        if (m & (1u << S_GPOW)) v = fsign(v) * powf(fabsf(v), a.gpow);
        if (m & (1u << S_CLIP)) v = fabsf(v) > a.clip ? a.clip * fsign(v) : v;
        if (m & (1u << S_PCLIP)) v = v > a.pclip ? a.pclip : v;
        if (m & (1u << S_NCLIP)) v = v < a.nclip ? a.nclip : v;
        if (m & (1u << S_QCLIP)) {
            const double q = a.qthr[j];
            v = (double)fabsf(v) > q ? (float)(q * (double)fsign(v)) : v;
        }
        if (m & (1u << S_LINEAR)) v = (float)((double)v * a.linear[t]);
        if (m & (1u << S_PGC)) v = v * a.pgc[t];
        if (m & (1u << S_DIV)) v = v / a.div[j];
        if (m & (1u << S_SCALE)) v = a.norm ? v / a.scale : v * a.scale;
        out[i] = v;
    }
}

// per-trace rms (kind 0: sqrt(sum(x^2) / nt), squares rounded to float32 as NumPy squares a float32 array, sum in double) or
// max |x| (kind 1); a zero result becomes 1 (the reference's guard before dividing), except for kind 2 (the plain rms)
__global__ void __launch_bounds__(TPB) pre_reduce_kernel(const float* __restrict__ x, long long nt, long long ntr, int kind, float* __restrict__ res)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    double s = 0.0;
    float mx = 0.0f;
    bool nan = false;
    for (long long t = 0; t < nt; ++t) {
        const float v = x[t * ntr + j];
        if (kind != 1) {
            s += (double)(v * v);
        } else {
            const float av = fabsf(v);
            nan |= av != av;
            mx = av > mx ? av : mx;
        }
    }
    const float r = kind != 1 ? (float)sqrt(s / (double)nt) : (nan ? NAN : mx);
    res[j] = (r == 0.0f && kind != 2) ? 1.0f : r;
}

// per-trace quantile of |x| with NumPy's default (linear) method: the order statistics lo = floor(q (n - 1)) and lo + 1 of |x| are
// found exactly by bisection on the IEEE bit pattern (monotonic for non-negative floats), one pass over the trace per bit, then
// interpolated like numpy's _lerp.  No per-lane array: no scratch memory.  A trace with a NaN gives NaN (NumPy does the same).
__global__ void __launch_bounds__(TPB) pre_quantile_kernel(const float* __restrict__ x, long long nt, long long ntr, double q, double* __restrict__ res)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    const double vidx = q * (double)(nt - 1);
    double flo = floor(vidx);
    if (flo < 0.0) flo = 0.0;
    if (flo > (double)(nt - 1)) flo = (double)(nt - 1);
    const long long lo = (long long)flo, hi = lo + 1 < nt ? lo + 1 : nt - 1;
    const double gamma = vidx - flo;
    bool nan = false;
    for (long long t = 0; t < nt && !nan; ++t) {
        const float v = x[t * ntr + j];
        nan = v != v;
    }
    if (nan) { res[j] = NAN; return; }
    unsigned a = 0u, b = 0x7f800000u;   // |x| <= +inf
    while (a < b) {
        const unsigned mid = a + (b - a) / 2;
        long long c = 0;
        for (long long t = 0; t < nt; ++t) c += (__float_as_uint(x[t * ntr + j]) & 0x7fffffffu) <= mid;
        if (c >= lo + 1) b = mid; else a = mid + 1;
    }
    const float vlo = __uint_as_float(a);
    long long cle = 0;
    unsigned nxt = 0x7f800000u;
    for (long long t = 0; t < nt; ++t) {
        const unsigned u = __float_as_uint(x[t * ntr + j]) & 0x7fffffffu;
        cle += u <= a;
        if (u > a && u < nxt) nxt = u;
    }
    const float vhi = cle >= hi + 1 ? vlo : __uint_as_float(nxt);
    const double d = (double)vhi - (double)vlo;
    res[j] = gamma >= 0.5 ? (double)vhi - d * (1.0 - gamma) : (double)vlo + d * gamma;
}

// ---- sosfiltfilt ---------------------------------------------------------------------------------------------------------------
constexpr int SOS_GROUP = 8;

struct SosArgs {
    double b0[SOS_GROUP], b1[SOS_GROUP], b2[SOS_GROUP], a1[SOS_GROUP], a2[SOS_GROUP], zi0[SOS_GROUP], zi1[SOS_GROUP];
};

// sample i of scipy's odd extension of trace j (edge samples on both ends), in float32 like scipy's odd_ext of a float32 array
__device__ __forceinline__ float odd_ext_at(const float* __restrict__ x, long long i, long long nt, long long ntr, long long edge, long long j)
{
    const long long k = i - edge;
    if (k < 0) return 2.0f * x[j] - x[(-k) * ntr + j];
    if (k >= nt) return 2.0f * x[(nt - 1) * ntr + j] - x[(2 * (nt - 1) - k) * ntr + j];
    return x[k * ntr + j];
}

template <int NS>
struct SosState {
    double z0[NS], z1[NS];
    __device__ __forceinline__ void init(const SosArgs& s, double v)
    {
#pragma unroll
        for (int k = 0; k < NS; ++k) { z0[k] = s.zi0[k] * v; z1[k] = s.zi1[k] * v; }
    }
    // scipy's _sosfilt step: transposed direct form II, section by section
    __device__ __forceinline__ double step(const SosArgs& s, double xc)
    {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double xn = s.b0[k] * xc + z0[k];
            z0[k] = s.b1[k] * xc - s.a1[k] * xn + z1[k];
            z1[k] = s.b2[k] * xc - s.a2[k] * xn;
            xc = xn;
        }
        return xc;
    }
};

// the whole cascade in one group: forward over the extension into tmp [nt + 2 edge][ntr], backward from the end into out
template <int NS>
__global__ void __launch_bounds__(TPB) sos_fused_kernel(const float* __restrict__ x, float* __restrict__ tmp, float* __restrict__ out, SosArgs s,
                                                        long long nt, long long ntr, long long edge)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    const long long ne = nt + 2 * edge;
    SosState<NS> st;
    st.init(s, (double)odd_ext_at(x, 0, nt, ntr, edge, j));
    double y = 0.0;
    for (long long i = 0; i < ne; ++i) {
        y = st.step(s, (double)odd_ext_at(x, i, nt, ntr, edge, j));
        tmp[i * ntr + j] = (float)y;
    }
    st.init(s, y);
    for (long long i = ne - 1; i >= 0; --i) {
        const double v = st.step(s, (double)tmp[i * ntr + j]);
        if (i >= edge && i < edge + nt) out[(i - edge) * ntr + j] = (float)v;
    }
}

// one group of a longer cascade, forward: from the extension of x (first group) or in place on tmp, which holds the signal
// between the groups in double [nt + 2 edge][ntr]; the last group also keeps its last output (y0), where the backward cascade starts
template <int NS>
__global__ void __launch_bounds__(TPB) sos_fwd_kernel(const float* __restrict__ x, double* __restrict__ tmp, double* __restrict__ y0, SosArgs s,
                                                      long long nt, long long ntr, long long edge, int first, int last)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    const long long ne = nt + 2 * edge;
    SosState<NS> st;
    st.init(s, (double)odd_ext_at(x, 0, nt, ntr, edge, j));   // every group starts from zi * ext[0] of the ORIGINAL input
    double y = 0.0;
    for (long long i = 0; i < ne; ++i) {
        const double v = first ? (double)odd_ext_at(x, i, nt, ntr, edge, j) : tmp[i * ntr + j];
        y = st.step(s, v);
        tmp[i * ntr + j] = y;
    }
    if (last) y0[j] = y;
}

// ... backward: in place on tmp from its end, from zi * y0 (y0: the last forward output of the cascade);
// the last group writes the interior to out
template <int NS>
__global__ void __launch_bounds__(TPB) sos_bwd_kernel(double* __restrict__ tmp, float* __restrict__ out, const double* __restrict__ y0, SosArgs s,
                                                      long long nt, long long ntr, long long edge, int last)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    const long long ne = nt + 2 * edge;
    SosState<NS> st;
    st.init(s, y0[j]);
    for (long long i = ne - 1; i >= 0; --i) {
        const double v = st.step(s, tmp[i * ntr + j]);
        if (!last) tmp[i * ntr + j] = v;
        else if (i >= edge && i < edge + nt) out[(i - edge) * ntr + j] = (float)v;
    }
}

template <template <int> class K, typename... A>
hipError_t launch_ns(int ns, dim3 g, A... args)
{
    switch (ns) {
    case 1: K<1>::go(g, args...); break;
    case 2: K<2>::go(g, args...); break;
    case 3: K<3>::go(g, args...); break;
    case 4: K<4>::go(g, args...); break;
    case 5: K<5>::go(g, args...); break;
    case 6: K<6>::go(g, args...); break;
    case 7: K<7>::go(g, args...); break;
    case 8: K<8>::go(g, args...); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <int NS> struct FusedL { template <typename... A> static void go(dim3 g, A... a) { sos_fused_kernel<NS><<<g, TPB>>>(a...); } };
template <int NS> struct FwdL { template <typename... A> static void go(dim3 g, A... a) { sos_fwd_kernel<NS><<<g, TPB>>>(a...); } };
template <int NS> struct BwdL { template <typename... A> static void go(dim3 g, A... a) { sos_bwd_kernel<NS><<<g, TPB>>>(a...); } };

// ---- upfirdn -------------------------------------------------------------------------------------------------------------------
// y[i] = sum_q h[m - up q] x[q], m = (pre_remove + i) down, q over the input samples with 0 <= m - up q < nh
__global__ void __launch_bounds__(TPB) pre_upfirdn_kernel(const float* __restrict__ x, float* __restrict__ out, const double* __restrict__ h, int nh,
                                                          int up, int down, long long pre_remove, long long nt, long long nout, long long ntr)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    for (long long i = blockIdx.y; i < nout; i += gridDim.y) {
        const long long m = (pre_remove + i) * down;
        long long qmax = m / up;
        if (qmax > nt - 1) qmax = nt - 1;
        const long long r = m - (nh - 1);
        long long qmin = r <= 0 ? 0 : (r + up - 1) / up;
        double acc = 0.0;
        for (long long q = qmin; q <= qmax; ++q) acc += h[m - up * q] * (double)x[q * ntr + j];
        out[i * ntr + j] = (float)acc;
    }
}

// ---- spectral ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) real_to_c32_kernel(const float* __restrict__ x, c32* __restrict__ w, long long n)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) w[i] = c32{x[i], 0.0f};
}

// Z[k] = op(fac[k] * X[src[k] >> 2]): op 0 plain, 1 conjugate, 2 real part; src < 0: zero
__global__ void __launch_bounds__(TPB) spec_remap_kernel(const c32* X, c32* Z, const int* __restrict__ src, const float* __restrict__ fac, long long nout,
                                                         long long ntr)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= ntr) return;
    for (long long k = blockIdx.y; k < nout; k += gridDim.y) {
        const int s = src[k];
        c32 z{0.0f, 0.0f};
        if (s >= 0) {
            const c32 v = X[(long long)(s >> 2) * ntr + j];
            const float f = fac[k];
            z = c32{v.x * f, v.y * f};
            const int op = s & 3;
            if (op == 1) z.y = -z.y;
            else if (op == 2) z.y = 0.0f;
        }
        Z[k * ntr + j] = z;
    }
}

__global__ void __launch_bounds__(TPB) c32_to_real_kernel(const c32* __restrict__ w, float* __restrict__ out, long long n, float s1, float s2, int modulus)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const c32 v = w[i];
    if (modulus) {
        const float re = v.x * s1, im = v.y * s1;
        out[i] = sqrtf(re * re + im * im);   // |analytic signal| (hypot without the overflow guard: |x| << FLT_MAX here)
    } else {
        out[i] = (v.x * s1) * s2;
    }
}

int gain_pass(const float* x, float* out, size_t nt, size_t ntr, GainArgs a)
{
    if (!a.mask) {
        if (x != out) P3D_TRY(hipMemcpy(out, x, sizeof(float) * nt * ntr, hipMemcpyDeviceToDevice));
        return P3D_OK;
    }
    pre_gain_kernel<<<grid2(ntr, nt), TPB>>>(x, out, (long long)nt, (long long)ntr, a);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

unsigned range_mask(int lo, int hi) { return (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u); }

}  // namespace

extern "C" {

int p3d_pre_reduce_dev(int device, const float* x, size_t nt, size_t ntr, int kind, float* res)
{
    if (!x || !res) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (kind < 0 || kind > 2) return fail(P3D_ERR_INVALID, "unknown reduction %d (0 = rms, 1 = max, 2 = rms without the 0 -> 1 guard)", kind);
    int rc = check_shape(nt, ntr);
    if (rc || (rc = use_device(device))) return rc;
    pre_reduce_kernel<<<(unsigned)((ntr + TPB - 1) / TPB), TPB>>>(x, (long long)nt, (long long)ntr, kind, res);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_pre_balance_dev(int device, const float* x, size_t nt, size_t ntr, int kind, float* out, float* ref)
{
    if (!x || !out || !ref) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (kind != 0 && kind != 1) return fail(P3D_ERR_INVALID, "unknown reference amplitude %d (0 = rms, 1 = max)", kind);
    int rc = p3d_pre_reduce_dev(device, x, nt, ntr, kind, ref);
    if (rc) return rc;
    GainArgs a{};
    a.mask = 1u << S_DIV;
    a.div = ref;
    if ((rc = gain_pass(x, out, nt, ntr, a))) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_pre_gain_dev(int device, const float* x, size_t nt, size_t ntr, const double* prm, const double* curves, float* out, float* work)
{
    if (!x || !out || !prm) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (x == out) return fail(P3D_ERR_INVALID, "x and out must be different buffers");
    int rc = check_shape(nt, ntr);
    if (rc || (rc = use_device(device))) return rc;
    const unsigned flags = (unsigned)prm[P3D_GAIN_FLAGS];
    if (flags & ~((1u << P3D_GAIN_NBITS) - 1u)) return fail(P3D_ERR_INVALID, "unknown gain flags 0x%x", flags);
    const bool agc = flags & P3D_GAIN_F_AGC;
    if (agc && !work) return fail(P3D_ERR_INVALID, "AGC needs a work buffer of nt x ntraces floats");
    const bool need_curves = flags & (P3D_GAIN_F_TPOW | P3D_GAIN_F_EPOW | P3D_GAIN_F_LINEAR | P3D_GAIN_F_PGC);
    if (need_curves && !curves) return fail(P3D_ERR_INVALID, "gain curves missing");

    // tables: tpow, epow, linear (float64) and pgc (float32) curves [nt]; per-trace quantile (double) and rms (float)
    DevBuf dcur, dq, drms;
    GainArgs a{};
    a.bias = (float)prm[P3D_GAIN_BIAS];
    a.gpow = (float)prm[P3D_GAIN_GPOW];
    a.clip = (float)prm[P3D_GAIN_CLIP];
    a.pclip = (float)prm[P3D_GAIN_PCLIP];
    a.nclip = (float)prm[P3D_GAIN_NCLIP];
    a.scale = (float)prm[P3D_GAIN_SCALE];
    a.norm = (flags & P3D_GAIN_F_NORM) != 0;
    if (need_curves) {
        std::vector<double> host(curves, curves + 4 * nt);
        std::vector<float> pgc(nt);
        for (size_t t = 0; t < nt; ++t) pgc[t] = (float)curves[3 * nt + t];
        P3D_TRY(hipMalloc(&dcur.p, sizeof(double) * 3 * nt + sizeof(float) * nt));
        P3D_TRY(hipMemcpy(dcur.p, host.data(), sizeof(double) * 3 * nt, hipMemcpyHostToDevice));
        float* dp = (float*)((double*)dcur.p + 3 * nt);
        P3D_TRY(hipMemcpy(dp, pgc.data(), sizeof(float) * nt, hipMemcpyHostToDevice));
        a.tpow = (const double*)dcur.p;
        a.epow = a.tpow + nt;
        a.linear = a.tpow + 2 * nt;
        a.pgc = dp;
    }
    unsigned want = 0;
    if (flags & P3D_GAIN_F_BIAS) want |= 1u << S_BIAS;
    if (flags & P3D_GAIN_F_TPOW) want |= 1u << S_TPOW;
    if (flags & P3D_GAIN_F_EPOW) want |= 1u << S_EPOW;
    if (flags & P3D_GAIN_F_GPOW) want |= 1u << S_GPOW;
    if (flags & P3D_GAIN_F_CLIP) want |= 1u << S_CLIP;
    if (flags & P3D_GAIN_F_PCLIP) want |= 1u << S_PCLIP;
    if (flags & P3D_GAIN_F_NCLIP) want |= 1u << S_NCLIP;
    if (flags & P3D_GAIN_F_QCLIP) want |= 1u << S_QCLIP;
    if (flags & P3D_GAIN_F_LINEAR) want |= 1u << S_LINEAR;
    if (flags & P3D_GAIN_F_PGC) want |= 1u << S_PGC;
    if (flags & P3D_GAIN_F_NORM_RMS) want |= 1u << S_DIV;
    if (flags & P3D_GAIN_F_SCALE) want |= 1u << S_SCALE;

    // one pass per maximal run of stages with no per-trace barrier inside it; the barriers exist only where requested:
    // AGC before S_CLIP, the quantile of |x| before S_QCLIP, the rms before S_DIV.  Every stage works on the float32 value of
    // the one before, so a fused pass gives the same bits as separate ones.
    // the data moves x -> out (first pass), then out -> work -> out ... ; a pass with no stage is skipped
    const float* cur = x;
    auto dst_for = [&](const float* c) { return c == out ? work : out; };
    auto run = [&](int lo, int hi) -> int {
        GainArgs b = a;
        b.mask = want & range_mask(lo, hi);
        if (!b.mask) return P3D_OK;
        float* d = dst_for(cur);
        if (!d) return fail(P3D_ERR_INVALID, "this gain needs a work buffer of nt x ntraces floats");
        int r = gain_pass(cur, d, nt, ntr, b);
        if (r) return r;
        cur = d;
        return P3D_OK;
    };
    int lo = 0;
    if (agc) {
        if ((rc = run(lo, S_CLIP))) return rc;
        lo = S_CLIP;
        float* d = dst_for(cur);
        const int win = (int)prm[P3D_GAIN_AGC_WIN], kind = (int)prm[P3D_GAIN_AGC_KIND], sq = prm[P3D_GAIN_AGC_SQRT] != 0.0;
        if ((rc = p3d_agc_dev(device, cur, nt, ntr, win, kind, sq, d, nullptr))) return rc;
        cur = d;
    }
    if (want & (1u << S_QCLIP)) {
        if ((rc = run(lo, S_QCLIP))) return rc;
        lo = S_QCLIP;
        P3D_TRY(hipMalloc(&dq.p, sizeof(double) * ntr));
        pre_quantile_kernel<<<(unsigned)((ntr + TPB - 1) / TPB), TPB>>>(cur, (long long)nt, (long long)ntr, prm[P3D_GAIN_QCLIP], (double*)dq.p);
        P3D_TRY(hipGetLastError());
        a.qthr = (const double*)dq.p;
    }
    if (want & (1u << S_DIV)) {
        if ((rc = run(lo, S_DIV))) return rc;
        lo = S_DIV;
        P3D_TRY(hipMalloc(&drms.p, sizeof(float) * ntr));
        pre_reduce_kernel<<<(unsigned)((ntr + TPB - 1) / TPB), TPB>>>(cur, (long long)nt, (long long)ntr, 0, (float*)drms.p);
        P3D_TRY(hipGetLastError());
        a.div = (const float*)drms.p;
    }
    if ((rc = run(lo, S_COUNT))) return rc;
    if (cur == x) {
        P3D_TRY(hipMemcpy(out, x, sizeof(float) * nt * ntr, hipMemcpyDeviceToDevice));
    } else if (cur != out) {
        P3D_TRY(hipMemcpy(out, cur, sizeof(float) * nt * ntr, hipMemcpyDeviceToDevice));
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_pre_sosfiltfilt_dev(int device, const float* x, size_t nt, size_t ntr, int nsec, const double* sos, const double* zi, int padlen, float* out,
                            void* work)
{
    if (!x || !out || !sos || !zi) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (x == out) return fail(P3D_ERR_INVALID, "x and out must be different buffers");
    if (nsec < 1) return fail(P3D_ERR_INVALID, "%d sections", nsec);
    if (padlen < 0) return fail(P3D_ERR_INVALID, "padlen %d", padlen);
    int rc = check_shape(nt, ntr);
    if (rc || (rc = use_device(device))) return rc;
    if (nt <= (size_t)padlen)
        return fail(P3D_ERR_INVALID, "The length of the input vector x must be greater than padlen, which is %d.", padlen);
    for (int k = 0; k < nsec; ++k)
        if (sos[6 * k + 3] != 1.0) return fail(P3D_ERR_INVALID, "section %d: a0 must be 1", k);
    const size_t ne = nt + 2 * (size_t)padlen;
    const int ngroups = (nsec + SOS_GROUP - 1) / SOS_GROUP;
    // the intermediate: float32 for one group (between the forward and the backward pass), double between the groups of a longer cascade
    const size_t need = (ngroups == 1 ? sizeof(float) : sizeof(double)) * ne * ntr;
    DevBuf dtmp, dy0;
    void* tmp = work;
    if (!tmp) {
        P3D_TRY(hipMalloc(&dtmp.p, need));
        tmp = dtmp.p;
    } else {
        if ((rc = check_work(tmp, need, ngroups == 1 ? sizeof(float) : sizeof(double)))) return rc;
    }
    std::vector<SosArgs> groups(ngroups);
    std::vector<int> gsize(ngroups);
    for (int g = 0; g < ngroups; ++g) {
        SosArgs s{};
        const int k0 = g * SOS_GROUP, n = nsec - k0 < SOS_GROUP ? nsec - k0 : SOS_GROUP;
        for (int k = 0; k < n; ++k) {
            const double* c = sos + 6 * (k0 + k);
            s.b0[k] = c[0]; s.b1[k] = c[1]; s.b2[k] = c[2]; s.a1[k] = c[4]; s.a2[k] = c[5];
            s.zi0[k] = zi[2 * (k0 + k)]; s.zi1[k] = zi[2 * (k0 + k) + 1];
        }
        groups[g] = s;
        gsize[g] = n;
    }
    const dim3 g1((unsigned)((ntr + TPB - 1) / TPB));
    const long long lnt = (long long)nt, lntr = (long long)ntr, ledge = padlen;
    if (ngroups == 1) {
        P3D_TRY(launch_ns<FusedL>(gsize[0], g1, x, (float*)tmp, out, groups[0], lnt, lntr, ledge));
    } else {
        P3D_TRY(hipMalloc(&dy0.p, sizeof(double) * ntr));
        double* y0 = (double*)dy0.p;
        double* dt = (double*)tmp;
        for (int g = 0; g < ngroups; ++g)
            P3D_TRY(launch_ns<FwdL>(gsize[g], g1, x, dt, y0, groups[g], lnt, lntr, ledge, (int)(g == 0), (int)(g == ngroups - 1)));
        for (int g = 0; g < ngroups; ++g)
            P3D_TRY(launch_ns<BwdL>(gsize[g], g1, dt, out, (const double*)y0, groups[g], lnt, lntr, ledge, (int)(g == ngroups - 1)));
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_pre_upfirdn_dev(int device, const float* x, size_t nt, size_t ntr, const double* h, int nh, int up, int down, long long pre_remove,
                        size_t nout, float* out)
{
    if (!x || !out || !h) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (x == out) return fail(P3D_ERR_INVALID, "x and out must be different buffers");
    if (nh < 1 || up < 1 || down < 1 || pre_remove < 0 || nout < 1) return fail(P3D_ERR_INVALID, "bad upfirdn parameters");
    int rc = check_shape(nt, ntr);
    if (rc || (rc = use_device(device))) return rc;
    DevBuf dh;
    P3D_TRY(hipMalloc(&dh.p, sizeof(double) * nh));
    P3D_TRY(hipMemcpy(dh.p, h, sizeof(double) * nh, hipMemcpyHostToDevice));
    pre_upfirdn_kernel<<<grid2(ntr, nout), TPB>>>(x, out, (const double*)dh.p, nh, up, down, pre_remove, (long long)nt, (long long)nout, (long long)ntr);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_pre_spectral_dev(int device, const float* x, size_t nt, size_t ntr, int num, const int* src, const float* fac, int modulus, double s1,
                         double s2, float* out, void* work)
{
    if (!x || !out || !src || !fac) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (num < 1) return fail(P3D_ERR_INVALID, "output length %d", num);
    int rc = check_shape(nt, ntr);
    if (rc || (rc = use_device(device))) return rc;
    if (!p3d::axis0_fft_supported((int)nt) || nt > 2147483647u)
        return fail(P3D_ERR_UNSUPPORTED, "a trace of %zu samples: FFT lengths up to %d are supported", nt, FFT_MAX_N);
    if (!p3d::axis0_fft_supported(num)) return fail(P3D_ERR_UNSUPPORTED, "an output trace of %d samples: FFT lengths up to %d are supported", num, FFT_MAX_N);
    for (int k = 0; k < num; ++k)
        if (src[k] >= 0 && (size_t)(src[k] >> 2) >= nt) return fail(P3D_ERR_INVALID, "source bin %d of output bin %d outside 0..%zu", src[k] >> 2, k, nt - 1);
    DevBuf dw, dsrc, dfac;
    c32* wx = (c32*)work;
    if (!wx) {
        P3D_TRY(hipMalloc(&dw.p, sizeof(c32) * ((size_t)nt + (size_t)num) * ntr));
        wx = (c32*)dw.p;
    }
    c32* wz = wx + nt * ntr;
    P3D_TRY(hipMalloc(&dsrc.p, sizeof(int) * num));
    P3D_TRY(hipMalloc(&dfac.p, sizeof(float) * num));
    P3D_TRY(hipMemcpy(dsrc.p, src, sizeof(int) * num, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dfac.p, fac, sizeof(float) * num, hipMemcpyHostToDevice));
    const long long n_in = (long long)(nt * ntr), n_out = (long long)num * (long long)ntr;
    real_to_c32_kernel<<<(unsigned)((n_in + TPB - 1) / TPB), TPB>>>(x, wx, n_in);
    P3D_TRY(hipGetLastError());
    if ((rc = p3d::axis0_fft(device, wx, (int)nt, ntr, 0))) return rc;
    spec_remap_kernel<<<grid2(ntr, (size_t)num), TPB>>>(wx, wz, (const int*)dsrc.p, (const float*)dfac.p, num, (long long)ntr);
    P3D_TRY(hipGetLastError());
    if ((rc = p3d::axis0_fft(device, wz, num, ntr, 1))) return rc;
    c32_to_real_kernel<<<(unsigned)((n_out + TPB - 1) / TPB), TPB>>>(wz, out, n_out, (float)s1, (float)s2, modulus);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // extern "C"
