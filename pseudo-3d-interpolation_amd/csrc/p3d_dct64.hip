// p3d_dct64.hip -- the DCT POCS loop (transform_kind = 'DCT') in the REFERENCE's own precision: the passes of p3d_dct.hip in double, on the
// buffers and the transforms of the double-precision FFT plan (p3d_f64.hip / p3d_f64.hpp; plan64_fft2_work).  DESIGN.md section 3.16.1; the identities
// are those of p3d_dct_tables.hpp, whose factors stay doubles here.
//
// The iterate lives in the plan's work buffer in REORDERED sample order (even samples ascending, odd samples descending, both axes), so that fft2
// of the buffer is the V of the identities.  One iteration is fft2 | group pass | ifft2 | update pass, the traffic of the unfused double-precision
// FFT loop (216 bytes per point):
//   group pass   a thread owns the four coefficients {k1, n1 - k1} x {k2, n2 - k2}: combine V -> X, threshold X, split X -> V', in registers
//   update pass  update64_kernel (p3d_f64.hip) expression for expression, the reordering folded into the address of the iterate
// Along the fast axis a wavefront of the group pass reads 64 ascending and 64 descending neighbours of 16 bytes (1 KiB of whole lines either way);
// a wavefront of the update pass touches, for 64 neighbouring samples, the 32 + 32 buffer elements of their even and odd halves.  No atomics:
// the cost sums are per-block partials that fold64_kernel adds in a fixed order, so a slice's result does not depend on the batch around it.
//
// Entry points (include/p3d.h): p3d_dct2_c128, p3d_pocs64_dct_stats, p3d_pocs64_dct_run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "p3d.h"
#include "p3d_dct_tables.hpp"
#include "p3d_f64.hpp"
#include "p3d_host.hpp"
#include "p3d_internal.hpp"

using p3d::choose_out;
using p3d::elem_bytes;
using p3d::fail;
using p3d::grow;
using p3d::LoopFrame;
using p3d::stage_mask;
using p3d::take_x;

namespace {

namespace dct = p3d::dct;
using p3d::f64::c64;
using p3d::f64::shrink64;

// device tables of one norm: forward / inverse factors of axis 1 (length n1) and axis 2 (length n2)
struct DctTab64 {
    const c64 *f1, *i1, *f2, *i2;
};

enum { DCT64_FUSED = 0, DCT64_COMBINE = 1, DCT64_SPLIT = 2 };   // V -> X -> threshold -> V' | V -> X (statistics, forward hook) | X -> V (inverse hook)

// a * f + b * conj(f): one step of the combine
__device__ __forceinline__ c64 comb(c64 a, c64 b, c64 f) { return {a.x * f.x - a.y * f.y + (b.x * f.x + b.y * f.y), a.x * f.y + a.y * f.x + (b.y * f.x - b.x * f.y)}; }

template <int MODE>
__global__ __launch_bounds__(256) void dct_group64_kernel(c64* w, DctTab64 t, const c64* tau, int niter, int iter, int op, int n1, int n2, const int* done)
{
    const int s = blockIdx.z;
    if (done && done[s] != 0) return;
    const int k2 = blockIdx.x * 64 + threadIdx.x, k1 = blockIdx.y * 4 + threadIdx.y;
    if (k2 >= dct::owners(n2) || k1 >= dct::owners(n1)) return;
    const int p1 = dct::partner(n1, k1), p2 = dct::partner(n2, k2);
    c64* const base = w + (size_t)s * n1 * n2;
    const size_t a00 = (size_t)k1 * n2 + k2, a01 = (size_t)k1 * n2 + p2, a10 = (size_t)p1 * n2 + k2, a11 = (size_t)p1 * n2 + p2;
    // (a self-paired index reads its element twice: the arithmetic below needs no special case, only the stores do)
    c64 v00 = base[a00], v01 = base[a01], v10 = base[a10], v11 = base[a11];
    if (MODE == DCT64_FUSED || MODE == DCT64_COMBINE) {
        const c64 t2 = t.f2[k2], t2p = t.f2[p2], t1 = t.f1[k1], t1p = t.f1[p1];
        const c64 y00 = comb(v00, v01, t2), y01 = comb(v01, v00, t2p);
        const c64 y10 = comb(v10, v11, t2), y11 = comb(v11, v10, t2p);
        v00 = comb(y00, y10, t1);
        v10 = comb(y10, y00, t1p);
        v01 = comb(y01, y11, t1);
        v11 = comb(y11, y01, t1p);
    }
    if (MODE == DCT64_FUSED) {
        const c64 th = tau[(size_t)s * niter + iter];
        v00 = shrink64(v00, th, op); v01 = shrink64(v01, th, op); v10 = shrink64(v10, th, op); v11 = shrink64(v11, th, op);
    }
    if (MODE != DCT64_COMBINE) {
        c64 y00, y01, y10, y11;
        if (k1 == 0) {
            const c64 u = t.i1[0];
            y00 = y10 = v00 * u;
            y01 = y11 = v01 * u;
        } else {
            const c64 u = t.i1[k1], up = t.i1[p1];
            y00 = sub_i(v00, v10) * u;
            y10 = sub_i(v10, v00) * up;
            y01 = sub_i(v01, v11) * u;
            y11 = sub_i(v11, v01) * up;
        }
        if (k2 == 0) {
            const c64 u = t.i2[0];
            v00 = v01 = y00 * u;
            v10 = v11 = y10 * u;
        } else {
            const c64 u = t.i2[k2], up = t.i2[p2];
            v00 = sub_i(y00, y01) * u;
            v01 = sub_i(y01, y00) * up;
            v10 = sub_i(y10, y11) * u;
            v11 = sub_i(y11, y10) * up;
        }
    }
    base[a00] = v00;
    if (p2 != k2) base[a01] = v01;
    if (p1 != k1) {
        base[a10] = v10;
        if (p2 != k2) base[a11] = v11;
    }
}

__device__ inline double block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// update64_kernel (p3d_f64.hip) with w addressed through the reordering: sample (i1, i2) of x, mask and out lives at w[perm(n1, i1)][perm(n2, i2)].
// mode 0 / 1 as there; mode 2: out = w through the reordering, nothing else (the inverse test hook)
__global__ __launch_bounds__(256) void dct_update64_kernel(c64* w, const void* x, int dtype, const double* mask, size_t mask_stride, void* out, double* partial, int mode,
                                                           int adaptive, int write_out, double alpha, int n1, int n2, const int* done, int zero_fill)
{
    __shared__ double sh[256];
    const int s = blockIdx.y;
    const int dn = done ? done[s] : 0;
    const unsigned per_slice = (unsigned)n1 * (unsigned)n2, stride = gridDim.x * blockDim.x;   // (extents up to 5120: a slice has fewer than 2^25 points)
    const size_t s0 = (size_t)s * per_slice;
    auto put = [&](size_t g, c64 v) {
        if (dtype == P3D_C128) reinterpret_cast<c64*>(out)[g] = v;
        else if (dtype == P3D_F64) reinterpret_cast<double*>(out)[g] = v.x;
        else if (dtype == P3D_C64) reinterpret_cast<float2*>(out)[g] = float2{(float)v.x, (float)v.y};
        else reinterpret_cast<float*>(out)[g] = (float)v.x;
    };
    if (zero_fill && dn < 0) {   // an empty slice is handed back untouched (zeros), POCS.py:515-521
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < per_slice; i += stride) put(s0 + i, c64{0.0, 0.0});
    }
    if (dn != 0) {
        if (threadIdx.x == 0 && mode != 2) partial[(size_t)s * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    double acc = 0.0;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < per_slice; i += stride) {
        const size_t g = s0 + i;
        const unsigned i1 = i / (unsigned)n2, i2 = i - i1 * (unsigned)n2;
        const size_t gw = s0 + (size_t)dct::perm(n1, (int)i1) * n2 + dct::perm(n2, (int)i2);
        if (mode == 2) {
            put(g, w[gw]);
            continue;
        }
        c64 xo;
        if (dtype == P3D_C128) xo = reinterpret_cast<const c64*>(x)[g];
        else if (dtype == P3D_F64) xo = c64{reinterpret_cast<const double*>(x)[g], 0.0};
        else if (dtype == P3D_C64) { const float2 t = reinterpret_cast<const float2*>(x)[g]; xo = c64{(double)t.x, (double)t.y}; }
        else xo = c64{(double)reinterpret_cast<const float*>(x)[g], 0.0};
        const double m = mask ? mask[(size_t)s * mask_stride + i] : 0.0;
        const double wgt = 1.0 - alpha * m;
        c64 xn;
        if (mode == 0) {
            xn = xo;
        } else {
            xn = w[gw] * wgt + xo * alpha;
            if (write_out) put(g, xn);
        }
        acc += hypot(xn.x, xn.y);
        if (adaptive) {   // POCS.py:574-575
            const c64 tmp = xo * alpha + xn * wgt;
            w[gw] = tmp + (xo - xn * m) * (1.0 - alpha);
        } else {
            w[gw] = xn;
        }
    }
    if (mode == 2) return;
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = tot;
}

int check(p3d_plan64* p, int nslices, int dtype, int norm)
{
    if (!p) return fail(P3D_ERR_INVALID, "NULL plan");
    if (nslices < 1 || nslices > p->max_slices) return fail(P3D_ERR_INVALID, "nslices = %d outside 1..max_slices (%d)", nslices, p->max_slices);
    if (dtype != P3D_C128 && dtype != P3D_F64 && dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_INVALID, "unknown dtype %d", dtype);
    if (norm != P3D_DCT_BACKWARD && norm != P3D_DCT_ORTHO) return fail(P3D_ERR_UNSUPPORTED, "DCT norm %d is not implemented (backward, ortho)", norm);
    if (!p->st_x || !p->st_out) return fail(P3D_ERR_INVALID, "the plan has no staging buffers");
    P3D_TRY(hipSetDevice(p->device));
    p->sorted_slices = 0;   // (every entry overwrites the work buffer: a sorted spectrum kept there is gone)
    if (!p->dct_tab) {   // the factors of both norms, built by the first DCT call on the plan
        const size_t per = 2 * ((size_t)p->nil + p->nxl);
        std::vector<c64> host(2 * per);
        for (int nm = 0; nm < 2; ++nm) {
            c64* b = host.data() + nm * per;
            dct::build_tables(p->nil, nm, b, b + p->nil);
            dct::build_tables(p->nxl, nm, b + 2 * (size_t)p->nil, b + 2 * (size_t)p->nil + p->nxl);
        }
        P3D_TRY(hipMalloc((void**)&p->dct_tab, sizeof(c64) * host.size()));
        P3D_TRY(hipMemcpy(p->dct_tab, host.data(), sizeof(c64) * host.size(), hipMemcpyHostToDevice));
    }
    return P3D_OK;
}

DctTab64 tab_of(p3d_plan64* p, int norm)
{
    const c64* b = p->dct_tab + (size_t)norm * 2 * ((size_t)p->nil + p->nxl);
    return DctTab64{b, b + p->nil, b + 2 * (size_t)p->nil, b + 2 * (size_t)p->nil + p->nxl};
}

int group(p3d_plan64* p, int mode, int norm, int niter, int iter, int op, int nslices, const int* done)
{
    const int n1 = p->nil, n2 = p->nxl;
    const dim3 block(64, 4), grid((unsigned)((dct::owners(n2) + 63) / 64), (unsigned)((dct::owners(n1) + 3) / 4), (unsigned)nslices);
    const DctTab64 t = tab_of(p, norm);
    switch (mode) {
        case DCT64_FUSED: dct_group64_kernel<DCT64_FUSED><<<grid, block, 0, p->stream>>>(p->work, t, p->tau, niter, iter, op, n1, n2, done); break;
        case DCT64_COMBINE: dct_group64_kernel<DCT64_COMBINE><<<grid, block, 0, p->stream>>>(p->work, t, p->tau, niter, iter, op, n1, n2, done); break;
        default: dct_group64_kernel<DCT64_SPLIT><<<grid, block, 0, p->stream>>>(p->work, t, p->tau, niter, iter, op, n1, n2, done); break;
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

// the update pass on the plan's current x / out; modes 0 and 1 leave sum |x| of every slice in sums_row
int update(p3d_plan64* p, int dtype, double* sums_row, int mode, int adaptive, int write_out, double alpha, int nslices, const int* done, int zero_fill)
{
    dct_update64_kernel<<<dim3(p3d_plan64::BLOCKS, nslices), 256, 0, p->stream>>>(p->work, p->cur_x, dtype, mode == 0 && !adaptive ? nullptr : p->mask, p->mask_stride, p->cur_out,
                                                                                  p->spart, mode, adaptive, write_out, alpha, p->nil, p->nxl, done, zero_fill);
    P3D_TRY(hipGetLastError());
    return mode == 2 ? P3D_OK : p3d::plan64_fold_sums(p, sums_row, nslices, p3d_plan64::BLOCKS);
}

// cur_x -> reordered iterate -> fft2 -> combine: the work buffer holds X = dctn(x)
int forward(p3d_plan64* p, int dtype, int nslices, int norm)
{
    int rc;
    if ((rc = update(p, dtype, p->partial, 0, 0, 0, 1.0, nslices, nullptr, 0))) return rc;   // (its sums go to a scratch row)
    if ((rc = p3d::plan64_fft2_work(p, nslices, false, nullptr))) return rc;
    return group(p, DCT64_COMBINE, norm, 1, 0, 0, nslices, nullptr);
}

}  // namespace

extern "C" {

// test hook: scipy.fft.dctn / idctn (type 2) of HOST complex128 slices through the loop's own passes
int p3d_dct2_c128(p3d_plan64* p, const void* in_host, void* out_host, int nslices, int inverse, int norm)
{
    int rc = check(p, nslices, P3D_C128, norm);
    if (rc) return rc;
    if (!in_host || !out_host) return fail(P3D_ERR_INVALID, "NULL buffer");
    const size_t bytes = sizeof(c64) * p->per() * nslices;
    p->sparse = false;
    p->cur_x = p->st_x;
    p->cur_out = p->st_out;
    if (!inverse) {
        P3D_TRY(hipMemcpyAsync(p->st_x, in_host, bytes, hipMemcpyHostToDevice, p->stream));
        if ((rc = forward(p, P3D_C128, nslices, norm))) return rc;
        P3D_TRY(hipMemcpyAsync(out_host, p->work, bytes, hipMemcpyDeviceToHost, p->stream));
    } else {
        P3D_TRY(hipMemcpyAsync(p->work, in_host, bytes, hipMemcpyHostToDevice, p->stream));
        if ((rc = group(p, DCT64_SPLIT, norm, 1, 0, 0, nslices, nullptr))) return rc;
        if ((rc = p3d::plan64_fft2_work(p, nslices, true, nullptr))) return rc;
        if ((rc = update(p, P3D_C128, nullptr, 2, 0, 0, 1.0, nslices, nullptr, 0))) return rc;
        P3D_TRY(hipMemcpyAsync(out_host, p->st_out, bytes, hipMemcpyDeviceToHost, p->stream));
    }
    P3D_TRY(hipStreamSynchronize(p->stream));
    return P3D_OK;
}

// statistics of dctn(x) for the schedule: stats[nslices][P3D_STATS_PER_SLICE] as p3d_pocs64_stats (x: host or device pointer)
int p3d_pocs64_dct_stats(p3d_plan64* p, const void* x, int dtype, int nslices, double* stats, int norm)
{
    int rc = check(p, nslices, dtype, norm);
    if (rc) return rc;
    if (!x || !stats) return fail(P3D_ERR_INVALID, "NULL buffer");
    if ((rc = take_x(p, x, elem_bytes(dtype) * p->per() * nslices))) return rc;
    p->cur_out = p->st_out;
    p->sparse = false;
    if ((rc = forward(p, dtype, nslices, norm))) return rc;
    return p3d::plan64_work_stats(p, nslices, stats);
}

// p3d_pocs64_run's unfused loop with the DCT pair in place of the FFT pair: first input, then per iteration fft2 -> group pass (combine, threshold,
// split) -> ifft2 -> re-insertion.  Arguments as there.
int p3d_pocs64_dct_run(p3d_plan64* p, const void* x, int dtype, const double* mask, const double* tau, const uint8_t* active, const p3d_pocs_params* prm, void* out,
                       int nslices, int32_t* niter_done, double* sums, double* elapsed_ms, int norm)
{
    int rc = check(p, nslices, dtype, norm);
    if (rc) return rc;
    if (!x || !mask || !tau || !prm || !out) return fail(P3D_ERR_INVALID, "NULL argument");
    if (prm->niter < 1) return fail(P3D_ERR_INVALID, "niter must be >= 1");
    if (prm->thresh_op < P3D_OP_HARD || prm->thresh_op > P3D_OP_GARROTE)
        return fail(P3D_ERR_UNSUPPORTED, "thresh_op %d: the double-precision path has hard, soft and garrote", prm->thresh_op);
    if (prm->version < P3D_VER_REGULAR || prm->version > P3D_VER_ADAPTIVE) return fail(P3D_ERR_INVALID, "unknown version %d", prm->version);
    const int niter = prm->niter;
    const bool early = prm->eps > 0.0, adaptive = prm->version == P3D_VER_ADAPTIVE;
    const size_t ntau = (size_t)nslices * niter, nsum = (size_t)(niter + 1) * nslices, per = p->per();
    if ((rc = grow(p->tau, p->tau_cap, ntau)) || (rc = grow(p->sums, p->sums_cap, nsum))) return rc;
    LoopFrame frame(p, active, nslices, niter);
    const int* done_d = (early || frame.any_off()) ? p->done : nullptr;
    const size_t cube_bytes = elem_bytes(dtype) * per * nslices;
    if ((rc = take_x(p, x, cube_bytes))) return rc;
    const bool direct_out = choose_out(p, x, out, cube_bytes);
    if ((rc = stage_mask(p->mask, p->mask_cap, mask, per, prm, nslices, p->max_slices, p->stream, &p->mask_stride))) return rc;
    P3D_TRY(hipMemcpyAsync(p->tau, tau, sizeof(c64) * ntau, hipMemcpyHostToDevice, p->stream));   // (Re, Im) pairs of doubles: c64's layout
    if ((rc = frame.begin())) return rc;
    p->sparse = false;
    if ((rc = update(p, dtype, p->sums, 0, adaptive ? 1 : 0, 0, prm->alpha, nslices, done_d, 0))) return rc;
    for (int k = 0; k < niter; ++k) {
        const bool last = k + 1 == niter;
        if ((rc = p3d::plan64_fft2_work(p, nslices, false, done_d))) return rc;
        if ((rc = group(p, DCT64_FUSED, norm, niter, k, prm->thresh_op, nslices, done_d))) return rc;
        if ((rc = p3d::plan64_fft2_work(p, nslices, true, done_d))) return rc;
        if ((rc = update(p, dtype, p->sums + (size_t)(k + 1) * nslices, 1, (adaptive && !last) ? 1 : 0, (early || last) ? 1 : 0, prm->alpha, nslices, p->done, last ? 1 : 0)))
            return rc;
        if (early && (rc = p3d::plan64_converged(p, nslices, k, prm->eps))) return rc;
    }
    if ((rc = frame.enqueue_end(sums))) return rc;
    if (!direct_out) P3D_TRY(hipMemcpyAsync(out, p->st_out, cube_bytes, hipMemcpyDefault, p->stream));
    return frame.collect(niter_done, elapsed_ms);
}

}  // extern "C"
