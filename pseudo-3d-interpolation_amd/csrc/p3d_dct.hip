// p3d_dct.hip -- the passes that turn the plan's batched 2-D FFT into scipy.fft.dctn / idctn (type 2, norm 'backward' or 'ortho') inside
// the POCS loop (transform_kind = 'DCT'; DESIGN.md section 3.16, identities in p3d_dct_tables.hpp).
//
// The iterate lives in a row-major buffer in REORDERED sample order (even samples ascending, odd samples descending, both axes), so that
// fft2 of the buffer is the V of the identities.  One iteration is then fft2 | group pass | ifft2 | update pass:
//   group pass   a thread owns the four coefficients {k1, n1 - k1} x {k2, n2 - k2}: combine V -> X, threshold X, split X -> V', in registers
//   update pass  re-insertion, cost sums, result and APOCS mix as gen_update_kernel, the reordering folded into the addressing of the buffer
// Memory traffic equals the unfused FFT loop's (p3d_api.hip: run_generic).  Along the fast axis a wavefront of the group pass reads 64
// ascending and 64 descending neighbours (whole cache lines either way); a wavefront of the update pass touches, for 64 neighbouring
// samples, the 32 + 32 buffer elements of their even and odd halves -- again whole lines.
#include <hip/hip_runtime.h>

#include <cmath>

#include "p3d_dct.hpp"
#include "p3d_dct_tables.hpp"
#include "p3d_shrink.hpp"

namespace p3d {

template <int MODE>
__global__ __launch_bounds__(256) void dct_group_kernel(c32* w, DctTab t, const c32* tau, int niter, int iter, int op, int n1, int n2,
                                                        const int* done)
{
    const int s = blockIdx.z;
    if (done && done[s] != 0) return;
    const int k2 = blockIdx.x * 64 + threadIdx.x, k1 = blockIdx.y * 4 + threadIdx.y;
    if (k2 >= dct::owners(n2) || k1 >= dct::owners(n1)) return;
    const int p1 = dct::partner(n1, k1), p2 = dct::partner(n2, k2);
    c32* const base = w + (size_t)s * n1 * n2;
    const size_t a00 = (size_t)k1 * n2 + k2, a01 = (size_t)k1 * n2 + p2, a10 = (size_t)p1 * n2 + k2, a11 = (size_t)p1 * n2 + p2;
    // (a self-paired index reads its element twice: the arithmetic below needs no special case, only the stores do)
    c32 v00 = base[a00], v01 = base[a01], v10 = base[a10], v11 = base[a11];
    if (MODE == DCT_FUSED || MODE == DCT_COMBINE) {
        const c32 t2 = t.f2[k2], t2p = t.f2[p2], t1 = t.f1[k1], t1p = t.f1[p1];
        const c32 y00 = v00 * t2 + mul_conj(v01, t2), y01 = v01 * t2p + mul_conj(v00, t2p);
        const c32 y10 = v10 * t2 + mul_conj(v11, t2), y11 = v11 * t2p + mul_conj(v10, t2p);
        v00 = y00 * t1 + mul_conj(y10, t1);
        v10 = y10 * t1p + mul_conj(y00, t1p);
        v01 = y01 * t1 + mul_conj(y11, t1);
        v11 = y11 * t1p + mul_conj(y01, t1p);
    }
    if (MODE == DCT_FUSED || MODE == DCT_SHRINK_SPLIT) {
        const Shrink shr(tau[(size_t)s * niter + iter], op);
        v00 = shr(v00); v01 = shr(v01); v10 = shr(v10); v11 = shr(v11);
    }
    if (MODE != DCT_COMBINE) {
        c32 y00, y01, y10, y11;
        if (k1 == 0) {
            const c32 u = t.i1[0];
            y00 = y10 = v00 * u;
            y01 = y11 = v01 * u;
        } else {
            const c32 u = t.i1[k1], up = t.i1[p1];
            y00 = sub_ib(v00, v10) * u;
            y10 = sub_ib(v10, v00) * up;
            y01 = sub_ib(v01, v11) * u;
            y11 = sub_ib(v11, v01) * up;
        }
        if (k2 == 0) {
            const c32 u = t.i2[0];
            v00 = v01 = y00 * u;
            v10 = v11 = y10 * u;
        } else {
            const c32 u = t.i2[k2], up = t.i2[p2];
            v00 = sub_ib(y00, y01) * u;
            v01 = sub_ib(y01, y00) * up;
            v10 = sub_ib(y10, y11) * u;
            v11 = sub_ib(y11, y10) * up;
        }
    }
    base[a00] = v00;
    if (p2 != k2) base[a01] = v01;
    if (p1 != k1) {
        base[a10] = v10;
        if (p2 != k2) base[a11] = v11;
    }
}

__device__ inline double dct_block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// gen_update_kernel (p3d_generic.hip) with w addressed through the reordering; the arithmetic is the same, expression for expression
__global__ __launch_bounds__(256) void dct_update_kernel(c32* w, const void* x, int dtype, const float* mask, size_t mask_stride, void* out, double* sums, int mode,
                                                         int adaptive, int write_out, float alpha, int n1, int n2, const int* done, int zero_fill)
{
    __shared__ double sh[256];
    const int s = blockIdx.y;
    const size_t per_slice = (size_t)n1 * n2;
    const int dn = done ? done[s] : 0;
    if (zero_fill) {  // final pass: an empty slice is handed back untouched (zeros)
        if (dn < 0)
            for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_slice; i += (size_t)gridDim.x * blockDim.x) {
                if (dtype == 0) reinterpret_cast<c32*>(out)[(size_t)s * per_slice + i] = c32{0.f, 0.f};
                else reinterpret_cast<float*>(out)[(size_t)s * per_slice + i] = 0.f;
            }
    }
    if (dn != 0) return;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_slice; i += (size_t)gridDim.x * blockDim.x) {
        const size_t g = (size_t)s * per_slice + i;
        const int i1 = (int)(i / (size_t)n2), i2 = (int)(i - (size_t)i1 * n2);
        const size_t gw = (size_t)s * per_slice + (size_t)dct::perm(n1, i1) * n2 + dct::perm(n2, i2);
        if (mode == 2) {
            reinterpret_cast<c32*>(out)[g] = w[gw];
            continue;
        }
        c32 xo;
        if (dtype == 0) xo = reinterpret_cast<const c32*>(x)[g];
        else xo = c32{reinterpret_cast<const float*>(x)[g], 0.f};
        const float m = mask ? mask[(size_t)s * mask_stride + i] : 0.f;
        const float wgt = 1.0f - alpha * m;
        c32 xn;
        if (mode == 0) {
            xn = xo;
        } else {
            xn = axpby(w[gw], wgt, xo, alpha);
            if (write_out) {
                if (dtype == 0) reinterpret_cast<c32*>(out)[g] = xn;
                else reinterpret_cast<float*>(out)[g] = xn.x;
            }
        }
        acc += (double)sqrtf(xn.x * xn.x + xn.y * xn.y);
        if (adaptive) {
            const c32 blend = xo * alpha + xn * wgt;
            w[gw] = blend + (xo - xn * m) * (1.0f - alpha);
        } else {
            w[gw] = xn;
        }
    }
    if (mode == 2) return;
    const double tot = dct_block_sum(acc, sh);
    if (threadIdx.x == 0) atomicAdd(sums + s, tot);
}

hipError_t dct_launch_group(int mode, c32* w, const DctTab& tab, const c32* tau, int niter, int iter, int op, int nslices, int n1, int n2,
                            const int* done, hipStream_t st)
{
    const dim3 block(64, 4), grid((unsigned)((dct::owners(n2) + 63) / 64), (unsigned)((dct::owners(n1) + 3) / 4), (unsigned)nslices);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidConfiguration;
    switch (mode) {
        case DCT_FUSED: dct_group_kernel<DCT_FUSED><<<grid, block, 0, st>>>(w, tab, tau, niter, iter, op, n1, n2, done); break;
        case DCT_COMBINE: dct_group_kernel<DCT_COMBINE><<<grid, block, 0, st>>>(w, tab, tau, niter, iter, op, n1, n2, done); break;
        case DCT_SPLIT: dct_group_kernel<DCT_SPLIT><<<grid, block, 0, st>>>(w, tab, tau, niter, iter, op, n1, n2, done); break;
        case DCT_SHRINK_SPLIT: dct_group_kernel<DCT_SHRINK_SPLIT><<<grid, block, 0, st>>>(w, tab, tau, niter, iter, op, n1, n2, done); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dct_launch_update(c32* w, const void* x, int dtype, const float* mask, size_t mask_stride, void* out, double* sums, int mode, int adaptive, int write_out,
                             float alpha, int nslices, int n1, int n2, const int* done, int zero_fill, hipStream_t st)
{
    const size_t per_slice = (size_t)n1 * n2;
    const unsigned bx = (unsigned)((per_slice + 255) / 256 < 256 ? (per_slice + 255) / 256 : 256);
    dct_update_kernel<<<dim3(bx, nslices), 256, 0, st>>>(w, x, dtype, mask, mask_stride, out, sums, mode, adaptive, write_out, alpha, n1, n2, done, zero_fill);
    return hipGetLastError();
}

}  // namespace p3d
