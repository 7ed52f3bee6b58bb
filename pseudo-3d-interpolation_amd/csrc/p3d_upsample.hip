// p3d_upsample.hip -- iline / xline upsampling of step 15 (the reference's upsample_ilxl, cube_postprocessing_3D.py:350-488, which calls
// xarray's interp_like).  Every output line o of an axis reads source line i0[o] with weight w[o] towards line i0[o] + 1; the host builds
// the two tables per axis from the coordinates (linear / slinear: w = (c_out - c[i0]) / (c[i0 + 1] - c[i0]); nearest: the nearer source line,
// the lower one on an exact tie, w = 0).  The kernel is the separable form
//   out[s][p][q] = (1 - wy) * row(i0y)  +  wy * row(i0y + 1),   row(r) = (1 - wx) * x[s][r][i0x]  +  wx * x[s][r][i0x + 1]
// in float32 (complex64: real and imaginary parts alike), a term with weight 0 is not read -- source lines and `nearest` are copies.
// One thread per output sample, 64-bit indices; slices [nslices][ny][nx] row-major.
#include <hip/hip_runtime.h>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

// C = 1: float32, C = 2: complex64 as interleaved float pairs
template <int C>
__global__ void __launch_bounds__(256) upsample_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ iy,
                                                       const float* __restrict__ wy, const int* __restrict__ ix, const float* __restrict__ wx,
                                                       long long ny, long long nx, long long my, long long mx, long long total)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long per = my * mx, s = i / per, e = i - s * per;
        const long long p = e / mx, q = e - p * mx;
        const long long y0 = iy[p], x0 = ix[q];
        const float fy = wy[p], fx = wx[q];
        const float* base = x + s * ny * nx * C;
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* r0 = base + y0 * nx * C + c;
            float v0 = r0[x0 * C];
            if (fx != 0.0f) v0 = (1.0f - fx) * v0 + fx * r0[(x0 + 1) * C];
            if (fy != 0.0f) {
                const float* r1 = r0 + nx * C;
                float v1 = r1[x0 * C];
                if (fx != 0.0f) v1 = (1.0f - fx) * v1 + fx * r1[(x0 + 1) * C];
                v0 = (1.0f - fy) * v0 + fy * v1;
            }
            acc[c] = v0;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = acc[c];
    }
}

int check_table(const int* idx, const float* w, int n_out, int n_in, const char* axis)
{
    if (!idx || !w || n_out < 1) return fail(P3D_ERR_INVALID, "%s: empty or NULL interpolation table", axis);
    for (int o = 0; o < n_out; ++o) {
        if (idx[o] < 0 || idx[o] >= n_in) return fail(P3D_ERR_INVALID, "%s: source line %d of output line %d outside 0 .. %d", axis, idx[o], o, n_in - 1);
        if (!(w[o] >= 0.0f && w[o] < 1.0f)) return fail(P3D_ERR_INVALID, "%s: weight %g of output line %d outside [0, 1)", axis, (double)w[o], o);
        if (w[o] != 0.0f && idx[o] + 1 >= n_in) return fail(P3D_ERR_INVALID, "%s: output line %d interpolates past the last source line", axis, o);
    }
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_upsample(int device, const void* x, int dtype, size_t nslices, int ny, int nx, const int* iy, const float* wy, int my, const int* ix,
                 const float* wx, int mx, void* out)
{
    if (!x || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (dtype != P3D_F32 && dtype != P3D_C64) return fail(P3D_ERR_INVALID, "dtype %d: float32 (P3D_F32) or complex64 (P3D_C64)", dtype);
    if (nslices < 1 || ny < 1 || nx < 1) return fail(P3D_ERR_INVALID, "bad shape");
    int rc = check_table(iy, wy, my, ny, "iline");
    if (rc) return rc;
    rc = check_table(ix, wx, mx, nx, "xline");
    if (rc) return rc;
    rc = use_device(device);
    if (rc) return rc;

    const int C = dtype == P3D_C64 ? 2 : 1;
    const size_t in_b = (size_t)ny * nx * C * sizeof(float), out_b = (size_t)my * mx * C * sizeof(float);
    size_t free_b = 0, total_b = 0;
    P3D_TRY(hipMemGetInfo(&free_b, &total_b));
    size_t chunk = (free_b / 2) / (in_b + out_b);
    if (chunk > nslices) chunk = nslices;
    if (chunk < 1) return fail(P3D_ERR_UNSUPPORTED, "one %d x %d slice and its upsampled form do not fit in device memory", ny, nx);

    DevBuf din, dout, dt;
    P3D_TRY(hipMalloc(&din.p, in_b * chunk));
    P3D_TRY(hipMalloc(&dout.p, out_b * chunk));
    P3D_TRY(hipMalloc(&dt.p, (sizeof(int) + sizeof(float)) * (size_t)(my + mx)));
    int* d_iy = (int*)dt.p;
    int* d_ix = d_iy + my;
    float* d_wy = (float*)(d_ix + mx);
    float* d_wx = d_wy + my;
    P3D_TRY(hipMemcpy(d_iy, iy, sizeof(int) * my, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(d_ix, ix, sizeof(int) * mx, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(d_wy, wy, sizeof(float) * my, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(d_wx, wx, sizeof(float) * mx, hipMemcpyHostToDevice));
    for (size_t s0 = 0; s0 < nslices; s0 += chunk) {
        const size_t n = nslices - s0 < chunk ? nslices - s0 : chunk;
        P3D_TRY(hipMemcpy(din.p, (const char*)x + s0 * in_b, n * in_b, hipMemcpyHostToDevice));
        const long long total = (long long)n * my * mx;
        const long long b = (total + 255) / 256;
        const unsigned blocks = (unsigned)(b > 65535 * 16 ? 65535 * 16 : b);
        if (C == 2)
            upsample_kernel<2><<<blocks, 256>>>((const float*)din.p, (float*)dout.p, d_iy, d_wy, d_ix, d_wx, ny, nx, my, mx, total);
        else
            upsample_kernel<1><<<blocks, 256>>>((const float*)din.p, (float*)dout.p, d_iy, d_wy, d_ix, d_wx, ny, nx, my, mx, total);
        P3D_TRY(hipGetLastError());
        P3D_TRY(hipMemcpy((char*)out + s0 * out_b, dout.p, n * out_b, hipMemcpyDeviceToHost));
    }
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // extern "C"
