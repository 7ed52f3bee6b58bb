// p3d_vol_dct.hip -- 3-D DCT POCS: a whole (n0, n1, n2) volume as ONE job, the sparsifying transform scipy.fft.dctn / idctn (type 2, norm 'backward' or
// 'ortho') over all three axes (POCS_algorithm with transform=partial(dctn, norm=...) on a (twt, iline, xline) array).
//
// The iterate lives in a complex64 work volume [n0][n1][n2], in the REORDERED sample order of p3d_dct_tables.hpp along axes 1 and 2 (as in p3d_dct.hip) and
// in natural order along axis 0.  One iteration:
//   1. fft2 of the n0 slices: the borrowed p3d_plan's unfused forward passes, in place, max_slices slices per call
//   2. dct_launch_group(DCT_COMBINE): the FFT output becomes the 2-D DCT coefficients of every slice (real and imaginary parts alike)
//   3. voldct_z_kernel: for a tile of W consecutive positions of the n1*n2 plane all n0 points into LDS ([n0][W]), slice z to tile row perm(n0, z) -- the
//      even/odd reordering of axis 0 is part of the load address --, in-place decimation-in-frequency transform along axis 0 (every stage through LDS),
//      then the group step: a thread takes the owners k = 0 ... n0/2 of its column, reads V[k] and V[n0 - k] at their digit-reversed positions, combines
//      them to X[k], X[n0 - k], thresholds (p3d_shrink.hpp), splits to V'[k], V'[n0 - k] and writes both back where they came from; then the transposed
//      inverse, 1/n0, and the store with the reordering of axis 0 undone.  The work volume is read once and written once; the thresholded 3-D cosine
//      spectrum never exists in memory.
//   4. dct_launch_group(DCT_SPLIT)
//   5. ifft2 of the n0 slices
//   6. voldct_update_kernel: re-insertion, the next feed (POCS / FPOCS / APOCS) and sum |x_k| as vol_update_kernel (p3d_vol.hip) computes them, expression for
//      expression, with the reordering of axes 1 and 2 folded into the addressing of the work volume; per-block doubles folded by voldct_fold_kernel in a
//      fixed order (no atomics: the early exit and the results are bitwise repeatable).
// Axis-0 lengths: every 7-smooth n0 in 1 ... 1024 (radices 4, 2, 3, 5, 7; n0 = 1: the group step alone, X = 2 s_0 V).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "p3d_dct.hpp"
#include "p3d_dct_tables.hpp"
#include "p3d_host.hpp"
#include "p3d_shrink.hpp"
#include "p3d_vol_dct_index.hpp"

using namespace p3d;

namespace {

constexpr int VD_MAX_STAGES = voldct::MAX_STAGES;
constexpr int VD_THREADS = voldct::THREADS;
constexpr int VD_FOLD_X = 64;                // update blocks per slice (partial sums: [n0][VD_FOLD_X])
constexpr int VD_STAT = voldct::STAT;        // doubles per block of the statistics pass

enum { Z_FUSED = 0, Z_FWD = 1, Z_INV = 2, Z_STATS = 3 };

struct ZArgs {
    c32* work;
    const c32* tw;              // exp(-2 pi i k / n0), k = 0 .. n0 - 1
    const c32 *f, *g;           // the forward / inverse coefficients of axis 0 for the norm of the call (dct::build_tables)
    const unsigned short* pos;  // pos[k]: where the forward transform leaves coefficient k (voldct::pos_of_coef)
    double* partial;            // Z_STATS: [blocks][VD_STAT]
    size_t plane;               // n1 * n2
    int n0, width, nstage;
    int radix[VD_MAX_STAGES];
    int mode;
    int op;                     // P3D_OP_*, or -1: no threshold
    c32 tau;
    float scale;                // 1 / n0
};

// cos / sin of 2 pi m / R for the odd radices, m folded into 1 .. (R - 1) / 2 by the caller
constexpr float root_cos(int R, int m)
{
    return R == 3 ? -0.5f
         : R == 5 ? (m == 1 ? 0.30901699437494745f : -0.8090169943749475f)
                  : (m == 1 ? 0.6234898018587336f : m == 2 ? -0.2225209339563144f : -0.9009688679024191f);
}
constexpr float root_sin(int R, int m)
{
    return R == 3 ? 0.8660254037844386f
         : R == 5 ? (m == 1 ? 0.9510565162951535f : 0.5877852522924731f)
                  : (m == 1 ? 0.7818314824680298f : m == 2 ? 0.9749279121818236f : 0.4338837391175581f);
}

// natural-order DFT of R points, exp(DIR 2 pi i jk / R)
template <int R, int DIR>
__device__ __forceinline__ void bfly(c32* a)
{
    if constexpr (R == 2) {
        dft2(a[0], a[1]);
    } else if constexpr (R == 4) {
        dft4<DIR>(a[0], a[1], a[2], a[3]);
    } else if constexpr (R > 1) {
        constexpr int H = (R - 1) / 2;
        c32 s[H], d[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            s[j] = a[j + 1] + a[R - 1 - j];
            d[j] = a[j + 1] - a[R - 1 - j];
        }
        const c32 a0 = a[0];
        c32 sum = a0;
#pragma unroll
        for (int j = 0; j < H; ++j) sum = sum + s[j];
#pragma unroll
        for (int k = 1; k <= H; ++k) {
            c32 re = a0, im = c32{0.f, 0.f};
#pragma unroll
            for (int j = 1; j <= H; ++j) {
                const int m = (j * k) % R;
                const int f = m > H ? R - m : m;
                re = re + s[j - 1] * root_cos(R, f);
                im = im + d[j - 1] * (m > H ? -root_sin(R, f) : root_sin(R, f));
            }
            const c32 t = mul_i<DIR>(im);
            a[k] = re + t;
            a[R - k] = re - t;
        }
        a[0] = sum;
    }
}

struct StatAcc {
    float lr = -INFINITY, li = -INFINITY, mx = 0.f, mn = INFINITY;
    double sq = 0.0;
    __device__ __forceinline__ void add(c32 v)
    {
        const float p = v.x * v.x + v.y * v.y;
        if (v.x > lr || (v.x == lr && v.y > li)) { lr = v.x; li = v.y; }
        mx = fmaxf(mx, p);
        mn = fminf(mn, p);
        sq += (double)p;
    }
};

// forward stage on sub-blocks of M = r L points: butterfly, then the twiddle exp(-2 pi i n' k / M) = tw[step n' k]
template <int R>
__device__ __forceinline__ void stage_fwd(c32* col, int W, int base, int L, int twi, const c32* tw)
{
    c32 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = col[(size_t)(base + j * L) * W];
    bfly<R, FWD>(a);
    if (twi != 0) {
#pragma unroll
        for (int k = 1; k < R; ++k) a[k] = a[k] * tw[twi * k];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) col[(size_t)(base + j * L) * W] = a[j];
}

// its transpose with conjugate roots: twiddle, then butterfly
template <int R>
__device__ __forceinline__ void stage_inv(c32* col, int W, int base, int L, int twi, const c32* tw)
{
    c32 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = col[(size_t)(base + j * L) * W];
    if (twi != 0) {
#pragma unroll
        for (int k = 1; k < R; ++k) a[k] = mul_conj(a[k], tw[twi * k]);
    }
    bfly<R, INV>(a);
#pragma unroll
    for (int j = 0; j < R; ++j) col[(size_t)(base + j * L) * W] = a[j];
}

#define VD_RADIX_SWITCH(r, CALL)       \
    switch (r) {                       \
        case 1: { constexpr int R = 1; CALL; } break; \
        case 2: { constexpr int R = 2; CALL; } break; \
        case 3: { constexpr int R = 3; CALL; } break; \
        case 4: { constexpr int R = 4; CALL; } break; \
        case 5: { constexpr int R = 5; CALL; } break; \
        default: { constexpr int R = 7; CALL; } break; \
    }

__global__ __launch_bounds__(VD_THREADS) void voldct_z_kernel(const ZArgs a)
{
    extern __shared__ c32 tile[];   // [n0][W], the n0 roots, the n0 positions; Z_STATS reuses the tile for its reduction (voldct::lds_bytes)
    const int W = a.width, n0 = a.n0;
    c32* const twl = tile + (size_t)n0 * W;
    unsigned short* const posl = reinterpret_cast<unsigned short*>(twl + n0);
    const int w = threadIdx.x % W, r0 = threadIdx.x / W, rows = VD_THREADS / W;
    const size_t pos = (size_t)blockIdx.x * W + w;
    const bool in_range = pos < a.plane;
    c32* const col = tile + w;

    // slice z goes to row perm(n0, z): row p takes slice unperm(n0, p).  Z_INV takes the spectrum in natural order: coefficient k goes to its position
    for (int p = r0; p < n0; p += rows) {
        const int z = a.mode == Z_INV ? voldct::coef_of_pos(n0, a.nstage, a.radix, p) : voldct::unperm(n0, p);
        col[(size_t)p * W] = in_range ? a.work[(size_t)z * a.plane + pos] : c32{0.f, 0.f};
    }
    for (int i = threadIdx.x; i < n0; i += VD_THREADS) {
        twl[i] = a.tw[i];
        posl[i] = a.pos[i];
    }
    __syncthreads();

    const int last = a.nstage - 1;
    if (a.mode != Z_INV) {
        int M = n0;
        for (int s = 0; s <= last; ++s) {
            const int r = a.radix[s], L = M / r, step = n0 / M;
            for (int b = r0; b < n0 / r; b += rows) {
                const int blk = b / L, np = b - blk * L;
                VD_RADIX_SWITCH(r, stage_fwd<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
            M = L;
        }
    }

    // the group step of axis 0 (p3d_dct_tables.hpp): the owner k takes V[k] and V[n0 - k] from their positions, X = combine(V), threshold, V' = split(X),
    // both back to where they came from.  k = 0 and (n0 even) k = n0/2 are their own partners: read twice, stored once
    StatAcc st;
    {
        const Shrink shr(a.tau, a.op < 0 ? 0 : a.op);
        const bool combine = a.mode != Z_INV, split = a.mode == Z_FUSED || a.mode == Z_INV, shrink_on = a.op >= 0 && a.mode != Z_INV;
        for (int k = r0; k <= n0 / 2; k += rows) {
            const int kp = dct::partner(n0, k);
            const size_t ak = (size_t)posl[k] * W, ap = (size_t)posl[kp] * W;
            c32 vk = col[ak], vp = col[ap];
            if (combine) {
                const c32 fk = a.f[k], fp = a.f[kp];
                const c32 xk = vk * fk + mul_conj(vp, fk), xp = vp * fp + mul_conj(vk, fp);
                vk = xk;
                vp = xp;
            }
            if (a.mode == Z_STATS) {
                if (in_range) {
                    st.add(vk);
                    if (kp != k) st.add(vp);
                }
                continue;
            }
            if (shrink_on) {
                vk = shr(vk);
                vp = shr(vp);
            }
            if (split) {
                if (k == 0) {
                    vk = vp = vk * a.g[0];
                } else {
                    const c32 gk = a.g[k], gp = a.g[kp];
                    const c32 yk = sub_ib(vk, vp) * gk, yp = sub_ib(vp, vk) * gp;
                    vk = yk;
                    vp = yp;
                }
            }
            col[ak] = vk;
            if (kp != k) col[ap] = vp;
        }
        __syncthreads();
    }
    if (a.mode == Z_STATS) {   // (every thread is past its last read of the tile)
        double* const st_d = reinterpret_cast<double*>(tile);
        float* const st_f = reinterpret_cast<float*>(st_d + VD_THREADS);
        float* me = st_f + threadIdx.x * 4;
        me[0] = st.lr; me[1] = st.li; me[2] = st.mx; me[3] = st.mn;
        st_d[threadIdx.x] = st.sq;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int t = 1; t < VD_THREADS; ++t) {
                const float* o = st_f + t * 4;
                if (o[0] > st.lr || (o[0] == st.lr && o[1] > st.li)) { st.lr = o[0]; st.li = o[1]; }
                st.mx = fmaxf(st.mx, o[2]);
                st.mn = fminf(st.mn, o[3]);
                st.sq += st_d[t];
            }
            double* o = a.partial + (size_t)blockIdx.x * VD_STAT;
            o[0] = st.lr; o[1] = st.li; o[2] = st.mx; o[3] = st.mn; o[4] = st.sq;
        }
        return;
    }
    if (a.mode != Z_FWD) {
        int M = 1;
        for (int s = last; s >= 0; --s) {
            const int r = a.radix[s], L = M;
            M = L * r;
            const int step = n0 / M;
            for (int b = r0; b < n0 / r; b += rows) {
                const int blk = b / L, np = b - blk * L;
                VD_RADIX_SWITCH(r, stage_inv<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
        }
    }
    // Z_FWD hands the spectrum back in natural order; the others undo the reordering of axis 0
    if (in_range) {
        for (int p = r0; p < n0; p += rows) {
            const int z = a.mode == Z_FWD ? voldct::coef_of_pos(n0, a.nstage, a.radix, p) : voldct::unperm(n0, p);
            const c32 v = col[(size_t)p * W];
            a.work[(size_t)z * a.plane + pos] = a.mode == Z_FWD ? v : v * a.scale;
        }
    }
}

__device__ __forceinline__ double voldct_block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = VD_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// vol_update_kernel (p3d_vol.hip) with w addressed through the reordering of axes 1 and 2: sample (i1, i2) of x, mask and out lives at
// w[z][perm(n1, i1)][perm(n2, i2)]; the arithmetic is the same, expression for expression (grid: VD_FOLD_X x n0).  mode 0 -- w = x or its APOCS mix, partial
// sums of |x| and the count of non-zero samples; mode 1 -- xn = w (1 - alpha m) + alpha x, partial sums of |xn|, optional out = xn, w = xn or its APOCS mix;
// mode 2 -- out = w through the reordering, nothing else (complex64).  mask_stride: plane for a mask per slice, 0 for one shared mask.
__global__ __launch_bounds__(VD_THREADS) void voldct_update_kernel(c32* w, const void* x, int dtype, const float* mask, size_t mask_stride, void* out, double* part,
                                                                   double* part_nz, int mode, int adaptive, int write_out, float alpha, int n1, int n2)
{
    __shared__ double sh[VD_THREADS];
    const size_t z = blockIdx.y, plane = (size_t)n1 * n2;
    double acc = 0.0, nz = 0.0;
    for (size_t i = (size_t)blockIdx.x * VD_THREADS + threadIdx.x; i < plane; i += (size_t)gridDim.x * VD_THREADS) {
        const size_t g = z * plane + i;
        const int i1 = (int)(i / (size_t)n2), i2 = (int)(i - (size_t)i1 * n2);
        const size_t gw = z * plane + (size_t)dct::perm(n1, i1) * n2 + dct::perm(n2, i2);
        if (mode == 2) {
            reinterpret_cast<c32*>(out)[g] = w[gw];
            continue;
        }
        c32 xo;
        if (dtype == P3D_C64) xo = reinterpret_cast<const c32*>(x)[g];
        else xo = c32{reinterpret_cast<const float*>(x)[g], 0.f};
        const float m = mask ? mask[z * mask_stride + i] : 0.f;
        const float wgt = 1.0f - alpha * m;
        c32 xn;
        if (mode == 0) {
            xn = xo;
            nz += (xo.x != 0.f || xo.y != 0.f) ? 1.0 : 0.0;
        } else {
            xn = axpby(w[gw], wgt, xo, alpha);
            if (write_out) {
                if (dtype == P3D_C64) reinterpret_cast<c32*>(out)[g] = xn;
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
    const size_t b = z * gridDim.x + blockIdx.x;
    const double tot = voldct_block_sum(acc, sh);
    if (threadIdx.x == 0) part[b] = tot;
    if (mode == 0) {
        __syncthreads();
        const double cnt = voldct_block_sum(nz, sh);
        if (threadIdx.x == 0) part_nz[b] = cnt;
    }
}

// one workgroup: dst[0] = the n partial sums added in a fixed order (and dst_nz[0] those of part_nz, where given)
__global__ __launch_bounds__(VD_THREADS) void voldct_fold_kernel(const double* part, const double* part_nz, size_t n, double* dst, double* dst_nz)
{
    __shared__ double sh[VD_THREADS];
    double acc = 0.0, nz = 0.0;
    for (size_t i = threadIdx.x; i < n; i += VD_THREADS) {
        acc += part[i];
        if (part_nz) nz += part_nz[i];
    }
    const double tot = voldct_block_sum(acc, sh);
    if (threadIdx.x == 0) dst[0] = tot;
    if (part_nz) {
        __syncthreads();
        const double cnt = voldct_block_sum(nz, sh);
        if (threadIdx.x == 0) dst_nz[0] = cnt;
    }
}

}  // namespace

struct p3d_voldct_plan {
    int device = 0, n0 = 0, n1 = 0, n2 = 0;
    p3d_plan* plan = nullptr;   // the 2-D passes of an (n1, n2) slice
    bool own_plan = false;
    int max_slices = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    c32* work = nullptr;        // [n0][n1][n2]
    c32* tw = nullptr;          // [n0]
    c32* tab = nullptr;         // per norm: forward and inverse coefficients of axis 0, axis 1, axis 2 (dct::build_tables), [2][2 (n0 + n1 + n2)]
    unsigned short* pos = nullptr;   // [n0]
    double* part = nullptr;     // [2][n0 * VD_FOLD_X]: partial sums of |x|, non-zero counts
    double* sums = nullptr;     // device [niter + 2]: sum |x_k|, k = 0 .. niter; the non-zero count of x behind them
    size_t sums_cap = 0;
    double* zpart = nullptr;    // [z blocks][VD_STAT]
    float* mask = nullptr;      // staging of a host mask
    size_t mask_cap = 0;
    void* st_x = nullptr;       // staging of a host volume / of a result that may not go straight to `out`
    void* st_out = nullptr;
    size_t st_x_cap = 0, st_out_cap = 0;   // bytes
    ZArgs z{};
    double prof_z_ms = 0.0;     // P3D_FLAG_PROFILE: mean device time of the axis-0 pass in the last run, and its launches
    int prof_z_n = 0;

    size_t plane() const { return (size_t)n1 * n2; }
    size_t elems() const { return (size_t)n0 * plane(); }
    int zblocks() const { return (int)((plane() + z.width - 1) / z.width); }
    size_t nparts() const { return (size_t)n0 * VD_FOLD_X; }
    size_t tab_len() const { return 2 * ((size_t)n0 + n1 + n2); }
    const c32* f0(int norm) const { return tab + (size_t)norm * tab_len(); }
    const c32* g0(int norm) const { return f0(norm) + n0; }
    DctTab slice_tab(int norm) const
    {
        const c32* b = g0(norm) + n0;
        return DctTab{b, b + n1, b + 2 * (size_t)n1, b + 2 * (size_t)n1 + n2};
    }
};

namespace {

// event pairs around the axis-0 passes of a profiled run, destroyed on scope exit
struct ZProfile {
    std::vector<hipEvent_t> ev;
    ~ZProfile() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int mark(hipStream_t st)
    {
        hipEvent_t e = nullptr;
        P3D_TRY(hipEventCreate(&e));
        ev.push_back(e);
        P3D_TRY(hipEventRecord(e, st));
        return P3D_OK;
    }
};

int grow_bytes(void*& ptr, size_t& cap, size_t bytes)
{
    char* p = static_cast<char*>(ptr);
    const int rc = grow(p, cap, bytes);
    ptr = p;
    return rc;
}

int vd_check(p3d_voldct_plan* v, int norm)
{
    if (!v) return fail(P3D_ERR_INVALID, "NULL volume plan");
    if (norm != P3D_DCT_BACKWARD && norm != P3D_DCT_ORTHO) return fail(P3D_ERR_INVALID, "unknown DCT norm %d", norm);
    P3D_TRY(hipSetDevice(v->device));
    return P3D_OK;
}

// fft2 / ifft2 of every slice of the work volume, max_slices at a time
int vd_fft2(p3d_voldct_plan* v, int inverse)
{
    for (int lo = 0; lo < v->n0; lo += v->max_slices) {
        const int n = v->n0 - lo < v->max_slices ? v->n0 - lo : v->max_slices;
        c32* at = v->work + (size_t)lo * v->plane();
        if (int rc = fft2_async(v->plan, at, at, n, inverse)) return rc;
    }
    return P3D_OK;
}

// the group pass of the two slice axes on every slice: DCT_COMBINE (V -> X) or DCT_SPLIT (X -> V)
int vd_group(p3d_voldct_plan* v, int mode, int norm)
{
    P3D_TRY(dct_launch_group(mode, v->work, v->slice_tab(norm), nullptr, 1, 0, 0, v->n0, v->n1, v->n2, nullptr, v->stream));
    return P3D_OK;
}

int vd_zpass(p3d_voldct_plan* v, int mode, int norm, int op, c32 tau)
{
    ZArgs a = v->z;
    a.mode = mode;
    a.op = op;
    a.tau = tau;
    a.f = v->f0(norm);
    a.g = v->g0(norm);
    const size_t lds = voldct::lds_bytes(v->n0, a.width);
    voldct_z_kernel<<<v->zblocks(), VD_THREADS, lds, v->stream>>>(a);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int vd_update(p3d_voldct_plan* v, const void* x, int dtype, const float* mask, bool per_slice, void* out, int mode, int adaptive, int write_out, float alpha,
              double* dst)
{
    double* const nzp = mode == 0 ? v->part + v->nparts() : nullptr;
    voldct_update_kernel<<<dim3(VD_FOLD_X, v->n0), VD_THREADS, 0, v->stream>>>(v->work, x, dtype, mask, per_slice ? v->plane() : 0, out, v->part, nzp, mode, adaptive,
                                                                              write_out, alpha, v->n1, v->n2);
    if (mode != 2) voldct_fold_kernel<<<1, VD_THREADS, 0, v->stream>>>(v->part, nzp, v->nparts(), dst, mode == 0 ? dst + 1 : nullptr);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

// a volume of `dtype` (host or device) where the kernels can reach it: itself, or the staging volume filled on the plan's stream
int vd_take(p3d_voldct_plan* v, const void* x, int dtype, const void** xd)
{
    *xd = x;
    if (!on_device(v->device, x)) {
        const size_t bytes = elem_bytes(dtype) * v->elems();
        if (int rc = grow_bytes(v->st_x, v->st_x_cap, bytes)) return rc;
        P3D_TRY(hipMemcpyAsync(v->st_x, x, bytes, hipMemcpyDefault, v->stream));
        *xd = v->st_x;
    }
    return P3D_OK;
}

// work = dctn(x) in natural order along all three axes (x: complex64 or float32, host or device), optionally thresholded on the way
int vd_forward(p3d_voldct_plan* v, const void* x, int dtype, int norm, int op, c32 tau)
{
    const void* xd = nullptr;
    int rc = vd_take(v, x, dtype, &xd);
    if (rc) return rc;
    if ((rc = vd_update(v, xd, dtype, nullptr, false, nullptr, 0, 0, 0, 0.0f, v->sums))) return rc;   // work = x, reordered along axes 1 and 2
    if ((rc = vd_fft2(v, 0)) || (rc = vd_group(v, DCT_COMBINE, norm)) || (rc = vd_zpass(v, Z_FWD, norm, op, tau))) return rc;
    return P3D_OK;
}

int vd_dct3(p3d_voldct_plan* v, const void* in, void* out, int norm, int inverse)
{
    int rc = vd_check(v, norm);
    if (rc) return rc;
    if (!in || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    const size_t bytes = sizeof(c32) * v->elems();
    if (!inverse) {
        if ((rc = vd_forward(v, in, P3D_C64, norm, -1, c32{0.f, 0.f}))) return rc;
        P3D_TRY(hipMemcpyAsync(out, v->work, bytes, hipMemcpyDefault, v->stream));
    } else {
        P3D_TRY(hipMemcpyAsync(v->work, in, bytes, hipMemcpyDefault, v->stream));
        if ((rc = vd_zpass(v, Z_INV, norm, -1, c32{0.f, 0.f})) || (rc = vd_group(v, DCT_SPLIT, norm)) || (rc = vd_fft2(v, 1))) return rc;
        void* od = out;
        const bool direct = on_device(v->device, out);
        if (!direct) {
            if ((rc = grow_bytes(v->st_out, v->st_out_cap, bytes))) return rc;
            od = v->st_out;
        }
        if ((rc = vd_update(v, nullptr, P3D_C64, nullptr, false, od, 2, 0, 0, 0.0f, nullptr))) return rc;   // out = work with the reordering undone
        if (!direct) P3D_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDefault, v->stream));
    }
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int vd_stats(p3d_voldct_plan* v, const void* x, int dtype, int norm, double* stats)
{
    int rc = vd_check(v, norm);
    if (rc) return rc;
    if (!x || !stats) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_UNSUPPORTED, "volume dtype %d: complex64 and float32 only", dtype);
    const void* xd = nullptr;
    if ((rc = vd_take(v, x, dtype, &xd))) return rc;
    if ((rc = vd_update(v, xd, dtype, nullptr, false, nullptr, 0, 0, 0, 0.0f, v->sums))) return rc;   // work = x as complex64, reordered
    if ((rc = vd_fft2(v, 0)) || (rc = vd_group(v, DCT_COMBINE, norm)) || (rc = vd_zpass(v, Z_STATS, norm, -1, c32{0.f, 0.f}))) return rc;
    const int nb = v->zblocks();
    std::vector<double> part((size_t)nb * VD_STAT);
    P3D_TRY(hipMemcpyAsync(part.data(), v->zpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    double lr = -INFINITY, li = -INFINITY, mx = 0.0, mn = INFINITY, sq = 0.0;
    for (int b = 0; b < nb; ++b) {   // folded in workgroup order
        const double* q = &part[(size_t)b * VD_STAT];
        if (q[0] > lr || (q[0] == lr && q[1] > li)) { lr = q[0]; li = q[1]; }
        if (q[2] > mx) mx = q[2];
        if (q[3] < mn) mn = q[3];
        sq += q[4];
    }
    stats[0] = lr; stats[1] = li; stats[2] = (double)sqrtf((float)mx); stats[3] = (double)sqrtf((float)mn); stats[4] = sq; stats[5] = 0.0;
    return P3D_OK;
}

int vd_run(p3d_voldct_plan* v, const void* x, int dtype, const float* mask, const double* tau, const p3d_pocs_params* prm, int norm, void* out, int32_t* niter_done,
           double* sums, double* elapsed_ms)
{
    int rc = vd_check(v, norm);
    if (rc) return rc;
    if (!x || !mask || !tau || !prm || !out) return fail(P3D_ERR_INVALID, "NULL argument");
    if (dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_UNSUPPORTED, "volume dtype %d: complex64 and float32 only", dtype);
    if (prm->niter < 1) return fail(P3D_ERR_INVALID, "niter must be >= 1");
    if (prm->thresh_op < P3D_OP_HARD || prm->thresh_op > P3D_OP_GARROTE)
        return fail(P3D_ERR_UNSUPPORTED, "thresh_op %d is not implemented for volumes (hard, soft, garrote)", prm->thresh_op);
    if (prm->version < P3D_VER_REGULAR || prm->version > P3D_VER_ADAPTIVE) return fail(P3D_ERR_INVALID, "unknown version %d", prm->version);
    const int niter = prm->niter, op = prm->thresh_op;
    const bool per_slice = (prm->flags & P3D_FLAG_MASK_PER_SLICE) != 0, adaptive = prm->version == P3D_VER_ADAPTIVE, early = prm->eps > 0.0;
    const bool profile = (prm->flags & P3D_FLAG_PROFILE) != 0;
    ZProfile prof;
    v->prof_z_ms = 0.0;
    v->prof_z_n = 0;
    const float alpha = (float)prm->alpha;
    const size_t bytes = elem_bytes(dtype) * v->elems();

    // the volume, the mask and the result where the kernels can reach them
    const void* xd = nullptr;
    if ((rc = vd_take(v, x, dtype, &xd))) return rc;
    const float* md = mask;
    if (!on_device(v->device, mask)) {
        const size_t nm = per_slice ? v->elems() : v->plane();
        if ((rc = grow(v->mask, v->mask_cap, nm))) return rc;
        P3D_TRY(hipMemcpyAsync(v->mask, mask, sizeof(float) * nm, hipMemcpyDefault, v->stream));
        md = v->mask;
    }
    // every iteration reads x and may write the result: an `out` that overlaps x (or lies on the host) gets the result through the staging buffer
    const char* const xb = static_cast<const char*>(x);
    char* const ob = static_cast<char*>(out);
    const bool direct = on_device(v->device, out) && (ob + bytes <= xb || xb + bytes <= ob);
    void* od = out;
    if (!direct) {
        if ((rc = grow_bytes(v->st_out, v->st_out_cap, bytes))) return rc;
        od = v->st_out;
    }
    if ((rc = grow(v->sums, v->sums_cap, (size_t)niter + 2))) return rc;
    P3D_TRY(hipMemsetAsync(v->sums, 0, sizeof(double) * ((size_t)niter + 2), v->stream));
    P3D_TRY(hipEventRecord(v->ev0, v->stream));

    std::vector<double> sums_h((size_t)niter + 1, 0.0);
    int done = 0;
    // first input; sums[0] = sum |x|; sums[1] is overwritten by the first iteration, the fold leaves the non-zero count there for now
    if ((rc = vd_update(v, xd, dtype, md, per_slice, od, 0, adaptive ? 1 : 0, 0, alpha, v->sums))) return rc;
    double head[2] = {0.0, 0.0};
    P3D_TRY(hipMemcpyAsync(head, v->sums, sizeof head, hipMemcpyDeviceToHost, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    const bool empty = head[1] == 0.0;   // np.count_nonzero(x) == 0: handed back untouched (POCS.py:515-521)
    if (empty) {
        if (direct || !on_device(v->device, out)) {
            P3D_TRY(hipMemcpyAsync(out, xd, bytes, hipMemcpyDefault, v->stream));
        } else if (out != x) {   // a device `out` that overlaps x without being x
            P3D_TRY(hipMemcpyAsync(od, xd, bytes, hipMemcpyDefault, v->stream));
            P3D_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDefault, v->stream));
        }
    } else {
        sums_h[0] = head[0];
        done = niter;
        for (int k = 0; k < niter; ++k) {
            const bool last = k + 1 == niter;
            const c32 t = tau_for_device(tau[2 * k], tau[2 * k + 1], op == P3D_OP_HARD);
            if ((rc = vd_fft2(v, 0)) || (rc = vd_group(v, DCT_COMBINE, norm)) || (profile && (rc = prof.mark(v->stream))) || (rc = vd_zpass(v, Z_FUSED, norm, op, t)) ||
                (profile && (rc = prof.mark(v->stream))) || (rc = vd_group(v, DCT_SPLIT, norm)) || (rc = vd_fft2(v, 1)))
                return rc;
            if ((rc = vd_update(v, xd, dtype, md, per_slice, od, 1, (adaptive && !last) ? 1 : 0, (early || last) ? 1 : 0, alpha, v->sums + k + 1))) return rc;
            if (early) {   // POCS.py:622, 631
                double pair[2];
                P3D_TRY(hipMemcpyAsync(pair, v->sums + k, sizeof pair, hipMemcpyDeviceToHost, v->stream));
                P3D_TRY(hipStreamSynchronize(v->stream));
                const double d = pair[1] - pair[0];
                if (k > 2 && (d * d) / (pair[1] * pair[1]) < prm->eps) {
                    done = k + 1;
                    break;
                }
            }
        }
        P3D_TRY(hipMemcpyAsync(sums_h.data() + 1, v->sums + 1, sizeof(double) * done, hipMemcpyDeviceToHost, v->stream));
        if (!direct) P3D_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDefault, v->stream));
    }
    P3D_TRY(hipEventRecord(v->ev1, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    for (size_t i = 0; i + 1 < prof.ev.size(); i += 2) {
        float ms = 0.f;
        P3D_TRY(hipEventElapsedTime(&ms, prof.ev[i], prof.ev[i + 1]));
        v->prof_z_ms += ms;
        ++v->prof_z_n;
    }
    if (v->prof_z_n) v->prof_z_ms /= v->prof_z_n;
    if (niter_done) *niter_done = done;
    if (sums)
        for (int k = 0; k <= niter; ++k) sums[k] = sums_h[k];
    if (elapsed_ms) {
        float ms = 0.f;
        P3D_TRY(hipEventElapsedTime(&ms, v->ev0, v->ev1));
        *elapsed_ms = ms;
    }
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_voldct_shape_supported(int n0, int n1, int n2)
{
    int radix[VD_MAX_STAGES];
    return (voldct::factor(n0, radix) > 0 && p3d_shape_supported(n1, n2)) ? 1 : 0;
}

int p3d_voldct_plan_destroy(p3d_voldct_plan* v)
{
    if (!v) return P3D_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void* q : {(void*)v->work, (void*)v->tw, (void*)v->tab, (void*)v->pos, (void*)v->part, (void*)v->sums, (void*)v->zpart, (void*)v->mask, v->st_x, v->st_out})
        if (q) (void)hipFree(q);
    if (v->ev0) (void)hipEventDestroy(v->ev0);
    if (v->ev1) (void)hipEventDestroy(v->ev1);
    if (v->own_plan && v->plan) (void)p3d_plan_destroy(v->plan);
    delete v;
    return P3D_OK;
}

int p3d_voldct_plan_create(p3d_voldct_plan** out, int device, int n0, int n1, int n2, p3d_plan* plan)
{
    if (!out) return fail(P3D_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int radix[VD_MAX_STAGES];
    const int nstage = voldct::factor(n0, radix);
    if (nstage < 0)
        return fail(P3D_ERR_UNSUPPORTED, "n0 = %d: the axis-0 transform of a volume takes 7-smooth lengths from 1 to %d", n0, voldct::MAX_N0);
    if (!p3d_shape_supported(n1, n2)) return fail(P3D_ERR_UNSUPPORTED, "slice shape %d x %d is not covered by the HIP kernels", n1, n2);
    if (int rc = use_device(device)) return rc;
    p3d_voldct_plan* v = new p3d_voldct_plan;
    v->device = device; v->n0 = n0; v->n1 = n1; v->n2 = n2;
    int rc = P3D_OK;
    auto bail = [&](int code) { (void)p3d_voldct_plan_destroy(v); return code; };
    if (plan) {
        int pdev = -1, pil = 0, pxl = 0, pmax = 0, single = 0;
        plan_describe(plan, &pdev, &pil, &pxl, &pmax, &single);
        if (pdev != device || pil != n1 || pxl != n2)
            return bail(fail(P3D_ERR_INVALID, "the plan handed over is for %d x %d slices on device %d, the volume needs %d x %d on device %d", pil, pxl, pdev, n1, n2,
                             device));
        v->plan = plan;
        v->max_slices = pmax;
    } else {
        const size_t slice_bytes = sizeof(c32) * v->plane();
        size_t cap = ((size_t)256 << 20) / slice_bytes;   // the plan's own work buffer: about 256 MiB at most
        if (cap < 1) cap = 1;
        v->max_slices = (size_t)n0 < cap ? n0 : (int)cap;
        if ((rc = p3d_plan_create(&v->plan, device, n1, n2, v->max_slices))) return bail(rc);
        v->own_plan = true;
    }
    v->stream = plan_stream(v->plan);
    auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? P3D_OK : fail(P3D_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
    ZArgs& z = v->z;
    z.plane = v->plane();
    z.n0 = n0;
    z.width = voldct::width(n0);
    z.nstage = nstage;
    for (int s = 0; s < nstage; ++s) z.radix[s] = radix[s];
    z.scale = (float)(1.0 / (double)n0);
    std::vector<c32> tw(n0);
    std::vector<unsigned short> pos(n0);
    for (int k = 0; k < n0; ++k) {
        const double ang = -6.283185307179586476925286766559 * (double)k / (double)n0;
        tw[k] = c32{(float)std::cos(ang), (float)std::sin(ang)};
        pos[k] = (unsigned short)voldct::pos_of_coef(n0, nstage, radix, k);
    }
    // the tables of all three axes for both norms, owned by this plan: [norm][f0 g0 f1 i1 f2 i2]
    std::vector<c32> tab(2 * v->tab_len());
    for (int norm = 0; norm < 2; ++norm) {
        c32* b = tab.data() + (size_t)norm * v->tab_len();
        dct::build_tables<c32>(n0, norm, b, b + n0);
        dct::build_tables<c32>(n1, norm, b + 2 * (size_t)n0, b + 2 * (size_t)n0 + n1);
        dct::build_tables<c32>(n2, norm, b + 2 * (size_t)n0 + 2 * (size_t)n1, b + 2 * (size_t)n0 + 2 * (size_t)n1 + n2);
    }
    if ((rc = hip(hipEventCreate(&v->ev0), "hipEventCreate")) || (rc = hip(hipEventCreate(&v->ev1), "hipEventCreate"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->work, sizeof(c32) * v->elems()), "hipMalloc (volume work buffer)"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->tw, sizeof(c32) * (size_t)(n0 < 2 ? 2 : n0)), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMemcpy(v->tw, tw.data(), sizeof(c32) * n0, hipMemcpyHostToDevice), "hipMemcpy"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->pos, sizeof(unsigned short) * (size_t)(n0 < 4 ? 4 : n0)), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMemcpy(v->pos, pos.data(), sizeof(unsigned short) * n0, hipMemcpyHostToDevice), "hipMemcpy"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->tab, sizeof(c32) * tab.size()), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMemcpy(v->tab, tab.data(), sizeof(c32) * tab.size(), hipMemcpyHostToDevice), "hipMemcpy"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->part, sizeof(double) * 2 * v->nparts()), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->zpart, sizeof(double) * VD_STAT * (size_t)v->zblocks()), "hipMalloc"))) return bail(rc);
    if ((rc = grow(v->sums, v->sums_cap, (size_t)64))) return bail(rc);
    z.work = v->work;
    z.tw = v->tw;
    z.pos = v->pos;
    z.partial = v->zpart;
    // the largest tile of any plan (1024 x 16 points, 1024 roots and positions, 138 KiB).  Set at every plan creation: the attribute is kept per device, and
    // a flag latched once per process would leave a second device without it
    if ((rc = hip(hipFuncSetAttribute(reinterpret_cast<const void*>(voldct_z_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)voldct::lds_bytes(voldct::MAX_N0, 16)),
                  "hipFuncSetAttribute")))
        return bail(rc);
    *out = v;
    return P3D_OK;
}

int p3d_voldct_dct3_c64_dev(p3d_voldct_plan* v, const void* in_dev, void* out_dev, int norm, int inverse) { return vd_dct3(v, in_dev, out_dev, norm, inverse); }
int p3d_voldct_dct3_c64(p3d_voldct_plan* v, const void* in_host, void* out_host, int norm, int inverse) { return vd_dct3(v, in_host, out_host, norm, inverse); }

int p3d_voldct_shrink_c64(p3d_voldct_plan* v, const void* in_host, const double* tau, int thresh_op, int norm, void* out_host)
{
    int rc = vd_check(v, norm);
    if (rc) return rc;
    if (!in_host || !out_host || !tau) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (thresh_op < P3D_OP_HARD || thresh_op > P3D_OP_GARROTE) return fail(P3D_ERR_UNSUPPORTED, "thresh_op %d is not implemented", thresh_op);
    if ((rc = vd_forward(v, in_host, P3D_C64, norm, thresh_op, tau_for_device(tau[0], tau[1], thresh_op == P3D_OP_HARD)))) return rc;
    P3D_TRY(hipMemcpyAsync(out_host, v->work, sizeof(c32) * v->elems(), hipMemcpyDefault, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int p3d_voldct_last_profile(p3d_voldct_plan* v, double* zpass_ms, int* zpass_launches)
{
    if (!v || !zpass_ms || !zpass_launches) return fail(P3D_ERR_INVALID, "NULL argument");
    *zpass_ms = v->prof_z_ms;
    *zpass_launches = v->prof_z_n;
    return P3D_OK;
}

int p3d_voldct_stats_dev(p3d_voldct_plan* v, const void* x_dev, int dtype, int norm, double* stats_host) { return vd_stats(v, x_dev, dtype, norm, stats_host); }
int p3d_voldct_stats(p3d_voldct_plan* v, const void* x_host, int dtype, int norm, double* stats_host) { return vd_stats(v, x_host, dtype, norm, stats_host); }

int p3d_voldct_run_dev(p3d_voldct_plan* v, const void* x_dev, int dtype, const float* mask_dev, const double* tau, const p3d_pocs_params* params, int norm,
                       void* out_dev, int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vd_run(v, x_dev, dtype, mask_dev, tau, params, norm, out_dev, niter_done, sums, elapsed_ms);
}
int p3d_voldct_run(p3d_voldct_plan* v, const void* x_host, int dtype, const float* mask_host, const double* tau, const p3d_pocs_params* params, int norm,
                   void* out_host, int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vd_run(v, x_host, dtype, mask_host, tau, params, norm, out_host, niter_done, sums, elapsed_ms);
}

}  // extern "C"
