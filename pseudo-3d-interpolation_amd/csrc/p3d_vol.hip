// p3d_vol.hip -- 3-D FFT POCS: a whole (n0, n1, n2) volume as ONE job, the sparsifying transform np.fft.fftn / ifftn over all three axes
// (POCS_algorithm with transform=np.fft.fftn on a (twt, iline, xline) array; Abma & Kabir's 3-D POCS).
//
// One iteration on the complex64 work buffer [n0][n1][n2]:
//   1. fft2 of the n0 slices: the borrowed p3d_plan's unfused forward passes, in place, max_slices slices per call
//   2. vol_z_kernel: for a tile of W consecutive positions of the n1*n2 plane all n0 points into LDS ([n0][W], a tile row is W*8 >= 128 B and
//      a wavefront's loads / stores cover whole rows), in-place decimation-in-frequency transform along axis 0, threshold (p3d_shrink.hpp),
//      the transposed (decimation-in-time) inverse, 1/n0, store.  The forward transform leaves coefficient k at a digit-reversed position;
//      thresholding is pointwise and the transposed inverse takes exactly that order, so no permutation is ever made.  The last forward
//      stage, the threshold and the first inverse stage touch the same r points of a thread and run in its registers.  The work buffer
//      is read once and written once; the thresholded 3-D spectrum never exists in memory.
//   3. ifft2 of the n0 slices (the plan's passes)
//   4. vol_update_kernel: re-insertion x_inv (1 - alpha mask) + alpha x, the next feed (POCS / FPOCS / APOCS as gen_update_kernel builds it), and
//      sum |x_k| over the whole volume as per-block doubles folded by vol_fold_kernel in a fixed order (no atomics: the early exit and the
//      results are bitwise repeatable).
// Axis-0 lengths: every 7-smooth n0 in 1 ... 1024 (radices 4, 2, 3, 5, 7; n0 = 1: the z-pass thresholds only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "p3d_host.hpp"
#include "p3d_shrink.hpp"

using namespace p3d;

namespace {

constexpr int VOL_MAX_N0 = 1024;
constexpr int VOL_MAX_STAGES = 10;   // 2^10
constexpr int VOL_THREADS = 256;
constexpr int VOL_FOLD_X = 64;       // update blocks per slice (partial sums: [n0][VOL_FOLD_X])
constexpr int VOL_STAT = 5;          // doubles per block of the statistics pass

enum { Z_FUSED = 0, Z_FWD = 1, Z_INV = 2, Z_STATS = 3 };

struct ZArgs {
    c32* work;
    const c32* tw;      // exp(-2 pi i k / n0), k = 0 .. n0 - 1
    double* partial;    // Z_STATS: [blocks][VOL_STAT]
    size_t plane;       // n1 * n2
    int n0, width, nstage;
    int radix[VOL_MAX_STAGES];
    int mode;
    int op;             // P3D_OP_*, or -1: no threshold (Z_FWD)
    c32 tau;
    float scale;        // 1 / n0
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

// the innermost stage (L = 1, no twiddles) of both directions around the threshold, in registers
template <int R>
__device__ __forceinline__ void stage_mid(c32* col, int W, int base, int mode, bool shrink_on, const Shrink& shr, StatAcc& st, bool in_range)
{
    c32 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = col[(size_t)(base + j) * W];
    if (mode != Z_INV) {
        bfly<R, FWD>(a);
        if (mode == Z_STATS) {
            if (in_range) {
#pragma unroll
                for (int j = 0; j < R; ++j) st.add(a[j]);
            }
            return;
        }
        if (shrink_on) {
#pragma unroll
            for (int j = 0; j < R; ++j) a[j] = shr(a[j]);
        }
    }
    if (mode != Z_FWD) bfly<R, INV>(a);
#pragma unroll
    for (int j = 0; j < R; ++j) col[(size_t)(base + j) * W] = a[j];
}

#define VOL_RADIX_SWITCH(r, CALL)      \
    switch (r) {                       \
        case 1: { constexpr int R = 1; CALL; } break; \
        case 2: { constexpr int R = 2; CALL; } break; \
        case 3: { constexpr int R = 3; CALL; } break; \
        case 4: { constexpr int R = 4; CALL; } break; \
        case 5: { constexpr int R = 5; CALL; } break; \
        default: { constexpr int R = 7; CALL; } break; \
    }

// position p of the transformed column holds coefficient k: p = k_1 n0/r_1 + k_2 n0/(r_1 r_2) + ..., k = k_1 + r_1 k_2 + r_1 r_2 k_3 + ...
__device__ __forceinline__ int coef_of_pos(const ZArgs& a, int p)
{
    int k = 0, mult = 1, M = a.n0;
    for (int s = 0; s < a.nstage; ++s) {
        const int r = a.radix[s], L = M / r, d = p / L;
        p -= d * L;
        k += d * mult;
        mult *= r;
        M = L;
    }
    return k;
}

__global__ __launch_bounds__(VOL_THREADS) void vol_z_kernel(const ZArgs a)
{
    extern __shared__ c32 tile[];   // [n0][W], then the n0 twiddles; Z_STATS reuses the tile for its reduction (vol_lds_bytes)
    const int W = a.width, n0 = a.n0;
    c32* const twl = tile + (size_t)n0 * W;
    const int w = threadIdx.x % W, r0 = threadIdx.x / W, rows = VOL_THREADS / W;
    const size_t pos = (size_t)blockIdx.x * W + w;
    const bool in_range = pos < a.plane;
    c32* const col = tile + w;

    // Z_INV takes the spectrum in natural order: coefficient k goes to its digit-reversed position
    for (int p = r0; p < n0; p += rows) {
        const int z = a.mode == Z_INV ? coef_of_pos(a, p) : p;
        col[(size_t)p * W] = in_range ? a.work[(size_t)z * a.plane + pos] : c32{0.f, 0.f};
    }
    for (int i = threadIdx.x; i < n0; i += VOL_THREADS) twl[i] = a.tw[i];
    __syncthreads();

    const int last = a.nstage - 1;
    if (a.mode != Z_INV) {
        int M = n0;
        for (int s = 0; s < last; ++s) {
            const int r = a.radix[s], L = M / r, step = n0 / M;
            for (int b = r0; b < n0 / r; b += rows) {
                const int blk = b / L, np = b - blk * L;
                VOL_RADIX_SWITCH(r, stage_fwd<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
            M = L;
        }
    }
    StatAcc st;
    {
        const Shrink shr(a.tau, a.op < 0 ? 0 : a.op);
        const int r = a.radix[last];
        for (int b = r0; b < n0 / r; b += rows) {
            VOL_RADIX_SWITCH(r, stage_mid<R>(col, W, b * r, a.mode, a.op >= 0, shr, st, in_range));
        }
        __syncthreads();
    }
    if (a.mode == Z_STATS) {   // (every thread is past its last read of the tile)
        double* const st_d = reinterpret_cast<double*>(tile);
        float* const st_f = reinterpret_cast<float*>(st_d + VOL_THREADS);
        float* me = st_f + threadIdx.x * 4;
        me[0] = st.lr; me[1] = st.li; me[2] = st.mx; me[3] = st.mn;
        st_d[threadIdx.x] = st.sq;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int t = 1; t < VOL_THREADS; ++t) {
                const float* o = st_f + t * 4;
                if (o[0] > st.lr || (o[0] == st.lr && o[1] > st.li)) { st.lr = o[0]; st.li = o[1]; }
                st.mx = fmaxf(st.mx, o[2]);
                st.mn = fminf(st.mn, o[3]);
                st.sq += st_d[t];
            }
            double* o = a.partial + (size_t)blockIdx.x * VOL_STAT;
            o[0] = st.lr; o[1] = st.li; o[2] = st.mx; o[3] = st.mn; o[4] = st.sq;
        }
        return;
    }
    if (a.mode != Z_FWD) {
        int M = a.radix[last];
        for (int s = last - 1; s >= 0; --s) {
            const int r = a.radix[s], L = M;
            M = L * r;
            const int step = n0 / M;
            for (int b = r0; b < n0 / r; b += rows) {
                const int blk = b / L, np = b - blk * L;
                VOL_RADIX_SWITCH(r, stage_inv<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
        }
    }
    // Z_FWD hands the spectrum back in natural order
    if (in_range) {
        for (int p = r0; p < n0; p += rows) {
            const int z = a.mode == Z_FWD ? coef_of_pos(a, p) : p;
            const c32 v = col[(size_t)p * W];
            a.work[(size_t)z * a.plane + pos] = a.mode == Z_FWD ? v : v * a.scale;
        }
    }
}

__device__ __forceinline__ double vol_block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = VOL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// gen_update_kernel for a volume (grid: VOL_FOLD_X x n0): mode 0 -- w = x or its APOCS mix, partial sums of |x| and the count of non-zero samples;
// mode 1 -- xn = w (1 - alpha m) + alpha x, partial sums of |xn|, optional out = xn, w = xn or its APOCS mix.  mask_stride: plane for a mask per
// slice, 0 for one shared mask.
__global__ __launch_bounds__(VOL_THREADS) void vol_update_kernel(c32* w, const void* x, int dtype, const float* mask, size_t mask_stride, void* out, double* part,
                                                                 double* part_nz, int mode, int adaptive, int write_out, float alpha, size_t plane)
{
    __shared__ double sh[VOL_THREADS];
    const size_t z = blockIdx.y;
    double acc = 0.0, nz = 0.0;
    for (size_t i = (size_t)blockIdx.x * VOL_THREADS + threadIdx.x; i < plane; i += (size_t)gridDim.x * VOL_THREADS) {
        const size_t g = z * plane + i;
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
            xn = axpby(w[g], wgt, xo, alpha);
            if (write_out) {
                if (dtype == P3D_C64) reinterpret_cast<c32*>(out)[g] = xn;
                else reinterpret_cast<float*>(out)[g] = xn.x;
            }
        }
        acc += (double)sqrtf(xn.x * xn.x + xn.y * xn.y);
        if (adaptive) {
            const c32 blend = xo * alpha + xn * wgt;
            w[g] = blend + (xo - xn * m) * (1.0f - alpha);
        } else {
            w[g] = xn;
        }
    }
    const size_t b = z * gridDim.x + blockIdx.x;
    const double tot = vol_block_sum(acc, sh);
    if (threadIdx.x == 0) part[b] = tot;
    if (mode == 0) {
        __syncthreads();
        const double cnt = vol_block_sum(nz, sh);
        if (threadIdx.x == 0) part_nz[b] = cnt;
    }
}

// one workgroup: dst[0] = the n partial sums added in a fixed order (and dst_nz[0] those of part_nz, where given)
__global__ __launch_bounds__(VOL_THREADS) void vol_fold_kernel(const double* part, const double* part_nz, size_t n, double* dst, double* dst_nz)
{
    __shared__ double sh[VOL_THREADS];
    double acc = 0.0, nz = 0.0;
    for (size_t i = threadIdx.x; i < n; i += VOL_THREADS) {
        acc += part[i];
        if (part_nz) nz += part_nz[i];
    }
    const double tot = vol_block_sum(acc, sh);
    if (threadIdx.x == 0) dst[0] = tot;
    if (part_nz) {
        __syncthreads();
        const double cnt = vol_block_sum(nz, sh);
        if (threadIdx.x == 0) dst_nz[0] = cnt;
    }
}

// dynamic LDS of vol_z_kernel: the tile and the twiddles, at least the scratch of the statistics reduction
size_t vol_lds_bytes(int n0, int width)
{
    const size_t tile = sizeof(c32) * ((size_t)n0 * width + n0), scratch = (sizeof(double) + 4 * sizeof(float)) * VOL_THREADS;
    return tile > scratch ? tile : scratch;
}

// radices of a 7-smooth n (4s first, then 2, 3, 5, 7); n = 1: one stage of radix 1.  Returns the stage count, or -1
int vol_factor(int n, int* radix)
{
    if (n < 1 || n > VOL_MAX_N0) return -1;
    int ns = 0;
    if (n == 1) { radix[0] = 1; return 1; }
    while (n % 4 == 0) { radix[ns++] = 4; n /= 4; }
    const int rest[4] = {2, 3, 5, 7};
    for (int r : rest)
        while (n % r == 0) { radix[ns++] = r; n /= r; }
    return n == 1 ? ns : -1;
}

// tile width: 64 positions (rows of 512 B) while the tile stays within 32 KiB -- four workgroups then share a compute unit's LDS --, never below 16 (128 B)
int vol_width(int n0)
{
    int w = 64;
    while (w > 16 && sizeof(c32) * (size_t)n0 * w > 32768) w >>= 1;
    return w;
}

}  // namespace

struct p3d_vol_plan {
    int device = 0, n0 = 0, n1 = 0, n2 = 0;
    p3d_plan* plan = nullptr;   // the 2-D passes of an (n1, n2) slice
    bool own_plan = false;
    int max_slices = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    c32* work = nullptr;        // [n0][n1][n2]
    c32* tw = nullptr;          // [n0]
    double* part = nullptr;     // [2][n0 * VOL_FOLD_X]: partial sums of |x|, non-zero counts
    double* sums = nullptr;     // device [niter + 2]: sum |x_k|, k = 0 .. niter; the non-zero count of x behind them
    size_t sums_cap = 0;
    double* zpart = nullptr;    // [z blocks][VOL_STAT]
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
    size_t nparts() const { return (size_t)n0 * VOL_FOLD_X; }
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

int vol_check(p3d_vol_plan* v)
{
    if (!v) return fail(P3D_ERR_INVALID, "NULL volume plan");
    P3D_TRY(hipSetDevice(v->device));
    return P3D_OK;
}

// fft2 / ifft2 of every slice of the work buffer, max_slices at a time
int vol_fft2(p3d_vol_plan* v, int inverse)
{
    for (int lo = 0; lo < v->n0; lo += v->max_slices) {
        const int n = v->n0 - lo < v->max_slices ? v->n0 - lo : v->max_slices;
        c32* at = v->work + (size_t)lo * v->plane();
        if (int rc = fft2_async(v->plan, at, at, n, inverse)) return rc;
    }
    return P3D_OK;
}

int vol_zpass(p3d_vol_plan* v, int mode, int op, c32 tau)
{
    ZArgs a = v->z;
    a.mode = mode;
    a.op = op;
    a.tau = tau;
    const size_t lds = vol_lds_bytes(v->n0, a.width);
    vol_z_kernel<<<v->zblocks(), VOL_THREADS, lds, v->stream>>>(a);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int vol_update(p3d_vol_plan* v, const void* x, int dtype, const float* mask, bool per_slice, void* out, int mode, int adaptive, int write_out, float alpha, double* dst)
{
    double* const nzp = mode == 0 ? v->part + v->nparts() : nullptr;
    vol_update_kernel<<<dim3(VOL_FOLD_X, v->n0), VOL_THREADS, 0, v->stream>>>(v->work, x, dtype, mask, per_slice ? v->plane() : 0, out, v->part, nzp, mode, adaptive,
                                                                             write_out, alpha, v->plane());
    vol_fold_kernel<<<1, VOL_THREADS, 0, v->stream>>>(v->part, nzp, v->nparts(), dst, mode == 0 ? dst + 1 : nullptr);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

// `src` (host or device, complex64) into the work buffer
int vol_load_c64(p3d_vol_plan* v, const void* src)
{
    if (src != v->work) P3D_TRY(hipMemcpyAsync(v->work, src, sizeof(c32) * v->elems(), hipMemcpyDefault, v->stream));
    return P3D_OK;
}

int vol_fft3(p3d_vol_plan* v, const void* in, void* out, int inverse)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!in || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if ((rc = vol_load_c64(v, in))) return rc;
    if (!inverse) {
        if ((rc = vol_fft2(v, 0)) || (rc = vol_zpass(v, Z_FWD, -1, c32{0.f, 0.f}))) return rc;
    } else {
        if ((rc = vol_zpass(v, Z_INV, -1, c32{0.f, 0.f})) || (rc = vol_fft2(v, 1))) return rc;
    }
    if (out != v->work) P3D_TRY(hipMemcpyAsync(out, v->work, sizeof(c32) * v->elems(), hipMemcpyDefault, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int vol_stats(p3d_vol_plan* v, const void* x, int dtype, double* stats)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!x || !stats) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_UNSUPPORTED, "volume dtype %d: complex64 and float32 only", dtype);
    const void* xd = x;
    if (!on_device(v->device, x)) {
        const size_t bytes = elem_bytes(dtype) * v->elems();
        if ((rc = grow_bytes(v->st_x, v->st_x_cap, bytes))) return rc;
        P3D_TRY(hipMemcpyAsync(v->st_x, x, bytes, hipMemcpyDefault, v->stream));
        xd = v->st_x;
    }
    if ((rc = vol_update(v, xd, dtype, nullptr, false, nullptr, 0, 0, 0, 0.0f, v->sums))) return rc;   // work = x as complex64
    if ((rc = vol_fft2(v, 0)) || (rc = vol_zpass(v, Z_STATS, -1, c32{0.f, 0.f}))) return rc;
    const int nb = v->zblocks();
    std::vector<double> part((size_t)nb * VOL_STAT);
    P3D_TRY(hipMemcpyAsync(part.data(), v->zpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    double lr = -INFINITY, li = -INFINITY, mx = 0.0, mn = INFINITY, sq = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double* q = &part[(size_t)b * VOL_STAT];
        if (q[0] > lr || (q[0] == lr && q[1] > li)) { lr = q[0]; li = q[1]; }
        if (q[2] > mx) mx = q[2];
        if (q[3] < mn) mn = q[3];
        sq += q[4];
    }
    stats[0] = lr; stats[1] = li; stats[2] = (double)sqrtf((float)mx); stats[3] = (double)sqrtf((float)mn); stats[4] = sq; stats[5] = 0.0;
    return P3D_OK;
}

int vol_run(p3d_vol_plan* v, const void* x, int dtype, const float* mask, const double* tau, const p3d_pocs_params* prm, void* out, int32_t* niter_done,
            double* sums, double* elapsed_ms)
{
    int rc = vol_check(v);
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
    const void* xd = x;
    if (!on_device(v->device, x)) {
        if ((rc = grow_bytes(v->st_x, v->st_x_cap, bytes))) return rc;
        P3D_TRY(hipMemcpyAsync(v->st_x, x, bytes, hipMemcpyDefault, v->stream));
        xd = v->st_x;
    }
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
    if ((rc = vol_update(v, xd, dtype, md, per_slice, od, 0, adaptive ? 1 : 0, 0, alpha, v->sums))) return rc;
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
            if ((rc = vol_fft2(v, 0)) || (profile && (rc = prof.mark(v->stream))) || (rc = vol_zpass(v, Z_FUSED, op, t)) || (profile && (rc = prof.mark(v->stream))) ||
                (rc = vol_fft2(v, 1)))
                return rc;
            if ((rc = vol_update(v, xd, dtype, md, per_slice, od, 1, (adaptive && !last) ? 1 : 0, (early || last) ? 1 : 0, alpha, v->sums + k + 1))) return rc;
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

int p3d_vol_shape_supported(int n0, int n1, int n2)
{
    int radix[VOL_MAX_STAGES];
    return (vol_factor(n0, radix) > 0 && p3d_shape_supported(n1, n2)) ? 1 : 0;
}

int p3d_vol_plan_destroy(p3d_vol_plan* v)
{
    if (!v) return P3D_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void* q : {(void*)v->work, (void*)v->tw, (void*)v->part, (void*)v->sums, (void*)v->zpart, (void*)v->mask, v->st_x, v->st_out})
        if (q) (void)hipFree(q);
    if (v->ev0) (void)hipEventDestroy(v->ev0);
    if (v->ev1) (void)hipEventDestroy(v->ev1);
    if (v->own_plan && v->plan) (void)p3d_plan_destroy(v->plan);
    delete v;
    return P3D_OK;
}

int p3d_vol_plan_create(p3d_vol_plan** out, int device, int n0, int n1, int n2, p3d_plan* plan)
{
    if (!out) return fail(P3D_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int radix[VOL_MAX_STAGES];
    const int nstage = vol_factor(n0, radix);
    if (nstage < 0)
        return fail(P3D_ERR_UNSUPPORTED, "n0 = %d: the axis-0 transform of a volume takes 7-smooth lengths from 1 to %d", n0, VOL_MAX_N0);
    if (!p3d_shape_supported(n1, n2)) return fail(P3D_ERR_UNSUPPORTED, "slice shape %d x %d is not covered by the HIP kernels", n1, n2);
    if (int rc = use_device(device)) return rc;
    p3d_vol_plan* v = new p3d_vol_plan;
    v->device = device; v->n0 = n0; v->n1 = n1; v->n2 = n2;
    int rc = P3D_OK;
    auto bail = [&](int code) { (void)p3d_vol_plan_destroy(v); return code; };
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
    z.width = vol_width(n0);
    z.nstage = nstage;
    for (int s = 0; s < nstage; ++s) z.radix[s] = radix[s];
    z.scale = (float)(1.0 / (double)n0);
    std::vector<c32> tw(n0);
    for (int k = 0; k < n0; ++k) {
        const double ang = -6.283185307179586476925286766559 * (double)k / (double)n0;
        tw[k] = c32{(float)std::cos(ang), (float)std::sin(ang)};
    }
    if ((rc = hip(hipEventCreate(&v->ev0), "hipEventCreate")) || (rc = hip(hipEventCreate(&v->ev1), "hipEventCreate"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->work, sizeof(c32) * v->elems()), "hipMalloc (volume work buffer)"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->tw, sizeof(c32) * (size_t)(n0 < 2 ? 2 : n0)), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMemcpy(v->tw, tw.data(), sizeof(c32) * n0, hipMemcpyHostToDevice), "hipMemcpy"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->part, sizeof(double) * 2 * v->nparts()), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->zpart, sizeof(double) * VOL_STAT * (size_t)v->zblocks()), "hipMalloc"))) return bail(rc);
    if ((rc = grow(v->sums, v->sums_cap, (size_t)64))) return bail(rc);
    z.work = v->work;
    z.tw = v->tw;
    z.partial = v->zpart;
    // the largest tile of any plan (1024 x 16 points and 1024 twiddles, 136 KiB): the attribute belongs to the kernel, not to the plan
    if ((rc = hip(hipFuncSetAttribute(reinterpret_cast<const void*>(vol_z_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vol_lds_bytes(VOL_MAX_N0, 16)),
                  "hipFuncSetAttribute")))
        return bail(rc);
    *out = v;
    return P3D_OK;
}

int p3d_vol_fft3_c64_dev(p3d_vol_plan* v, const void* in_dev, void* out_dev, int inverse) { return vol_fft3(v, in_dev, out_dev, inverse); }
int p3d_vol_fft3_c64(p3d_vol_plan* v, const void* in_host, void* out_host, int inverse) { return vol_fft3(v, in_host, out_host, inverse); }

int p3d_vol_shrink_c64(p3d_vol_plan* v, const void* in_host, const double* tau, int thresh_op, void* out_host)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!in_host || !out_host || !tau) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (thresh_op < P3D_OP_HARD || thresh_op > P3D_OP_GARROTE) return fail(P3D_ERR_UNSUPPORTED, "thresh_op %d is not implemented", thresh_op);
    if ((rc = vol_load_c64(v, in_host)) || (rc = vol_fft2(v, 0))) return rc;
    if ((rc = vol_zpass(v, Z_FWD, thresh_op, tau_for_device(tau[0], tau[1], thresh_op == P3D_OP_HARD)))) return rc;
    P3D_TRY(hipMemcpyAsync(out_host, v->work, sizeof(c32) * v->elems(), hipMemcpyDefault, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int p3d_vol_last_profile(p3d_vol_plan* v, double* zpass_ms, int* zpass_launches)
{
    if (!v || !zpass_ms || !zpass_launches) return fail(P3D_ERR_INVALID, "NULL argument");
    *zpass_ms = v->prof_z_ms;
    *zpass_launches = v->prof_z_n;
    return P3D_OK;
}

int p3d_vol_stats_dev(p3d_vol_plan* v, const void* x_dev, int dtype, double* stats_host) { return vol_stats(v, x_dev, dtype, stats_host); }
int p3d_vol_stats(p3d_vol_plan* v, const void* x_host, int dtype, double* stats_host) { return vol_stats(v, x_host, dtype, stats_host); }

int p3d_vol_run_dev(p3d_vol_plan* v, const void* x_dev, int dtype, const float* mask_dev, const double* tau, const p3d_pocs_params* params, void* out_dev,
                    int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vol_run(v, x_dev, dtype, mask_dev, tau, params, out_dev, niter_done, sums, elapsed_ms);
}
int p3d_vol_run(p3d_vol_plan* v, const void* x_host, int dtype, const float* mask_host, const double* tau, const p3d_pocs_params* params, void* out_host,
                int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vol_run(v, x_host, dtype, mask_host, tau, params, out_host, niter_done, sums, elapsed_ms);
}

}  // extern "C"
