// p3d_vol64.hip -- 3-D FFT POCS in double precision: the loop of p3d_vol.hip on a complex128 work volume, what the reference computes when it is handed a
// double volume with transform=np.fft.fftn (POCS.py:566-575, 616: complex128 / float64 throughout).
//
// One iteration on the complex128 work buffer [n0][n1][n2]:
//   1. fft2 of the n0 slices: the line passes of a p3d_plan64 for (n1, n2) slices (plan64_fft2), in place, max_slices slices per call
//   2. vol64_z_kernel: for a tile of W consecutive positions of the n1*n2 plane all n0 points into LDS ([n0][W], W = 32 / 16 / 8: a tile row is at least
//      128 B), in-place decimation-in-frequency transform along axis 0, shrink64 (NumPy's threshold semantics in double, p3d_f64.hpp), the transposed
//      (decimation-in-time) inverse with conjugate roots, 1/n0, store.  No permutation: the forward transform leaves coefficient k at a digit-reversed
//      position, the threshold is pointwise and the transposed inverse takes exactly that order.  The last forward stage, the threshold and the first
//      inverse stage run in registers.  The work buffer is read once and written once; the thresholded 3-D spectrum never exists in memory.
//      Elements move as 128-bit LDS and global accesses.
//   3. ifft2 of the n0 slices (the plan's passes)
//   4. vol64_update_kernel: re-insertion x_inv (1 - alpha mask) + alpha x with a double mask, the next feed (POCS / FPOCS / APOCS expression for expression
//      as update64_kernel of p3d_f64.hip builds it), and sum |x_k| as per-workgroup doubles folded by vol64_fold_kernel in a fixed order (no atomics: results,
//      costs and the early exit are bitwise repeatable).
// Axis-0 lengths: every 7-smooth n0 in 1 ... 1024 (radices 4, 2, 3, 5, 7; n0 = 1: the z-pass thresholds only).  x and out: complex128, float64, complex64 or
// float32, converted on load and store; real volumes run as complex with a zero imaginary part.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "p3d_f64.hpp"
#include "p3d_host.hpp"
#include "p3d_vol64_index.hpp"

using namespace p3d;
using p3d::f64::c64;
using p3d::f64::shrink64;

namespace {

namespace vx = p3d::vol64;
constexpr int V64_THREADS = vx::THREADS;
constexpr int V64_FOLD_X = 64;       // update workgroups per slice (partial sums: [n0][V64_FOLD_X])
constexpr int V64_STAT = vx::STAT;

enum { Z_FUSED = 0, Z_FWD = 1, Z_INV = 2, Z_STATS = 3 };

struct Z64Args {
    c64* work;
    const c64* tw;      // exp(-2 pi i k / n0), k = 0 .. n0 - 1
    double* partial;    // Z_STATS: [workgroups][V64_STAT]
    size_t plane;       // n1 * n2
    int n0, width, nstage;
    int radix[vx::MAX_STAGES];
    int mode;
    int op;             // P3D_OP_*, or -1: no threshold (Z_FWD)
    c64 tau;
    double scale;       // 1 / n0
};

// cos / sin of 2 pi m / R for the odd radices, m folded into 1 .. (R - 1) / 2 by the caller
constexpr double root_cos(int R, int m)
{
    return R == 3 ? -0.5
         : R == 5 ? (m == 1 ? 0.30901699437494742410 : -0.80901699437494742410)
                  : (m == 1 ? 0.62348980185873353053 : m == 2 ? -0.22252093395631440429 : -0.90096886790241912624);
}
constexpr double root_sin(int R, int m)
{
    return R == 3 ? 0.86602540378443864676
         : R == 5 ? (m == 1 ? 0.95105651629515357212 : 0.58778525229247312917)
                  : (m == 1 ? 0.78183148246802980871 : m == 2 ? 0.97492791218182360702 : 0.43388373911755812048);
}

// -i v (forward) / +i v (inverse)
template <bool INVERSE>
__device__ __forceinline__ c64 times_i(c64 v)
{
    return INVERSE ? c64{-v.y, v.x} : c64{v.y, -v.x};
}
__device__ __forceinline__ c64 mul_conj(c64 a, c64 w) { return {a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y}; }

// natural-order DFT of R points, exp(-+ 2 pi i jk / R)
template <int R, bool INVERSE>
__device__ __forceinline__ void bfly(c64* a)
{
    if constexpr (R == 2) {
        const c64 t = a[0] - a[1];
        a[0] = a[0] + a[1];
        a[1] = t;
    } else if constexpr (R == 4) {
        const c64 s02 = a[0] + a[2], d02 = a[0] - a[2], s13 = a[1] + a[3], d13 = times_i<INVERSE>(a[1] - a[3]);
        a[0] = s02 + s13;
        a[1] = d02 + d13;
        a[2] = s02 - s13;
        a[3] = d02 - d13;
    } else if constexpr (R > 1) {
        constexpr int H = (R - 1) / 2;
        c64 s[H], d[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            s[j] = a[j + 1] + a[R - 1 - j];
            d[j] = a[j + 1] - a[R - 1 - j];
        }
        const c64 a0 = a[0];
        c64 sum = a0;
#pragma unroll
        for (int j = 0; j < H; ++j) sum = sum + s[j];
#pragma unroll
        for (int k = 1; k <= H; ++k) {
            c64 re = a0, im = c64{0.0, 0.0};
#pragma unroll
            for (int j = 1; j <= H; ++j) {
                const int m = (j * k) % R;
                const int f = m > H ? R - m : m;
                re = re + s[j - 1] * root_cos(R, f);
                im = im + d[j - 1] * (m > H ? -root_sin(R, f) : root_sin(R, f));
            }
            const c64 t = times_i<INVERSE>(im);
            a[k] = re + t;
            a[R - k] = re - t;
        }
        a[0] = sum;
    }
}

// every reduction in double; the peak is NumPy's complex maximum (lexicographic), as stats64_kernel of p3d_f64.hip
struct StatAcc {
    double lr = -INFINITY, li = -INFINITY, mx = 0.0, mn = INFINITY, sq = 0.0;
    __device__ __forceinline__ void add(c64 v)
    {
        const double m = hypot(v.x, v.y);
        if (v.x > lr || (v.x == lr && v.y > li)) { lr = v.x; li = v.y; }
        mx = fmax(mx, m);
        mn = fmin(mn, m);
        sq += v.x * v.x + v.y * v.y;
    }
};

// the element of tile row p in this thread's column
#define V64_AT(p) col[(size_t)(p) * W]

// forward stage on sub-blocks of M = r L points: butterfly, then the twiddle exp(-2 pi i n' k / M) = tw[step n' k]
template <int R>
__device__ __forceinline__ void stage_fwd(c64* col, int W, int base, int L, int twi, const c64* tw)
{
    c64 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = V64_AT(base + j * L);
    bfly<R, false>(a);
    if (twi != 0) {
#pragma unroll
        for (int k = 1; k < R; ++k) a[k] = a[k] * tw[twi * k];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) V64_AT(base + j * L) = a[j];
}

// its transpose with conjugate roots: twiddle, then butterfly
template <int R>
__device__ __forceinline__ void stage_inv(c64* col, int W, int base, int L, int twi, const c64* tw)
{
    c64 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = V64_AT(base + j * L);
    if (twi != 0) {
#pragma unroll
        for (int k = 1; k < R; ++k) a[k] = mul_conj(a[k], tw[twi * k]);
    }
    bfly<R, true>(a);
#pragma unroll
    for (int j = 0; j < R; ++j) V64_AT(base + j * L) = a[j];
}

// the innermost stage (L = 1, no twiddles) of both directions around the threshold, in registers
template <int R>
__device__ __forceinline__ void stage_mid(c64* col, int W, int base, int mode, int op, c64 tau, StatAcc& st, bool in_range)
{
    c64 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = V64_AT(base + j);
    if (mode != Z_INV) {
        bfly<R, false>(a);
        if (mode == Z_STATS) {
            if (in_range) {
#pragma unroll
                for (int j = 0; j < R; ++j) st.add(a[j]);
            }
            return;
        }
        if (op >= 0) {
#pragma unroll
            for (int j = 0; j < R; ++j) a[j] = shrink64(a[j], tau, op);
        }
    }
    if (mode != Z_FWD) bfly<R, true>(a);
#pragma unroll
    for (int j = 0; j < R; ++j) V64_AT(base + j) = a[j];
}

#define V64_RADIX_SWITCH(r, CALL)      \
    switch (r) {                       \
        case 1: { constexpr int R = 1; CALL; } break; \
        case 2: { constexpr int R = 2; CALL; } break; \
        case 3: { constexpr int R = 3; CALL; } break; \
        case 4: { constexpr int R = 4; CALL; } break; \
        case 5: { constexpr int R = 5; CALL; } break; \
        default: { constexpr int R = 7; CALL; } break; \
    }

__global__ __launch_bounds__(V64_THREADS) void vol64_z_kernel(const Z64Args a)
{
    extern __shared__ c64 tile[];   // [n0][W], then the n0 roots; Z_STATS reuses the tile for its reduction (vol64::lds_bytes)
    const int W = a.width, n0 = a.n0;
    c64* const twl = tile + (size_t)n0 * W;
    // a wavefront covers 64 / W whole tile rows: with 16-B elements a 128-bit access of 64 lanes is then one contiguous 1-KiB run wherever the rows of a
    // stage are neighbours, and the 16-lane groups the LDS serves it in fall on distinct 16-B slots.  With W = 8 two rows share the 256 B the LDS serves per
    // clock and the innermost stages of radix 4 and 2 (row stride 4 or 2) read two-way conflicted; a row swizzle that removes the conflict left the pass's
    // time unchanged, so the tile stays linear
    const int w = threadIdx.x % W, r0 = threadIdx.x / W, rows = V64_THREADS / W;
    const size_t pos = (size_t)blockIdx.x * W + w;
    const bool in_range = pos < a.plane;
    c64* const col = tile + w;

    // Z_INV takes the spectrum in natural order: coefficient k goes to its digit-reversed position
    for (int p = r0; p < n0; p += rows) {
        const int z = a.mode == Z_INV ? vx::coef_of_pos(n0, a.nstage, a.radix, p) : p;
        V64_AT(p) = in_range ? a.work[(size_t)z * a.plane + pos] : c64{0.0, 0.0};
    }
    for (int i = threadIdx.x; i < n0; i += V64_THREADS) twl[i] = a.tw[i];
    __syncthreads();

    const int last = a.nstage - 1;
    if (a.mode != Z_INV) {
        int M = n0;
        for (int s = 0; s < last; ++s) {
            const int r = a.radix[s], L = M / r, step = n0 / M;
            for (int b = r0; b < n0 / r; b += rows) {
                const int blk = b / L, np = b - blk * L;
                V64_RADIX_SWITCH(r, stage_fwd<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
            M = L;
        }
    }
    StatAcc st;
    {
        const int r = a.radix[last];
        for (int b = r0; b < n0 / r; b += rows) {
            V64_RADIX_SWITCH(r, stage_mid<R>(col, W, b * r, a.mode, a.op, a.tau, st, in_range));
        }
        __syncthreads();
    }
    if (a.mode == Z_STATS) {   // (every thread is past its last read of the tile)
        double* const sh = reinterpret_cast<double*>(tile);
        double* me = sh + threadIdx.x * V64_STAT;
        me[0] = st.lr; me[1] = st.li; me[2] = st.mx; me[3] = st.mn; me[4] = st.sq;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int t = 1; t < V64_THREADS; ++t) {
                const double* o = sh + t * V64_STAT;
                if (o[0] > st.lr || (o[0] == st.lr && o[1] > st.li)) { st.lr = o[0]; st.li = o[1]; }
                st.mx = fmax(st.mx, o[2]);
                st.mn = fmin(st.mn, o[3]);
                st.sq += o[4];
            }
            double* o = a.partial + (size_t)blockIdx.x * V64_STAT;
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
                V64_RADIX_SWITCH(r, stage_inv<R>(col, W, blk * M + np, L, step * np, twl));
            }
            __syncthreads();
        }
    }
    // Z_FWD hands the spectrum back in natural order
    if (in_range) {
        for (int p = r0; p < n0; p += rows) {
            const int z = a.mode == Z_FWD ? vx::coef_of_pos(n0, a.nstage, a.radix, p) : p;
            const c64 v = V64_AT(p);
            a.work[(size_t)z * a.plane + pos] = a.mode == Z_FWD ? v : v * a.scale;
        }
    }
}

__device__ __forceinline__ double vol64_block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = V64_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// update64_kernel (p3d_f64.hip) for a volume (grid: V64_FOLD_X x n0): mode 0 -- w = x or its APOCS mix, partial sums of |x| and the count of non-zero
// samples; mode 1 -- xn = w (1 - alpha m) + alpha x, partial sums of |xn|, optional out = xn, w = xn or its APOCS mix.  mask_stride: plane for a mask per
// slice, 0 for one shared mask.  dtype (of x and out): P3D_C128 / P3D_F64 / P3D_C64 / P3D_F32; the arithmetic is double either way.
__global__ __launch_bounds__(V64_THREADS) void vol64_update_kernel(c64* w, const void* x, int dtype, const double* mask, size_t mask_stride, void* out, double* part,
                                                                   double* part_nz, int mode, int adaptive, int write_out, double alpha, size_t plane)
{
    __shared__ double sh[V64_THREADS];
    const size_t z = blockIdx.y;
    double acc = 0.0, nz = 0.0;
    for (size_t i = (size_t)blockIdx.x * V64_THREADS + threadIdx.x; i < plane; i += (size_t)gridDim.x * V64_THREADS) {
        const size_t g = z * plane + i;
        c64 xo;
        if (dtype == P3D_C128) xo = reinterpret_cast<const c64*>(x)[g];
        else if (dtype == P3D_F64) xo = c64{reinterpret_cast<const double*>(x)[g], 0.0};
        else if (dtype == P3D_C64) { const float2 t = reinterpret_cast<const float2*>(x)[g]; xo = c64{(double)t.x, (double)t.y}; }
        else xo = c64{(double)reinterpret_cast<const float*>(x)[g], 0.0};
        const double m = mask ? mask[z * mask_stride + i] : 0.0;
        const double wgt = 1.0 - alpha * m;
        c64 xn;
        if (mode == 0) {
            xn = xo;
            nz += (xo.x != 0.0 || xo.y != 0.0) ? 1.0 : 0.0;
        } else {
            xn = w[g] * wgt + xo * alpha;
            if (write_out) {
                if (dtype == P3D_C128) reinterpret_cast<c64*>(out)[g] = xn;
                else if (dtype == P3D_F64) reinterpret_cast<double*>(out)[g] = xn.x;
                else if (dtype == P3D_C64) reinterpret_cast<float2*>(out)[g] = float2{(float)xn.x, (float)xn.y};
                else reinterpret_cast<float*>(out)[g] = (float)xn.x;
            }
        }
        acc += hypot(xn.x, xn.y);
        if (adaptive) {   // POCS.py:574-575
            const c64 tmp = xo * alpha + xn * wgt;
            w[g] = tmp + (xo - xn * m) * (1.0 - alpha);
        } else {
            w[g] = xn;
        }
    }
    const size_t b = z * gridDim.x + blockIdx.x;
    const double tot = vol64_block_sum(acc, sh);
    if (threadIdx.x == 0) part[b] = tot;
    if (mode == 0) {
        __syncthreads();
        const double cnt = vol64_block_sum(nz, sh);
        if (threadIdx.x == 0) part_nz[b] = cnt;
    }
}

// one workgroup: dst[0] = the n partial sums added in a fixed order (and dst_nz[0] those of part_nz, where given)
__global__ __launch_bounds__(V64_THREADS) void vol64_fold_kernel(const double* part, const double* part_nz, size_t n, double* dst, double* dst_nz)
{
    __shared__ double sh[V64_THREADS];
    double acc = 0.0, nz = 0.0;
    for (size_t i = threadIdx.x; i < n; i += V64_THREADS) {
        acc += part[i];
        if (part_nz) nz += part_nz[i];
    }
    const double tot = vol64_block_sum(acc, sh);
    if (threadIdx.x == 0) dst[0] = tot;
    if (part_nz) {
        __syncthreads();
        const double cnt = vol64_block_sum(nz, sh);
        if (threadIdx.x == 0) dst_nz[0] = cnt;
    }
}

}  // namespace

struct p3d_vol64_plan {
    int device = 0, n0 = 0, n1 = 0, n2 = 0;
    p3d_plan64* plan = nullptr;   // the 2-D line passes of an (n1, n2) slice
    bool own_plan = false;
    int max_slices = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    c64* work = nullptr;        // [n0][n1][n2]
    c64* tw = nullptr;          // [n0]
    double* part = nullptr;     // [2][n0 * V64_FOLD_X]: partial sums of |x|, non-zero counts
    double* sums = nullptr;     // device [niter + 2]: sum |x_k|, k = 0 .. niter; the non-zero count of x behind them
    size_t sums_cap = 0;
    double* zpart = nullptr;    // [z workgroups][V64_STAT]
    double* mask = nullptr;     // staging of a host mask
    size_t mask_cap = 0;
    void* st_x = nullptr;       // staging of a host volume / of a result that may not go straight to `out`
    void* st_out = nullptr;
    size_t st_x_cap = 0, st_out_cap = 0;   // bytes
    Z64Args z{};
    double prof_z_ms = 0.0;     // P3D_FLAG_PROFILE: mean device time of the axis-0 pass in the last run, and its launches
    int prof_z_n = 0;

    size_t plane() const { return (size_t)n1 * n2; }
    size_t elems() const { return (size_t)n0 * plane(); }
    int zblocks() const { return (int)((plane() + z.width - 1) / z.width); }
    size_t nparts() const { return (size_t)n0 * V64_FOLD_X; }
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

bool known_dtype(int dtype) { return dtype == P3D_C128 || dtype == P3D_F64 || dtype == P3D_C64 || dtype == P3D_F32; }

int vol_check(p3d_vol64_plan* v)
{
    if (!v) return fail(P3D_ERR_INVALID, "NULL volume plan");
    P3D_TRY(hipSetDevice(v->device));
    return P3D_OK;
}

// fft2 / ifft2 of every slice of the work buffer, max_slices at a time
int vol_fft2(p3d_vol64_plan* v, bool inverse)
{
    for (int lo = 0; lo < v->n0; lo += v->max_slices) {
        const int n = v->n0 - lo < v->max_slices ? v->n0 - lo : v->max_slices;
        if (int rc = plan64_fft2(v->plan, v->work + (size_t)lo * v->plane(), n, inverse, nullptr, 1)) return rc;
    }
    return P3D_OK;
}

int vol_zpass(p3d_vol64_plan* v, int mode, int op, c64 tau)
{
    Z64Args a = v->z;
    a.mode = mode;
    a.op = op;
    a.tau = tau;
    const size_t lds = vx::lds_bytes(v->n0, a.width);
    vol64_z_kernel<<<v->zblocks(), V64_THREADS, lds, v->stream>>>(a);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int vol_update(p3d_vol64_plan* v, const void* x, int dtype, const double* mask, bool per_slice, void* out, int mode, int adaptive, int write_out, double alpha, double* dst)
{
    double* const nzp = mode == 0 ? v->part + v->nparts() : nullptr;
    vol64_update_kernel<<<dim3(V64_FOLD_X, v->n0), V64_THREADS, 0, v->stream>>>(v->work, x, dtype, mask, per_slice ? v->plane() : 0, out, v->part, nzp, mode, adaptive,
                                                                                 write_out, alpha, v->plane());
    vol64_fold_kernel<<<1, V64_THREADS, 0, v->stream>>>(v->part, nzp, v->nparts(), dst, mode == 0 ? dst + 1 : nullptr);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

// `src` (host or device, complex128) into the work buffer
int vol_load_c128(p3d_vol64_plan* v, const void* src)
{
    if (src != v->work) P3D_TRY(hipMemcpyAsync(v->work, src, sizeof(c64) * v->elems(), hipMemcpyDefault, v->stream));
    return P3D_OK;
}

int vol_fft3(p3d_vol64_plan* v, const void* in, void* out, int inverse)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!in || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if ((rc = vol_load_c128(v, in))) return rc;
    if (!inverse) {
        if ((rc = vol_fft2(v, false)) || (rc = vol_zpass(v, Z_FWD, -1, c64{0.0, 0.0}))) return rc;
    } else {
        if ((rc = vol_zpass(v, Z_INV, -1, c64{0.0, 0.0})) || (rc = vol_fft2(v, true))) return rc;
    }
    if (out != v->work) P3D_TRY(hipMemcpyAsync(out, v->work, sizeof(c64) * v->elems(), hipMemcpyDefault, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int vol_stats(p3d_vol64_plan* v, const void* x, int dtype, double* stats)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!x || !stats) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (!known_dtype(dtype)) return fail(P3D_ERR_UNSUPPORTED, "volume dtype %d: complex128, float64, complex64 and float32 only", dtype);
    const void* xd = x;
    if (!on_device(v->device, x)) {
        const size_t bytes = elem_bytes(dtype) * v->elems();
        if ((rc = grow_bytes(v->st_x, v->st_x_cap, bytes))) return rc;
        P3D_TRY(hipMemcpyAsync(v->st_x, x, bytes, hipMemcpyDefault, v->stream));
        xd = v->st_x;
    }
    if ((rc = vol_update(v, xd, dtype, nullptr, false, nullptr, 0, 0, 0, 0.0, v->sums))) return rc;   // work = x as complex128
    if ((rc = vol_fft2(v, false)) || (rc = vol_zpass(v, Z_STATS, -1, c64{0.0, 0.0}))) return rc;
    const int nb = v->zblocks();
    std::vector<double> part((size_t)nb * V64_STAT);
    P3D_TRY(hipMemcpyAsync(part.data(), v->zpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    double lr = -INFINITY, li = -INFINITY, mx = 0.0, mn = INFINITY, sq = 0.0;
    for (int b = 0; b < nb; ++b) {   // the workgroups' records in their order
        const double* q = &part[(size_t)b * V64_STAT];
        if (q[0] > lr || (q[0] == lr && q[1] > li)) { lr = q[0]; li = q[1]; }
        mx = std::fmax(mx, q[2]);
        mn = std::fmin(mn, q[3]);
        sq += q[4];
    }
    stats[0] = lr; stats[1] = li; stats[2] = mx; stats[3] = mn; stats[4] = sq; stats[5] = 0.0;
    return P3D_OK;
}

int vol_run(p3d_vol64_plan* v, const void* x, int dtype, const double* mask, const double* tau, const p3d_pocs_params* prm, void* out, int32_t* niter_done,
            double* sums, double* elapsed_ms)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!x || !mask || !tau || !prm || !out) return fail(P3D_ERR_INVALID, "NULL argument");
    if (!known_dtype(dtype)) return fail(P3D_ERR_UNSUPPORTED, "volume dtype %d: complex128, float64, complex64 and float32 only", dtype);
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
    const double alpha = prm->alpha;
    const size_t bytes = elem_bytes(dtype) * v->elems();

    // the volume, the mask and the result where the kernels can reach them
    const void* xd = x;
    if (!on_device(v->device, x)) {
        if ((rc = grow_bytes(v->st_x, v->st_x_cap, bytes))) return rc;
        P3D_TRY(hipMemcpyAsync(v->st_x, x, bytes, hipMemcpyDefault, v->stream));
        xd = v->st_x;
    }
    const double* md = mask;
    if (!on_device(v->device, mask)) {
        const size_t nm = per_slice ? v->elems() : v->plane();
        if ((rc = grow(v->mask, v->mask_cap, nm))) return rc;
        P3D_TRY(hipMemcpyAsync(v->mask, mask, sizeof(double) * nm, hipMemcpyDefault, v->stream));
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
            const c64 t{tau[2 * k], tau[2 * k + 1]};
            if ((rc = vol_fft2(v, false)) || (profile && (rc = prof.mark(v->stream))) || (rc = vol_zpass(v, Z_FUSED, op, t)) || (profile && (rc = prof.mark(v->stream))) ||
                (rc = vol_fft2(v, true)))
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

int p3d_vol64_shape_supported(int n0, int n1, int n2)
{
    int radix[vx::MAX_STAGES];
    return (vx::factor(n0, radix) > 0 && plan64_shape_ok(n1, n2)) ? 1 : 0;
}

int p3d_vol64_plan_destroy(p3d_vol64_plan* v)
{
    if (!v) return P3D_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void* q : {(void*)v->work, (void*)v->tw, (void*)v->part, (void*)v->sums, (void*)v->zpart, (void*)v->mask, v->st_x, v->st_out})
        if (q) (void)hipFree(q);
    if (v->ev0) (void)hipEventDestroy(v->ev0);
    if (v->ev1) (void)hipEventDestroy(v->ev1);
    if (v->own_plan && v->plan) (void)p3d_plan64_destroy(v->plan);
    delete v;
    return P3D_OK;
}

int p3d_vol64_plan_create(p3d_vol64_plan** out, int device, int n0, int n1, int n2, p3d_plan64* plan)
{
    if (!out) return fail(P3D_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int radix[vx::MAX_STAGES];
    const int nstage = vx::factor(n0, radix);
    if (nstage < 0)
        return fail(P3D_ERR_UNSUPPORTED, "n0 = %d: the axis-0 transform of a volume takes 7-smooth lengths from 1 to %d", n0, vx::MAX_N0);
    if (!plan64_shape_ok(n1, n2)) return fail(P3D_ERR_UNSUPPORTED, "slice shape %d x %d is not covered by the double-precision passes", n1, n2);
    if (int rc = use_device(device)) return rc;
    p3d_vol64_plan* v = new p3d_vol64_plan;
    v->device = device; v->n0 = n0; v->n1 = n1; v->n2 = n2;
    int rc = P3D_OK;
    auto bail = [&](int code) { (void)p3d_vol64_plan_destroy(v); return code; };
    if (plan) {
        if (plan->device != device || plan->nil != n1 || plan->nxl != n2)
            return bail(fail(P3D_ERR_INVALID, "the plan handed over is for %d x %d slices on device %d, the volume needs %d x %d on device %d", plan->nil, plan->nxl,
                             plan->device, n1, n2, device));
        v->plan = plan;
        v->max_slices = plan->max_slices;
    } else {
        const size_t slice_bytes = sizeof(c64) * v->plane();
        size_t cap = ((size_t)256 << 20) / slice_bytes;   // slices per call of the line passes: about 256 MiB at most
        if (cap < 1) cap = 1;
        v->max_slices = (size_t)n0 < cap ? n0 : (int)cap;
        if ((rc = plan64_create_bare(&v->plan, device, n1, n2, v->max_slices))) return bail(rc);
        v->own_plan = true;
    }
    v->stream = plan64_stream(v->plan);
    auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? P3D_OK : fail(P3D_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
    Z64Args& z = v->z;
    z.plane = v->plane();
    z.n0 = n0;
    z.width = vx::width(n0);
    z.nstage = nstage;
    for (int s = 0; s < nstage; ++s) z.radix[s] = radix[s];
    z.scale = 1.0 / (double)n0;
    std::vector<c64> tw(n0);
    for (int k = 0; k < n0; ++k) {
        const long double ang = -6.283185307179586476925286766559005768L * (long double)k / (long double)n0;
        tw[k] = c64{(double)cosl(ang), (double)sinl(ang)};
    }
    if ((rc = hip(hipEventCreate(&v->ev0), "hipEventCreate")) || (rc = hip(hipEventCreate(&v->ev1), "hipEventCreate"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->work, sizeof(c64) * v->elems()), "hipMalloc (volume work buffer)"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->tw, sizeof(c64) * (size_t)(n0 < 2 ? 2 : n0)), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMemcpy(v->tw, tw.data(), sizeof(c64) * n0, hipMemcpyHostToDevice), "hipMemcpy"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->part, sizeof(double) * 2 * v->nparts()), "hipMalloc"))) return bail(rc);
    if ((rc = hip(hipMalloc((void**)&v->zpart, sizeof(double) * V64_STAT * (size_t)v->zblocks()), "hipMalloc"))) return bail(rc);
    if ((rc = grow(v->sums, v->sums_cap, (size_t)64))) return bail(rc);
    z.work = v->work;
    z.tw = v->tw;
    z.partial = v->zpart;
    // the largest tile of any plan (1024 x 8 points and 1024 roots, 144 KiB): the attribute belongs to the kernel, not to the plan
    if ((rc = hip(hipFuncSetAttribute(reinterpret_cast<const void*>(vol64_z_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vx::lds_bytes(vx::MAX_N0, 8)),
                  "hipFuncSetAttribute")))
        return bail(rc);
    *out = v;
    return P3D_OK;
}

int p3d_vol64_fft3_c128_dev(p3d_vol64_plan* v, const void* in_dev, void* out_dev, int inverse) { return vol_fft3(v, in_dev, out_dev, inverse); }
int p3d_vol64_fft3_c128(p3d_vol64_plan* v, const void* in_host, void* out_host, int inverse) { return vol_fft3(v, in_host, out_host, inverse); }

int p3d_vol64_shrink_c128(p3d_vol64_plan* v, const void* in_host, const double* tau, int thresh_op, void* out_host)
{
    int rc = vol_check(v);
    if (rc) return rc;
    if (!in_host || !out_host || !tau) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (thresh_op < P3D_OP_HARD || thresh_op > P3D_OP_GARROTE) return fail(P3D_ERR_UNSUPPORTED, "thresh_op %d is not implemented", thresh_op);
    if ((rc = vol_load_c128(v, in_host)) || (rc = vol_fft2(v, false))) return rc;
    if ((rc = vol_zpass(v, Z_FWD, thresh_op, c64{tau[0], tau[1]}))) return rc;
    P3D_TRY(hipMemcpyAsync(out_host, v->work, sizeof(c64) * v->elems(), hipMemcpyDefault, v->stream));
    P3D_TRY(hipStreamSynchronize(v->stream));
    return P3D_OK;
}

int p3d_vol64_last_profile(p3d_vol64_plan* v, double* zpass_ms, int* zpass_launches)
{
    if (!v || !zpass_ms || !zpass_launches) return fail(P3D_ERR_INVALID, "NULL argument");
    *zpass_ms = v->prof_z_ms;
    *zpass_launches = v->prof_z_n;
    return P3D_OK;
}

int p3d_vol64_stats_dev(p3d_vol64_plan* v, const void* x_dev, int dtype, double* stats_host) { return vol_stats(v, x_dev, dtype, stats_host); }
int p3d_vol64_stats(p3d_vol64_plan* v, const void* x_host, int dtype, double* stats_host) { return vol_stats(v, x_host, dtype, stats_host); }

int p3d_vol64_run_dev(p3d_vol64_plan* v, const void* x_dev, int dtype, const double* mask_dev, const double* tau, const p3d_pocs_params* params, void* out_dev,
                      int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vol_run(v, x_dev, dtype, mask_dev, tau, params, out_dev, niter_done, sums, elapsed_ms);
}
int p3d_vol64_run(p3d_vol64_plan* v, const void* x_host, int dtype, const double* mask_host, const double* tau, const p3d_pocs_params* params, void* out_host,
                  int32_t* niter_done, double* sums, double* elapsed_ms)
{
    return vol_run(v, x_host, dtype, mask_host, tau, params, out_host, niter_done, sums, elapsed_ms);
}

}  // extern "C"
