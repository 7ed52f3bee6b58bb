// p3d_patch.hip -- windowed POCS: patch gather, packed mask windows, tapered overlap-add blend, and the C entry points of p3d_patch_plan.
//
// Production POCS interpolation runs in overlapping spatial windows (events are only locally planar): a slice of nil x nxl bins is cut into
// n_il x n_xl windows of w_il x w_xl bins, every window of every slice is an independent POCS job (own statistics, schedule, early exit), and the
// results are blended with a separable taper.  Here:
//
//     cube [n][nil][nxl]  --patch_gather_kernel-->  patch cube [n npatch][w_il][w_xl]                     (8 + 8 B per patch point, complex64)
//     mask                --patch_pack_kernel-->    packed words of the single-kernel loop, one mask per window (resident_kernel<.., op | RESIDENT_MASK_PER_JOB>)
//                                                   (DCT windows: resident_dct_kernel of p3d_patch_dct.hip on the same words, p3d_patch_dct_run_dev below)
//     patch results       --patch_blend_kernel-->   out [n][nil][nxl] = sum_k W_k y_k / sum_k W_k            (8 B per covering window + 8 B per point)
//
// All three are bound by memory: one element per thread, consecutive threads on consecutive xline positions (coalesced 8-byte / 4-byte accesses; window starts
// are arbitrary, so nothing wider is aligned).  No atomics but the flag: the blend takes the covering windows in ascending order, the result is deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "p3d_fft.hpp"
#include "p3d_host.hpp"
#include "p3d_patch.hpp"
#include "p3d_resident_job.hpp"

namespace p3d {

// one thread per element of the patch cube: blockIdx.x = job, blockIdx.y * 256 + threadIdx.x = position in the window
template <class T, bool CHECK>
__global__ __launch_bounds__(256) void patch_gather_kernel(const PatchGeom g, const T* __restrict__ src, int src_slices, T* __restrict__ patches, int* nonbinary)
{
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int per = g.w_il * g.w_xl;
    if (e >= per) return;
    const size_t job = blockIdx.x;
    const int npatch = g.n_il * g.n_xl;
    const int p = (int)(job % npatch);
    const size_t s = (job / npatch) % (size_t)src_slices;
    const int r = e / g.w_xl, c = e - r * g.w_xl;
    const int i = g.starts_il[p / g.n_xl] + r, j = g.starts_xl[p % g.n_xl] + c;
    const T v = src[(s * g.nil + i) * g.nxl + j];
    patches[job * per + e] = v;
    if constexpr (CHECK) {
        if (nonbinary && v != 0.0f && v != 1.0f) atomicOr(nonbinary, 1);
    }
}

// one thread per packed word: blockIdx.x = mask window, blockIdx.y * 256 + threadIdx.x = (row, thread of the row) as resident_kernel reads it
__global__ __launch_bounds__(256) void patch_pack_kernel(const PatchGeom g, const float* __restrict__ mask, int mask_slices, uint16_t* __restrict__ bits, int* nonbinary)
{
    const int tpl = g.w_xl / 16;
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= g.w_il * tpl) return;
    const size_t job = blockIdx.x;
    const int npatch = g.n_il * g.n_xl;
    const int p = (int)(job % npatch);
    const size_t s = (job / npatch) % (size_t)mask_slices;
    const int r = e / tpl, tl = e - r * tpl;
    const float* row = mask + (s * g.nil + g.starts_il[p / g.n_xl] + r) * g.nxl + g.starts_xl[p % g.n_xl];
    unsigned w = 0;
    bool odd = false;
    for (int q = 0; q < 16; ++q) {
        const float m = row[tl + tpl * q];
        if (m == 1.0f) w |= 1u << q;
        else if (m != 0.0f) odd = true;
    }
    bits[job * ((size_t)g.w_il * tpl) + e] = (uint16_t)w;
    if (odd) atomicOr(nonbinary, 1);
}

// one thread per output point: blockIdx.z = slice, blockIdx.y = iline, blockIdx.x * 256 + threadIdx.x = xline
template <class T>
__global__ __launch_bounds__(256) void patch_blend_kernel(const PatchGeom g, const PatchBlend b, const T* __restrict__ patches, T* __restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.nxl) return;
    const int i = blockIdx.y;
    const size_t s = blockIdx.z;
    const int npatch = g.n_il * g.n_xl;
    const size_t per = (size_t)g.w_il * g.w_xl;
    const int a0 = b.first_il[i], a1 = b.last_il[i], b0 = b.first_xl[j], b1 = b.last_xl[j];
    T num{};
    float den = 0.f;
    for (int a = a0; a <= a1; ++a) {
        const int r = i - g.starts_il[a];
        const float ti = b.taper_il[r];
        for (int bb = b0; bb <= b1; ++bb) {
            const size_t job = s * npatch + (size_t)a * g.n_xl + bb;
            if (b.state[job] < 0) continue;
            const int c = j - g.starts_xl[bb];
            const float w = ti * b.taper_xl[c];
            const T y = patches[job * per + (size_t)r * g.w_xl + c];
            if constexpr (sizeof(T) == 8) {
                num.x = num.x + w * y.x;
                num.y = num.y + w * y.y;
            } else {
                num = num + w * y;
            }
            den += w;
        }
    }
    T res{};
    if (den > 0.f) {
        if constexpr (sizeof(T) == 8) {
            res.x = num.x / den;
            res.y = num.y / den;
        } else {
            res = num / den;
        }
    }
    out[(s * g.nil + i) * g.nxl + j] = res;
}

// The single-kernel loop of p3d_resident.hip with the mask words of job j read at bits + (j % mask_period) * bits_stride: the same kernel template
// (p3d_resident_job.hpp) instantiated with RESIDENT_MASK_PER_JOB, so the same transforms, operation order and reduction order -- window results, sums and
// iteration counts are those the shared-mask instantiation gives for the same slice and mask.
template <int N1, int N2>
static hipError_t launch_patch_shape(const ResidentArgs& a, hipStream_t st)
{
    constexpr size_t lds = resident_lds_bytes<N1, N2>();
    constexpr int T = N1 * N2 / 16;
#define P3D_RES(OP)                                                                                                         \
    do {                                                                                                                    \
        if (lds > 64 * 1024) {                                                                                              \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(resident_kernel<N1, N2, OP | RESIDENT_MASK_PER_JOB>),  \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                 \
            if (e != hipSuccess) return e;                                                                                  \
        }                                                                                                                   \
        resident_kernel<N1, N2, OP | RESIDENT_MASK_PER_JOB><<<a.nslices, T, lds, st>>>(a);                                  \
    } while (0)
    switch (a.op) {
        case 0: P3D_RES(0); break;
        case 1: P3D_RES(1); break;
        case 2: P3D_RES(2); break;
        default: return hipErrorInvalidValue;
    }
#undef P3D_RES
    return hipGetLastError();
}

// the shapes the single-kernel path is routed to (at most 8192 points: no 128 x 128)
hipError_t resident_patch_launch(int nil, int nxl, const ResidentArgs& a, hipStream_t st)
{
    if (a.mask_period < 1 || !a.bits) return hipErrorInvalidValue;
#define P3D_SHAPE(A, B) if (nil == A && nxl == B) return launch_patch_shape<A, B>(a, st)
    P3D_SHAPE(32, 32); P3D_SHAPE(32, 64); P3D_SHAPE(32, 128);
    P3D_SHAPE(64, 32); P3D_SHAPE(64, 64); P3D_SHAPE(64, 128);
    P3D_SHAPE(128, 32); P3D_SHAPE(128, 64);
#undef P3D_SHAPE
    return hipErrorNotSupported;
}

static bool grid_ok(size_t njobs, int per) { return njobs >= 1 && njobs <= 0x7fffffffu && per >= 1 && (per + 255) / 256 <= 65535; }

hipError_t patch_launch_gather(const PatchGeom& g, const void* src, int src_slices, void* patches, size_t njobs, int elem_bytes, int* nonbinary, hipStream_t st)
{
    const int per = g.w_il * g.w_xl;
    if (!grid_ok(njobs, per) || src_slices < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)njobs, (per + 255) / 256);
    if (elem_bytes == 8) patch_gather_kernel<c32, false><<<grid, 256, 0, st>>>(g, static_cast<const c32*>(src), src_slices, static_cast<c32*>(patches), nullptr);
    else if (nonbinary) patch_gather_kernel<float, true><<<grid, 256, 0, st>>>(g, static_cast<const float*>(src), src_slices, static_cast<float*>(patches), nonbinary);
    else patch_gather_kernel<float, false><<<grid, 256, 0, st>>>(g, static_cast<const float*>(src), src_slices, static_cast<float*>(patches), nullptr);
    return hipGetLastError();
}

hipError_t patch_launch_pack(const PatchGeom& g, const float* mask, int mask_slices, uint16_t* bits, size_t nmasks, int* nonbinary, hipStream_t st)
{
    if (g.w_xl % 16 != 0 || !nonbinary || mask_slices < 1) return hipErrorInvalidValue;
    const int per = g.w_il * (g.w_xl / 16);
    if (!grid_ok(nmasks, per)) return hipErrorInvalidValue;
    patch_pack_kernel<<<dim3((unsigned)nmasks, (per + 255) / 256), 256, 0, st>>>(g, mask, mask_slices, bits, nonbinary);
    return hipGetLastError();
}

hipError_t patch_launch_blend(const PatchGeom& g, const PatchBlend& b, const void* patches, void* out, int nslices, int dtype, hipStream_t st)
{
    if (nslices < 1 || nslices > 65535 || g.nil > 65535) return hipErrorInvalidValue;
    const dim3 grid((g.nxl + 255) / 256, g.nil, nslices);
    if (dtype == P3D_C64) patch_blend_kernel<c32><<<grid, 256, 0, st>>>(g, b, static_cast<const c32*>(patches), static_cast<c32*>(out));
    else patch_blend_kernel<float><<<grid, 256, 0, st>>>(g, b, static_cast<const float*>(patches), static_cast<float*>(out));
    return hipGetLastError();
}

}  // namespace p3d

using namespace p3d;

// The geometry of one windowed job family on the device, over a (w_il, w_xl) plan the caller owns: start tables, tapers, the per-position window ranges of
// the blend, the packed mask windows and the per-job state.
struct p3d_patch_plan {
    p3d_plan* plan = nullptr;     // not owned
    int device = 0, max_slices = 0, max_jobs = 0;
    PatchGeom g{};
    PatchBlend b{};
    int* tables = nullptr;        // starts_il | starts_xl | first_il | last_il | first_xl | last_xl
    float* tapers = nullptr;      // taper_il | taper_xl
    uint16_t* bits = nullptr;     // [max_jobs][w_il][w_xl / 16], allocated by the first p3d_patch_mask_dev on a shape the single-kernel loop covers
    int* state = nullptr;         // [max_jobs]
    int* flag = nullptr;
    bool resident_shape = false;  // the plan's shape is one of the single-kernel loop's
    bool packed = false;          // bits hold the windows of the last p3d_patch_mask_dev ...
    int packed_period = 0;        // ... this many of them
    int nonbinary = 0;            // ... and that mask held values other than 0 and 1
};

static int check_axis(const char* what, const int32_t* starts, int n, int w, int extent, const float* taper)
{
    if (!starts || !taper || n < 1) return fail(P3D_ERR_INVALID, "%s: missing start table or taper", what);
    if (w < 1 || w > extent) return fail(P3D_ERR_INVALID, "%s: window %d outside 1..%d", what, w, extent);
    for (int k = 0; k < n; ++k) {
        if (starts[k] < 0 || starts[k] + w > extent) return fail(P3D_ERR_INVALID, "%s: window %d starts at %d, %d points do not fit %d", what, k, starts[k], w, extent);
        if (k > 0 && starts[k] <= starts[k - 1]) return fail(P3D_ERR_INVALID, "%s: window starts must increase (%d after %d)", what, starts[k], starts[k - 1]);
    }
    for (int k = 0; k < w; ++k)
        if (!(taper[k] > 0.0f) || !std::isfinite(taper[k])) return fail(P3D_ERR_INVALID, "%s: taper[%d] = %g is not positive", what, k, (double)taper[k]);
    return P3D_OK;
}

// first / last window covering every position of an axis (-1 / -2 where none: the blend's loop is then empty)
static void cover(const int32_t* starts, int n, int w, int extent, int* first, int* last)
{
    for (int i = 0; i < extent; ++i) {
        first[i] = -1;
        last[i] = -2;
        for (int k = 0; k < n; ++k)
            if (starts[k] <= i && i < starts[k] + w) {
                if (first[i] < 0) first[i] = k;
                last[i] = k;
            }
        if (first[i] < 0) first[i] = 0, last[i] = -1;
    }
}

extern "C" {

int p3d_patch_plan_create(p3d_patch_plan** out, p3d_plan* plan, int nil, int nxl, const int32_t* starts_il, int n_il, const int32_t* starts_xl, int n_xl,
                          const float* taper_il, const float* taper_xl, int max_slices)
{
    if (!out || !plan) return fail(P3D_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int device = 0, w_il = 0, w_xl = 0, plan_slices = 0, resident = 0;
    plan_describe(plan, &device, &w_il, &w_xl, &plan_slices, &resident);
    if (nil < 1 || nxl < 1 || nil > 65535 || max_slices < 1 || max_slices > 65535) return fail(P3D_ERR_INVALID, "slice %d x %d, %d slices: outside the blend's grid", nil, nxl, max_slices);
    int rc;
    if ((rc = check_axis("iline", starts_il, n_il, w_il, nil, taper_il)) || (rc = check_axis("xline", starts_xl, n_xl, w_xl, nxl, taper_xl))) return rc;
    const long long jobs = (long long)max_slices * n_il * n_xl;
    if (jobs > plan_slices) return fail(P3D_ERR_INVALID, "%d slices of %d x %d windows are %lld jobs, the plan holds %d", max_slices, n_il, n_xl, jobs, plan_slices);
    P3D_TRY(hipSetDevice(device));
    p3d_patch_plan* pp = new p3d_patch_plan;
    pp->plan = plan; pp->device = device; pp->max_slices = max_slices; pp->max_jobs = (int)jobs; pp->resident_shape = resident != 0;
    std::vector<int> tab((size_t)n_il + n_xl + 2 * ((size_t)nil + nxl));
    int* t = tab.data();
    for (int k = 0; k < n_il; ++k) t[k] = starts_il[k];
    for (int k = 0; k < n_xl; ++k) t[n_il + k] = starts_xl[k];
    int* cov = t + n_il + n_xl;
    cover(starts_il, n_il, w_il, nil, cov, cov + nil);
    cover(starts_xl, n_xl, w_xl, nxl, cov + 2 * (size_t)nil, cov + 2 * (size_t)nil + nxl);
    std::vector<float> tap((size_t)w_il + w_xl);
    for (int k = 0; k < w_il; ++k) tap[k] = taper_il[k];
    for (int k = 0; k < w_xl; ++k) tap[(size_t)w_il + k] = taper_xl[k];
    hipError_t e = hipMalloc((void**)&pp->tables, sizeof(int) * tab.size());
    if (e == hipSuccess) e = hipMalloc((void**)&pp->tapers, sizeof(float) * tap.size());
    if (e == hipSuccess) e = hipMalloc((void**)&pp->state, sizeof(int) * (size_t)jobs);
    if (e == hipSuccess) e = hipMalloc((void**)&pp->flag, sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(pp->tables, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pp->tapers, tap.data(), sizeof(float) * tap.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        p3d_patch_plan_destroy(pp);
        return fail(P3D_ERR_HIP, "allocating the tables of a patch plan failed: %s", hipGetErrorString(e));
    }
    pp->g = PatchGeom{nil, nxl, w_il, w_xl, n_il, n_xl, pp->tables, pp->tables + n_il};
    const int* c = pp->tables + n_il + n_xl;
    pp->b = PatchBlend{pp->tapers, pp->tapers + w_il, c, c + nil, c + 2 * (size_t)nil, c + 2 * (size_t)nil + nxl, pp->state};
    *out = pp;
    return P3D_OK;
}

int p3d_patch_plan_destroy(p3d_patch_plan* pp)
{
    if (!pp) return P3D_OK;
    (void)hipSetDevice(pp->device);
    for (void* q : {(void*)pp->tables, (void*)pp->tapers, (void*)pp->bits, (void*)pp->state, (void*)pp->flag})
        if (q) (void)hipFree(q);
    delete pp;
    return P3D_OK;
}

int p3d_patch_plan_info(p3d_patch_plan* pp, int* npatch, int* max_jobs, int* resident_shape)
{
    if (!pp) return fail(P3D_ERR_INVALID, "NULL plan");
    if (npatch) *npatch = pp->g.n_il * pp->g.n_xl;
    if (max_jobs) *max_jobs = pp->max_jobs;
    if (resident_shape) *resident_shape = pp->resident_shape ? 1 : 0;
    return P3D_OK;
}

static int check_slices(p3d_patch_plan* pp, int nslices)
{
    if (!pp) return fail(P3D_ERR_INVALID, "NULL plan");
    if (nslices < 1 || nslices > pp->max_slices) return fail(P3D_ERR_INVALID, "nslices = %d outside 1..max_slices (%d)", nslices, pp->max_slices);
    P3D_TRY(hipSetDevice(pp->device));
    return P3D_OK;
}

int p3d_patch_gather_dev(p3d_patch_plan* pp, const void* cube, int dtype, int nslices, void* patches)
{
    if (int rc = check_slices(pp, nslices)) return rc;
    if (!cube || !patches) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_INVALID, "unknown dtype %d", dtype);
    hipStream_t st = plan_stream(pp->plan);
    P3D_TRY(patch_launch_gather(pp->g, cube, nslices, patches, (size_t)nslices * pp->g.n_il * pp->g.n_xl, dtype == P3D_C64 ? 8 : 4, nullptr, st));
    P3D_TRY(hipStreamSynchronize(st));
    return P3D_OK;
}

int p3d_patch_mask_dev(p3d_patch_plan* pp, const float* mask, int mask_slices, int nslices, float* windows, int* nonbinary)
{
    if (int rc = check_slices(pp, nslices)) return rc;
    if (!mask) return fail(P3D_ERR_INVALID, "NULL mask");
    if (mask_slices != 1 && mask_slices != nslices) return fail(P3D_ERR_INVALID, "a mask of %d slices for %d slices (1: shared, nslices: one each)", mask_slices, nslices);
    hipStream_t st = plan_stream(pp->plan);
    const int npatch = pp->g.n_il * pp->g.n_xl;
    const size_t period = (size_t)mask_slices * npatch;
    P3D_TRY(hipMemsetAsync(pp->flag, 0, sizeof(int), st));
    pp->packed = false;
    if (pp->resident_shape) {
        if (!pp->bits) P3D_TRY(hipMalloc((void**)&pp->bits, sizeof(uint16_t) * (size_t)pp->max_jobs * pp->g.w_il * (pp->g.w_xl / 16)));
        P3D_TRY(patch_launch_pack(pp->g, mask, mask_slices, pp->bits, period, pp->flag, st));
    }
    if (windows) P3D_TRY(patch_launch_gather(pp->g, mask, mask_slices, windows, (size_t)nslices * npatch, 4, pp->flag, st));
    int odd = 0;
    if (pp->resident_shape || windows) P3D_TRY(hipMemcpyAsync(&odd, pp->flag, sizeof(int), hipMemcpyDeviceToHost, st));
    P3D_TRY(hipStreamSynchronize(st));
    pp->packed = pp->resident_shape;
    pp->packed_period = (int)period;
    pp->nonbinary = odd;
    if (nonbinary) *nonbinary = odd;
    return P3D_OK;
}

// the single-kernel loop takes a job when the window shape is one of its own, the masks of the last p3d_patch_mask_dev are binary, the operator is hard / soft /
// garrote on a given schedule, the version is not APOCS -- and P3D_NO_PATCH_RESIDENT is not set (read here, once per call)
static bool one_kernel(const p3d_patch_plan* pp, const p3d_pocs_params* prm)
{
    if (getenv("P3D_NO_PATCH_RESIDENT") != nullptr) return false;
    return pp->resident_shape && pp->packed && !pp->nonbinary && prm->thresh_op >= P3D_OP_HARD && prm->thresh_op <= P3D_OP_GARROTE &&
           (prm->version == P3D_VER_REGULAR || prm->version == P3D_VER_FAST);
}

int p3d_patch_route(p3d_patch_plan* pp, const p3d_pocs_params* params, int* single_kernel)
{
    if (!pp || !params || !single_kernel) return fail(P3D_ERR_INVALID, "NULL argument");
    *single_kernel = one_kernel(pp, params) ? 1 : 0;
    return P3D_OK;
}

int p3d_patch_run_dev(p3d_patch_plan* pp, const void* patches, int dtype, const double* tau, const uint8_t* active, const p3d_pocs_params* params, void* out,
                      int nslices, int32_t* niter_done, double* sums, double* elapsed_ms)
{
    if (int rc = check_slices(pp, nslices)) return rc;
    if (!params) return fail(P3D_ERR_INVALID, "NULL argument");
    if (!one_kernel(pp, params))
        return fail(P3D_ERR_UNSUPPORTED, "the single-kernel windowed loop does not cover this job (window shape, operator, version, non-binary masks, or P3D_NO_PATCH_RESIDENT): "
                                         "run the plan's own loop on the patch cube with P3D_FLAG_MASK_PER_SLICE");
    const int npatch = pp->g.n_il * pp->g.n_xl;
    if (pp->packed_period != npatch && pp->packed_period != nslices * npatch)
        return fail(P3D_ERR_INVALID, "the packed masks are those of another batch (%d windows, this one has %d per slice x %d slices)", pp->packed_period, npatch, nslices);
    return resident_run_jobs(pp->plan, patches, dtype, pp->bits, pp->packed_period, (size_t)pp->g.w_il * (pp->g.w_xl / 16), tau, active, params, out, nslices * npatch,
                             niter_done, sums, elapsed_ms);
}

// the DCT loop's route: the jobs of one_kernel() with a norm the factor tables have
static bool one_kernel_dct(const p3d_patch_plan* pp, const p3d_pocs_params* prm, int norm)
{
    return (norm == P3D_DCT_BACKWARD || norm == P3D_DCT_ORTHO) && one_kernel(pp, prm);
}

int p3d_patch_dct_route(p3d_patch_plan* pp, const p3d_pocs_params* params, int norm, int* single_kernel)
{
    if (!pp || !params || !single_kernel) return fail(P3D_ERR_INVALID, "NULL argument");
    *single_kernel = one_kernel_dct(pp, params, norm) ? 1 : 0;
    return P3D_OK;
}

int p3d_patch_dct_run_dev(p3d_patch_plan* pp, const void* patches, int dtype, const double* tau, const uint8_t* active, const p3d_pocs_params* params, int norm,
                          void* out, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms)
{
    if (int rc = check_slices(pp, nslices)) return rc;
    if (!params) return fail(P3D_ERR_INVALID, "NULL argument");
    if (!one_kernel_dct(pp, params, norm))
        return fail(P3D_ERR_UNSUPPORTED, "the single-kernel windowed DCT loop does not cover this job (window shape, operator, version, norm, non-binary masks, or "
                                         "P3D_NO_PATCH_RESIDENT): run p3d_pocs_dct_run_dev on the patch cube with P3D_FLAG_MASK_PER_SLICE");
    const int npatch = pp->g.n_il * pp->g.n_xl;
    if (pp->packed_period != npatch && pp->packed_period != nslices * npatch)
        return fail(P3D_ERR_INVALID, "the packed masks are those of another batch (%d windows, this one has %d per slice x %d slices)", pp->packed_period, npatch, nslices);
    return resident_dct_run_jobs(pp->plan, patches, dtype, pp->bits, pp->packed_period, (size_t)pp->g.w_il * (pp->g.w_xl / 16), tau, active, params, out,
                                 nslices * npatch, niter_done, sums, elapsed_ms, norm);
}

int p3d_patch_blend_dev(p3d_patch_plan* pp, const void* patches, int dtype, const uint8_t* active, void* out, int nslices)
{
    if (int rc = check_slices(pp, nslices)) return rc;
    if (!patches || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (dtype != P3D_C64 && dtype != P3D_F32) return fail(P3D_ERR_INVALID, "unknown dtype %d", dtype);
    hipStream_t st = plan_stream(pp->plan);
    const int njobs = nslices * pp->g.n_il * pp->g.n_xl;
    const std::vector<int> state = done_from_active(active, njobs);
    P3D_TRY(hipMemcpyAsync(pp->state, state.data(), sizeof(int) * njobs, hipMemcpyHostToDevice, st));
    P3D_TRY(patch_launch_blend(pp->g, pp->b, patches, out, nslices, dtype, st));
    P3D_TRY(hipStreamSynchronize(st));
    return P3D_OK;
}

}  // extern "C"
