// p3d_host.hpp -- the host-side plumbing every HIP unit of libp3d_hip.so repeats: the formatted error, the check of a HIP call,
// a device buffer that frees itself, the selection of the device and the frame the six POCS loops share around their passes (LoopFrame).
// Host code only; what one unit alone needs stays in that unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "p3d_internal.hpp"

namespace p3d {

// records the formatted message (cut to 511 characters) for p3d_last_error() and returns `code`: `return fail(P3D_ERR_INVALID, ...)`
inline int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_last_error(buf);
    return code;
}

// leaves the calling function with P3D_ERR_HIP and "<expr> failed: <what the runtime says>" unless the HIP call succeeds
#define P3D_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return p3d::fail(P3D_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// a device allocation freed on scope exit: hipMalloc(&buf.p, bytes)
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// makes `device` the calling thread's current device, after checking it against the visible ones
inline int use_device(int device)
{
    int ndev = 0;
    P3D_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(P3D_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    P3D_TRY(hipSetDevice(device));
    return P3D_OK;
}

// a grow-only device buffer of `cap` elements: untouched while cap >= n, otherwise freed and allocated anew for n elements (the contents
// are not kept).  A failed allocation leaves ptr == nullptr and cap == 0.
template <class T>
int grow(T*& ptr, size_t& cap, size_t n)
{
    if (cap >= n) return P3D_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    P3D_TRY(hipMalloc((void**)&ptr, sizeof(T) * n));
    cap = n;
    return P3D_OK;
}

// The mask of a job into a plan's own buffer, on the plan's stream (`mask` may be a host or a device pointer).  The buffer holds one slice
// until the first P3D_FLAG_MASK_PER_SLICE job, then max_slices slices; *stride is what the update kernels add per slice (0: shared mask).
template <class T>
int stage_mask(T*& buf, size_t& cap, const T* mask, size_t per, const p3d_pocs_params* prm, int nslices, int max_slices, hipStream_t stream, size_t* stride)
{
    const bool per_slice = (prm->flags & P3D_FLAG_MASK_PER_SLICE) != 0;
    if (int rc = grow(buf, cap, per * (per_slice ? (size_t)max_slices : 1))) return rc;
    P3D_TRY(hipMemcpyAsync(buf, mask, sizeof(T) * per * (per_slice ? (size_t)nslices : 1), hipMemcpyDefault, stream));
    *stride = per_slice ? per : 0;
    return P3D_OK;
}

// the per-slice state of a loop: 0 = running, -1 = switched off by the caller (`active`, NULL: every slice runs), k > 0 = converged at iteration k
inline std::vector<int> done_from_active(const uint8_t* active, int nslices)
{
    std::vector<int> done_h(nslices, 0);
    if (active)
        for (int s = 0; s < nslices; ++s) done_h[s] = active[s] ? 0 : -1;
    return done_h;
}

// ... and the iterations each slice made: none when switched off, all of them unless it converged
inline void niter_from_done(const int* done_h, int nslices, int niter, int32_t* niter_done)
{
    for (int s = 0; s < nslices; ++s) niter_done[s] = done_h[s] < 0 ? 0 : (done_h[s] > 0 ? done_h[s] : niter);
}

// np.percentile's position of percentage `perc` among per_slice sorted values: the two order statistics and the weight of the upper one
// (a NaN or negative percentage reads as 0, one above 100 as 100)
inline void percentile_rank(double perc, size_t per_slice, unsigned* lo, unsigned* hi, float* frac)
{
    double pos = perc / 100.0 * (double)(per_slice - 1);
    if (!(pos >= 0.0)) pos = 0.0;
    if (pos > (double)(per_slice - 1)) pos = (double)(per_slice - 1);
    const double fl = std::floor(pos);
    *lo = (unsigned)fl;
    *hi = (unsigned)std::fmin(fl + 1.0, (double)(per_slice - 1));
    *frac = (float)(pos - fl);
}

// ... with the weight in double, for the double-precision loop: NumPy's own (n - 1) q - floor((n - 1) q) (the float above costs about 1e-8)
inline void percentile_rank64(double perc, size_t per_slice, unsigned* lo, unsigned* hi, double* frac)
{
    double pos = (double)(per_slice - 1) * (perc / 100.0);
    if (!(pos >= 0.0)) pos = 0.0;
    if (pos > (double)(per_slice - 1)) pos = (double)(per_slice - 1);
    const double fl = std::floor(pos);
    *lo = (unsigned)fl;
    *hi = (unsigned)std::fmin(fl + 1.0, (double)(per_slice - 1));
    *frac = pos - fl;
}

// 16 / 8 / 4 bytes per sample of a P3D_C128 / P3D_F64, P3D_C64 / P3D_F32 cube; real cubes
inline size_t elem_bytes(int dtype) { return dtype == P3D_C128 ? 16 : (dtype == P3D_F64 || dtype == P3D_C64) ? 8 : 4; }
inline bool real_dtype(int dtype) { return dtype == P3D_F64 || dtype == P3D_F32; }

// a pointer into the memory of device `device` (the entry points of the optional transforms take host or device pointers)
inline bool on_device(int device, const void* ptr)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();   // ordinary host memory
        return false;
    }
    return at.type == hipMemoryTypeDevice && at.device == device;
}
template <class Plan>
bool on_plan_device(const Plan* p, const void* ptr) { return on_device(p->device, ptr); }

// x (host or device) -> cur_x: the caller's own device buffer where it passed one, the plan's staging buffer (filled on its stream) otherwise
template <class Plan>
int take_x(Plan* p, const void* x, size_t bytes)
{
    if (on_plan_device(p, x)) {
        p->cur_x = x;
    } else {
        P3D_TRY(hipMemcpyAsync(p->st_x, x, bytes, hipMemcpyDefault, p->stream));
        p->cur_x = p->st_x;
    }
    return P3D_OK;
}

// cur_out: the caller's `out` where it lies on the plan's device and does not overlap the observed cube (`bytes` each; the loops read x in every
// iteration), the staging buffer otherwise.  True when the result goes straight to `out`.
template <class Plan>
bool choose_out(Plan* p, const void* x, void* out, size_t bytes)
{
    const char* const xb = static_cast<const char*>(x);
    char* const ob = static_cast<char*>(out);
    const bool direct_out = on_plan_device(p, out) && (ob + bytes <= xb || xb + bytes <= ob);
    p->cur_out = direct_out ? out : p->st_out;
    return direct_out;
}

// The frame around the passes of a POCS loop, the same in all six: begin() uploads the per-slice state, clears the cost sums and starts the
// clock; enqueue_end() stops it and queues the downloads; collect() waits for the stream and hands niter_done / elapsed_ms to the caller.
// A loop puts whatever else must be downloaded (its result, its own counters) between enqueue_end() and collect(), or copies after collect().
struct LoopFrame {
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    int* done;          // device [nslices]
    double* sums;       // device [niter + 1][nslices]
    int nslices, niter;
    std::vector<int> done_h;

    template <class Plan>
    LoopFrame(Plan* p, const uint8_t* active, int nslices_, int niter_)
        : stream(p->stream), ev0(p->ev0), ev1(p->ev1), done(p->done), sums(p->sums), nslices(nslices_), niter(niter_), done_h(done_from_active(active, nslices_))
    {
    }
    size_t nsum() const { return (size_t)(niter + 1) * nslices; }
    bool any_off() const
    {
        for (int d : done_h)
            if (d != 0) return true;
        return false;
    }
    int begin()
    {
        P3D_TRY(hipMemcpyAsync(done, done_h.data(), sizeof(int) * nslices, hipMemcpyHostToDevice, stream));
        P3D_TRY(hipMemsetAsync(sums, 0, sizeof(double) * nsum(), stream));
        P3D_TRY(hipEventRecord(ev0, stream));
        return P3D_OK;
    }
    int enqueue_end(double* sums_out)
    {
        P3D_TRY(hipEventRecord(ev1, stream));
        P3D_TRY(hipMemcpyAsync(done_h.data(), done, sizeof(int) * nslices, hipMemcpyDeviceToHost, stream));
        if (sums_out) P3D_TRY(hipMemcpyAsync(sums_out, sums, sizeof(double) * nsum(), hipMemcpyDeviceToHost, stream));
        return P3D_OK;
    }
    int collect(int32_t* niter_done, double* elapsed_ms)
    {
        P3D_TRY(hipStreamSynchronize(stream));
        if (niter_done) niter_from_done(done_h.data(), nslices, niter, niter_done);
        if (elapsed_ms) {
            float ms = 0.f;
            P3D_TRY(hipEventElapsedTime(&ms, ev0, ev1));
            *elapsed_ms = ms;
        }
        return P3D_OK;
    }
};

}  // namespace p3d
