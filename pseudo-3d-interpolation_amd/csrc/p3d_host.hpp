// p3d_host.hpp -- the host-side plumbing every HIP unit of libp3d_hip.so repeats: the formatted error, the check of a HIP call,
// a device buffer that frees itself and the selection of the device.  Host code only; what one unit alone needs stays in that unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

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

}  // namespace p3d
