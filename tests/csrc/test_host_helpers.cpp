// Host-only check of csrc/p3d_host.hpp: p3d::fail, P3D_TRY, p3d::DevBuf and the host half of the POCS loops' frame (p3d::grow, the per-slice
// state and its mapping to iteration counts, np.percentile's ranks).  Calls nothing that needs a device: the program defines
// p3d::set_last_error (p3d_api.hip's in the library) and its own hipFree and hipMalloc, which only record their calls.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "p3d_host.hpp"

static std::string g_msg;
namespace p3d { void set_last_error(const char* msg) { g_msg = msg; } }

static int g_frees = 0;
static void* g_freed = nullptr;
extern "C" hipError_t hipFree(void* p)
{
    ++g_frees;
    g_freed = p;
    return hipSuccess;
}

static int g_mallocs = 0, g_malloc_fails = 0;   // g_malloc_fails: that many of the next calls fail
static size_t g_malloc_bytes = 0;
static double g_arena[4];
extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    ++g_mallocs;
    g_malloc_bytes = bytes;
    if (g_malloc_fails > 0) {
        --g_malloc_fails;
        return hipErrorOutOfMemory;
    }
    *p = g_arena;
    return hipSuccess;
}

static int g_bad = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { ++g_bad; printf("FAILED line %d: %s\n", __LINE__, #cond); }     \
    } while (0)

static int try_invalid()
{
    P3D_TRY(hipErrorInvalidValue);
    return P3D_OK;
}

static int try_success(int* reached)
{
    P3D_TRY(hipSuccess);
    *reached = 1;
    return P3D_OK;
}

int main()
{
    // fail returns its code and formats its arguments
    CHECK(p3d::fail(P3D_ERR_INVALID, "device %d out of range (%d visible)", 99, 8) == P3D_ERR_INVALID);
    CHECK(g_msg == "device 99 out of range (8 visible)");
    CHECK(p3d::fail(P3D_ERR_UNSUPPORTED, "a trace of %zu samples, %s", (size_t)12345, "too long") == P3D_ERR_UNSUPPORTED);
    CHECK(g_msg == "a trace of 12345 samples, too long");
    CHECK(p3d::fail(7, "plain") == 7 && g_msg == "plain");

    // a message longer than the buffer is cut to 511 characters and the terminator
    const std::string big(2000, 'x');
    CHECK(p3d::fail(P3D_ERR_INVALID, "%s", big.c_str()) == P3D_ERR_INVALID);
    CHECK(g_msg.size() == 511);
    CHECK(g_msg == big.substr(0, 511));
    CHECK(p3d::fail(P3D_ERR_INVALID, "[%s]", big.c_str()) == P3D_ERR_INVALID);
    CHECK(g_msg.size() == 511 && g_msg[0] == '[' && g_msg.back() == 'x');

    // P3D_TRY: passes on success, otherwise leaves the function with P3D_ERR_HIP and the expression's text in the message
    int reached = 0;
    g_msg = "untouched";
    CHECK(try_success(&reached) == P3D_OK && reached == 1 && g_msg == "untouched");
    CHECK(try_invalid() == P3D_ERR_HIP);
    CHECK(g_msg == "hipErrorInvalidValue failed: invalid argument");

    // DevBuf: an empty one never reaches the runtime, a filled one frees its pointer once
    {
        p3d::DevBuf empty;
        CHECK(empty.p == nullptr);
    }
    CHECK(g_frees == 0);
    int dummy = 0;
    {
        p3d::DevBuf full;
        full.p = &dummy;
    }
    CHECK(g_frees == 1 && g_freed == &dummy);

    // grow: enough capacity -> no runtime call, nothing changes
    double old_block = 0.0;
    double* buf = &old_block;
    size_t cap = 8;
    g_frees = g_mallocs = 0;
    CHECK(p3d::grow(buf, cap, 8) == P3D_OK && p3d::grow(buf, cap, 3) == P3D_OK);
    CHECK(g_frees == 0 && g_mallocs == 0 && buf == &old_block && cap == 8);
    // ... from empty: one allocation, no free
    float* fresh = nullptr;
    size_t fresh_cap = 0;
    CHECK(p3d::grow(fresh, fresh_cap, 5) == P3D_OK);
    CHECK(g_frees == 0 && g_mallocs == 1 && g_malloc_bytes == 5 * sizeof(float) && fresh == (float*)g_arena && fresh_cap == 5);
    // ... a filled buffer: one free, of the old pointer, then one allocation of n * sizeof(T) bytes
    g_frees = g_mallocs = 0;
    g_freed = nullptr;
    CHECK(p3d::grow(buf, cap, 9) == P3D_OK);
    CHECK(g_frees == 1 && g_freed == &old_block && g_mallocs == 1 && g_malloc_bytes == 9 * sizeof(double) && buf == g_arena && cap == 9);
    // ... a failing allocation: P3D_ERR_HIP, the message names the call, pointer null and capacity 0
    g_frees = g_mallocs = 0;
    g_malloc_fails = 1;
    CHECK(p3d::grow(buf, cap, 10) == P3D_ERR_HIP);
    CHECK(g_frees == 1 && g_mallocs == 1 && buf == nullptr && cap == 0);
    CHECK(g_msg.find("hipMalloc(") == 0 && g_msg.find(" failed: ") != std::string::npos);
    CHECK(p3d::grow(buf, cap, 10) == P3D_OK && buf == g_arena && cap == 10 && g_frees == 1);   // (and the next call starts from empty)

    // active -> done: NULL runs every slice, a 0 switches its slice off
    CHECK(p3d::done_from_active(nullptr, 3) == (std::vector<int>{0, 0, 0}));
    const uint8_t active[3] = {1, 0, 1};
    CHECK(p3d::done_from_active(active, 3) == (std::vector<int>{0, -1, 0}));
    // done -> niter_done: switched off = 0 iterations, still running = all of them, converged = where it stopped
    const int done[4] = {-1, 0, 3, 7};
    int32_t nd[4] = {99, 99, 99, 99};
    p3d::niter_from_done(done, 4, 7, nd);
    CHECK(nd[0] == 0 && nd[1] == 7 && nd[2] == 3 && nd[3] == 7);

    // np.percentile's ranks among 11 sorted values, pos = perc / 100 * 10: 0 -> 0 | 100 -> 10 | 25 -> 2.5 | 37 -> 3.7 | below 0, above 100 and NaN
    // clamp (NaN to rank 0); among 101 values 50.5 % -> 50.5; a single value has nothing above it
    unsigned lo = 9, hi = 9;
    float fr = 9.f;
    p3d::percentile_rank(0.0, 11, &lo, &hi, &fr);
    CHECK(lo == 0 && hi == 1 && fr == 0.0f);
    p3d::percentile_rank(100.0, 11, &lo, &hi, &fr);
    CHECK(lo == 10 && hi == 10 && fr == 0.0f);
    p3d::percentile_rank(25.0, 11, &lo, &hi, &fr);
    CHECK(lo == 2 && hi == 3 && fr == 0.5f);
    p3d::percentile_rank(37.0, 11, &lo, &hi, &fr);
    CHECK(lo == 3 && hi == 4 && std::fabs(fr - 0.7f) < 1e-6f);
    p3d::percentile_rank(-5.0, 11, &lo, &hi, &fr);
    CHECK(lo == 0 && hi == 1 && fr == 0.0f);
    p3d::percentile_rank(130.0, 11, &lo, &hi, &fr);
    CHECK(lo == 10 && hi == 10 && fr == 0.0f);
    p3d::percentile_rank(NAN, 11, &lo, &hi, &fr);
    CHECK(lo == 0 && hi == 1 && fr == 0.0f);
    p3d::percentile_rank(50.5, 101, &lo, &hi, &fr);
    CHECK(lo == 50 && hi == 51 && fr == 0.5f);
    p3d::percentile_rank(60.0, 1, &lo, &hi, &fr);
    CHECK(lo == 0 && hi == 0 && fr == 0.0f);

    if (g_bad) return 1;
    printf("ALL OK\n");
    return 0;
}
