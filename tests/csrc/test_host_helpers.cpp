// Host-only check of csrc/p3d_host.hpp: p3d::fail, P3D_TRY and p3d::DevBuf.  Calls nothing that needs a device: the program defines
// p3d::set_last_error (p3d_api.hip's in the library) and its own hipFree, which only records its calls.
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

    if (g_bad) return 1;
    printf("ALL OK\n");
    return 0;
}
