// The plain-C++ helpers of the double-precision order statistics on the CPU: the order-preserving key of a double and its inverse, the key of a
// modulus (csrc/p3d_select64.hpp), np.percentile's rank and double weight (csrc/p3d_host.hpp, beside the float one), and NumPy's interpolation of two
// order statistics -- against a sort-based percentile written out here and against literals taken from np.percentile.
// Built as host code only: hipcc -x hip --offload-host-only (the headers include the HIP runtime's declarations).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "p3d_host.hpp"
#include "p3d_select64.hpp"

namespace p3d { void set_last_error(const char*) {} }   // (p3d_host.hpp's fail() records its message through the library; not needed here)

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

using namespace p3d::sel64;

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

static void test_keys()
{
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min(), tiny = std::numeric_limits<double>::min();
    const double ladder[] = {-inf, -1.7976931348623157e308, -2.5, -1.0, -tiny, -den, 0.0, den, tiny, 1.0, 1.0000000000000002, 2.5, 1.7976931348623157e308, inf};
    const int n = sizeof ladder / sizeof ladder[0];
    for (int i = 0; i + 1 < n; ++i) CHECK(ord64(ladder[i]) < ord64(ladder[i + 1]));
    for (int i = 0; i < n; ++i) CHECK(bits(unord64(ord64(ladder[i]))) == bits(ladder[i]));
    CHECK(ord64(-0.0) == ord64(0.0));                      // NumPy compares them equal
    CHECK(bits(unord64(ord64(-0.0))) == bits(0.0));        // ... and the key stands for +0.0
    std::mt19937_64 rng(1);
    for (int i = 0; i < 200000; ++i) {
        double a, b;
        uint64_t ua = rng(), ub = rng();
        std::memcpy(&a, &ua, 8); std::memcpy(&b, &ub, 8);
        if (std::isnan(a) || std::isnan(b)) continue;
        CHECK((a < b) == (ord64(a) < ord64(b)) && (a == b) == (ord64(a) == ord64(b)));
        const double r = unord64(ord64(a));
        CHECK(r == a && (a == 0.0 || bits(r) == bits(a)));
        const double ma = std::fabs(a), mb = std::fabs(b);   // moduli order like their bit patterns
        CHECK((ma < mb) == (mod_key(ma) < mod_key(mb)) && bits(mod_value(mod_key(ma))) == bits(ma));
    }
    CHECK(mod_key(0.0) == 0 && mod_key(den) == 1 && mod_key(inf) == 0x7ff0000000000000ull);
}

static void test_rank()
{
    unsigned lo, hi;
    double fr;
    p3d::percentile_rank64(0.0, 11, &lo, &hi, &fr);    CHECK(lo == 0 && hi == 1 && fr == 0.0);
    p3d::percentile_rank64(100.0, 11, &lo, &hi, &fr);  CHECK(lo == 10 && hi == 10 && fr == 0.0);
    p3d::percentile_rank64(25.0, 11, &lo, &hi, &fr);   CHECK(lo == 2 && hi == 3 && fr == 0.5);
    p3d::percentile_rank64(-5.0, 11, &lo, &hi, &fr);   CHECK(lo == 0 && hi == 1 && fr == 0.0);
    p3d::percentile_rank64(130.0, 11, &lo, &hi, &fr);  CHECK(lo == 10 && hi == 10 && fr == 0.0);
    p3d::percentile_rank64(NAN, 11, &lo, &hi, &fr);    CHECK(lo == 0 && hi == 1 && fr == 0.0);
    p3d::percentile_rank64(60.0, 1, &lo, &hi, &fr);    CHECK(lo == 0 && hi == 0 && fr == 0.0);
    p3d::percentile_rank64(50.0, 1155, &lo, &hi, &fr); CHECK(lo == 577 && hi == 578 && fr == 0.0);
    // (n - 1) * (perc / 100) in double, NumPy's own expression: 4095 * 0.373 = 1527.435, the weight keeps all its bits
    p3d::percentile_rank64(37.3, 4096, &lo, &hi, &fr);
    CHECK(lo == 1527 && hi == 1528 && fr == 4095.0 * (37.3 / 100.0) - 1527.0 && std::fabs(fr - 0.435) < 1e-12);
    float f32;
    p3d::percentile_rank(37.3, 4096, &lo, &hi, &f32);   // the float32 loop's weight: the same ranks, the weight rounded to float (left as it is)
    CHECK(lo == 1527 && hi == 1528 && f32 == (float)fr && (double)f32 != fr);
    p3d::percentile_rank64(97.0, (size_t)5120 * 5120, &lo, &hi, &fr);
    CHECK(lo == 25427967u && hi == 25427968u && fr == 26214399.0 * 0.97 - 25427967.0);
}

// np.percentile(v, perc) by sorting: the rank, then _lerp
static double percentile_by_sort(std::vector<double> v, double perc)
{
    std::sort(v.begin(), v.end());
    unsigned lo, hi;
    double fr;
    p3d::percentile_rank64(perc, v.size(), &lo, &hi, &fr);
    return lerp64(v[lo], v[hi], fr);
}

static void test_lerp()
{
    CHECK(lerp64(1.0, 3.0, 0.0) == 1.0 && lerp64(1.0, 3.0, 0.25) == 1.5 && lerp64(1.0, 3.0, 0.5) == 2.0 && lerp64(1.0, 3.0, 0.75) == 2.5);
    CHECK(lerp64(7.0, 7.0, 0.3) == 7.0 && lerp64(7.0, 7.0, 0.9) == 7.0 && lerp64(0.0, 0.0, 0.5) == 0.0);
    // the two branches differ in the last bit: below 0.5 from the left value, from 0.5 on from the right one (numpy.lib._function_base_impl._lerp)
    const double a = 0.1, b = 0.7;
    CHECK(lerp64(a, b, 0.3) == a + (b - a) * 0.3 && lerp64(a, b, 0.6) == b - (b - a) * (1.0 - 0.6));
    CHECK(lerp64(a, b, 0.5) == b - (b - a) * 0.5);
    // literals: np.percentile([0.1, 0.7, 0.2, 0.9, 0.4], [37.3, 80.0, 50.0]) (NumPy 2.2) = 0.2984, 0.74, 0.4
    const std::vector<double> v = {0.1, 0.7, 0.2, 0.9, 0.4};
    CHECK(percentile_by_sort(v, 37.3) == 0.2984);
    CHECK(percentile_by_sort(v, 80.0) == 0.74);
    CHECK(percentile_by_sort(v, 50.0) == 0.4 && percentile_by_sort(v, 0.0) == 0.1 && percentile_by_sort(v, 100.0) == 0.9);
}

int main()
{
    test_keys();
    test_rank();
    test_lerp();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
