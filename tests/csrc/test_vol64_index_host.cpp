// The index arithmetic of the double-precision axis-0 pass (csrc/p3d_vol64_index.hpp) on the CPU, built with the address and undefined-behaviour
// sanitizers (tests/test_vol64_index_host.py).  For every 7-smooth n0 <= 1024: the factorisation multiplies back to n0 with radices of 1, 2, 3, 4, 5, 7, the
// position -> coefficient map is a permutation of 0 ... n0 - 1 and is the map the unpermuted decimation-in-frequency transform produces (checked by running
// that transform in double against the direct sum), the width is 32 / 16 / 8 by the 32-KiB rule and the LDS size stays
// within 163 840 B.  Every other n0 in 0 ... 1100 is refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "p3d_vol64_index.hpp"

namespace vx = p3d::vol64;
using cd = std::complex<double>;

static int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s: ", #cond);               \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            ++fails;                                       \
        }                                                  \
    } while (0)

static bool smooth(int n)
{
    if (n < 1 || n > vx::MAX_N0) return false;
    for (int r : {2, 3, 5, 7})
        while (n % r == 0) n /= r;
    return n == 1;
}

// the stages of vol64_z_kernel's forward transform on one column, with direct r-point sums for the butterflies
static void dif_forward(std::vector<cd>& x, int n0, int nstage, const int* radix)
{
    const double tau = -6.283185307179586476925286766559;
    int M = n0;
    for (int s = 0; s < nstage; ++s) {
        const int r = radix[s], L = M / r;
        for (int b = 0; b < n0 / r; ++b) {
            const int blk = b / L, np = b - blk * L, base = blk * M + np;
            std::vector<cd> a(r), y(r);
            for (int j = 0; j < r; ++j) a[j] = x[base + j * L];
            for (int k = 0; k < r; ++k) {
                cd acc = 0.0;
                for (int j = 0; j < r; ++j) acc += a[j] * std::polar(1.0, tau * (double)((j * k) % r) / r);
                y[k] = acc * std::polar(1.0, tau * (double)(np * k) / M);
            }
            for (int j = 0; j < r; ++j) x[base + j * L] = y[j];
        }
        M = L;
    }
}

int main()
{
    int nsmooth = 0;
    size_t worst_lds = 0;
    for (int n0 = 0; n0 <= 1100; ++n0) {
        int radix[vx::MAX_STAGES + 2] = {0};
        const int ns = vx::factor(n0, radix);
        if (!smooth(n0)) {
            CHECK(ns < 0, "n0 = %d is not 7-smooth but factor() returned %d", n0, ns);
            continue;
        }
        ++nsmooth;
        CHECK(ns >= 1 && ns <= vx::MAX_STAGES, "n0 = %d: %d stages", n0, ns);
        if (ns < 1 || ns > vx::MAX_STAGES) continue;
        int prod = 1;
        for (int s = 0; s < ns; ++s) {
            const int r = radix[s];
            CHECK(r == 1 || r == 2 || r == 3 || r == 4 || r == 5 || r == 7, "n0 = %d: radix %d", n0, r);
            prod *= r;
        }
        CHECK(prod == n0, "n0 = %d: the radices multiply to %d", n0, prod);

        // the map is a permutation
        std::vector<int> seen(n0, 0), coef(n0);
        for (int p = 0; p < n0; ++p) {
            const int k = vx::coef_of_pos(n0, ns, radix, p);
            CHECK(k >= 0 && k < n0, "n0 = %d: position %d -> coefficient %d", n0, p, k);
            if (k >= 0 && k < n0) ++seen[k];
            coef[p] = k;
        }
        for (int k = 0; k < n0; ++k) CHECK(seen[k] == 1, "n0 = %d: coefficient %d appears %d times", n0, k, seen[k]);

        // ... and the one the transform produces: an impulse at sample 1 has the spectrum exp(-2 pi i k / n0)
        {
            std::vector<cd> x(n0, 0.0);
            x[n0 > 1 ? 1 : 0] = 1.0;
            dif_forward(x, n0, ns, radix);
            double err = 0.0;
            for (int p = 0; p < n0; ++p) {
                const cd want = n0 > 1 ? std::polar(1.0, -6.283185307179586476925286766559 * coef[p] / n0) : cd(1.0);
                err = std::fmax(err, std::abs(x[p] - want));
            }
            CHECK(err < 1e-12, "n0 = %d: the transform's order differs from coef_of_pos (%.3e)", n0, err);
        }

        // width and LDS size
        const int w = vx::width(n0);
        CHECK(w == 32 || w == 16 || w == 8, "n0 = %d: width %d", n0, w);
        CHECK(w == 8 || (size_t)16 * n0 * w <= 32768, "n0 = %d: a tile of width %d exceeds 32 KiB", n0, w);
        CHECK(w == 32 || (size_t)16 * n0 * (2 * w) > 32768, "n0 = %d: width %d although %d fits", n0, w, 2 * w);
        CHECK(vx::THREADS % w == 0, "n0 = %d: %d threads do not split into rows of %d", n0, vx::THREADS, w);
        const size_t lds = vx::lds_bytes(n0, w);
        CHECK(lds <= vx::LDS_LIMIT, "n0 = %d: %zu bytes of LDS", n0, lds);
        CHECK(lds >= (size_t)16 * ((size_t)n0 * w + n0) && lds >= sizeof(double) * vx::STAT * vx::THREADS, "n0 = %d: %zu bytes are too few", n0, lds);
        if (lds > worst_lds) worst_lds = lds;
    }
    CHECK(nsmooth == 143, "%d 7-smooth lengths up to 1024", nsmooth);
    CHECK(worst_lds == 147456, "largest LDS size %zu (1024 x 8 points and 1024 roots: 144 KiB)", worst_lds);
    std::printf("%d lengths, largest LDS %zu bytes\n", nsmooth, worst_lds);
    if (fails) {
        std::printf("%d FAILURES\n", fails);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
