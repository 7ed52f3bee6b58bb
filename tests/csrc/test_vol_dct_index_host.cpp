// The index arithmetic of the axis-0 cosine pass (csrc/p3d_vol_dct_index.hpp) on the CPU, built with the address and undefined-behaviour sanitizers
// (tests/test_vol_dct_index_host.py).  For every 7-smooth n0 <= 1024: position <-> coefficient are inverse permutations, the partner of a position is the
// position of (n0 - k) mod n0, the pairs of the owners k = 0 ... n0/2 cover every position exactly once, row <-> slice (perm / unperm) are inverse, the width
// follows the 32-KiB rule and the LDS size stays within 163 840 B.  Every other n0 in 0 ... 1100 is refused.  For axis lengths 1 ... 40 the identities of
// p3d_dct_tables.hpp (reorder, FFT, combine, split) hold in double against the direct DCT-II sum, both norms; for the 7-smooth ones among them the column
// program of voldct_z_kernel itself -- load through the reordering, unpermuted forward stages, the group step at the table's positions, transposed inverse,
// store through the reordering -- gives the DCT at the owners' positions and returns the column.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "p3d_dct_tables.hpp"
#include "p3d_vol_dct_index.hpp"

namespace vx = p3d::voldct;
namespace dct = p3d::dct;
using cd = std::complex<double>;
struct c128 { double x, y; };

static const double PI = 3.14159265358979323846264338327950288;
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

// one stage of the kernel's transform on a column, with direct r-point sums for the butterflies: forward (butterfly, then twiddle) or its transpose with
// conjugate roots (twiddle, then butterfly)
static void stage(std::vector<cd>& x, int n0, int r, int L, bool inverse)
{
    const int M = r * L;
    const double sgn = inverse ? 2.0 * PI : -2.0 * PI;
    for (int b = 0; b < n0 / r; ++b) {
        const int blk = b / L, np = b - blk * L, base = blk * M + np;
        std::vector<cd> a(r), y(r);
        for (int j = 0; j < r; ++j) a[j] = x[base + j * L];
        if (inverse)
            for (int k = 0; k < r; ++k) a[k] *= std::polar(1.0, sgn * (double)(np * k) / M);
        for (int k = 0; k < r; ++k) {
            cd acc = 0.0;
            for (int j = 0; j < r; ++j) acc += a[j] * std::polar(1.0, sgn * (double)((j * k) % r) / r);
            y[k] = inverse ? acc : acc * std::polar(1.0, sgn * (double)(np * k) / M);
        }
        for (int j = 0; j < r; ++j) x[base + j * L] = y[j];
    }
}

// scipy.fft.dct(z, type=2, norm=...) of a complex column by the direct sum
static std::vector<cd> dct2_direct(const std::vector<cd>& z, int norm)
{
    const int n = (int)z.size();
    std::vector<cd> X(n);
    for (int k = 0; k < n; ++k) {
        cd acc = 0.0;
        for (int i = 0; i < n; ++i) acc += z[i] * std::cos(PI * (2.0 * i + 1.0) * k / (2.0 * n));
        X[k] = 2.0 * dct::scale(n, k, norm) * acc;
    }
    return X;
}

static cd tab(const c128& t) { return cd(t.x, t.y); }

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

        // position <-> coefficient: inverse permutations
        std::vector<int> seen(n0, 0);
        for (int p = 0; p < n0; ++p) {
            const int k = vx::coef_of_pos(n0, ns, radix, p);
            CHECK(k >= 0 && k < n0, "n0 = %d: position %d -> coefficient %d", n0, p, k);
            if (k < 0 || k >= n0) continue;
            ++seen[k];
            const int back = vx::pos_of_coef(n0, ns, radix, k);
            CHECK(back == p, "n0 = %d: position %d -> coefficient %d -> position %d", n0, p, k, back);
            // the partner of a position is the position of (n0 - k) mod n0
            const int pp = vx::partner_pos(n0, ns, radix, p);
            CHECK(pp == vx::pos_of_coef(n0, ns, radix, (n0 - k) % n0), "n0 = %d: partner of position %d is %d", n0, p, pp);
            CHECK(pp >= 0 && pp < n0 && vx::partner_pos(n0, ns, radix, pp) == p, "n0 = %d: the partner of the partner of position %d", n0, p);
        }
        for (int k = 0; k < n0; ++k) {
            CHECK(seen[k] == 1, "n0 = %d: coefficient %d appears %d times", n0, k, seen[k]);
            const int p = vx::pos_of_coef(n0, ns, radix, k);
            CHECK(p >= 0 && p < n0 && p <= 65535, "n0 = %d: coefficient %d -> position %d", n0, k, p);
        }

        // the owners' pairs cover every position exactly once
        std::vector<int> cover(n0, 0);
        for (int k = 0; k < dct::owners(n0); ++k) {
            const int kp = dct::partner(n0, k), a = vx::pos_of_coef(n0, ns, radix, k), b = vx::pos_of_coef(n0, ns, radix, kp);
            ++cover[a];
            if (kp != k) ++cover[b];
            CHECK(b == vx::partner_pos(n0, ns, radix, a), "n0 = %d: owner %d", n0, k);
        }
        for (int p = 0; p < n0; ++p) CHECK(cover[p] == 1, "n0 = %d: position %d is covered %d times", n0, p, cover[p]);

        // rows <-> slices
        std::vector<int> rows(n0, 0);
        for (int z = 0; z < n0; ++z) {
            const int p = dct::perm(n0, z);
            CHECK(p >= 0 && p < n0 && vx::unperm(n0, p) == z, "n0 = %d: slice %d -> row %d -> slice %d", n0, z, p, vx::unperm(n0, p));
            if (p >= 0 && p < n0) ++rows[p];
        }
        for (int p = 0; p < n0; ++p) CHECK(rows[p] == 1, "n0 = %d: row %d is loaded %d times", n0, p, rows[p]);

        // width and LDS size
        const int w = vx::width(n0);
        CHECK(w == 64 || w == 32 || w == 16, "n0 = %d: width %d", n0, w);
        CHECK(w == 16 || (size_t)8 * n0 * w <= 32768, "n0 = %d: a tile of width %d exceeds 32 KiB", n0, w);
        CHECK(w == 64 || (size_t)8 * n0 * (2 * w) > 32768, "n0 = %d: width %d although %d fits", n0, w, 2 * w);
        CHECK(vx::THREADS % w == 0, "n0 = %d: %d threads do not split into rows of %d", n0, vx::THREADS, w);
        const size_t lds = vx::lds_bytes(n0, w);
        CHECK(lds <= vx::LDS_LIMIT, "n0 = %d: %zu bytes of LDS", n0, lds);
        CHECK(lds >= (size_t)8 * ((size_t)n0 * w + n0) + 2 * (size_t)n0 && lds >= 24 * (size_t)vx::THREADS, "n0 = %d: %zu bytes are too few", n0, lds);
        CHECK(lds % 8 == 0 && vx::pos_table_bytes(n0) % 8 == 0, "n0 = %d: %zu bytes are not whole elements", n0, lds);
        if (lds > worst_lds) worst_lds = lds;
    }
    CHECK(nsmooth == 143, "%d 7-smooth lengths up to 1024", nsmooth);
    CHECK(worst_lds == 141312, "largest LDS size %zu (1024 x 16 points, 1024 roots, 1024 positions: 138 KiB)", worst_lds);

    // the identities, axis lengths 1 ... 40, both norms
    double worst_id = 0.0, worst_col = 0.0;
    for (int n = 1; n <= 40; ++n) {
        std::vector<cd> z(n);
        for (int i = 0; i < n; ++i) z[i] = cd(std::sin(0.7 * i + 0.3 * n) + 0.01 * i, std::cos(1.3 * i - 0.2 * n));
        for (int norm = 0; norm < 2; ++norm) {
            std::vector<c128> f(n), g(n);
            dct::build_tables<c128>(n, norm, f.data(), g.data());
            const std::vector<cd> want = dct2_direct(z, norm);
            double ref = 0.0;
            for (int k = 0; k < n; ++k) ref = std::fmax(ref, std::abs(want[k]));

            // reorder, direct DFT, combine; split, inverse DFT, undo the reordering
            std::vector<cd> v(n), V(n), X(n), V2(n), v2(n);
            for (int i = 0; i < n; ++i) v[dct::perm(n, i)] = z[i];
            for (int k = 0; k < n; ++k) {
                cd acc = 0.0;
                for (int i = 0; i < n; ++i) acc += v[i] * std::polar(1.0, -2.0 * PI * (double)((i * k) % n) / n);
                V[k] = acc;
            }
            for (int k = 0; k < n; ++k) X[k] = tab(f[k]) * V[k] + std::conj(tab(f[k])) * V[dct::partner(n, k)];
            for (int k = 0; k < n; ++k) worst_id = std::fmax(worst_id, std::abs(X[k] - want[k]) / ref);
            for (int k = 0; k < n; ++k) V2[k] = k == 0 ? tab(g[0]) * X[0] : tab(g[k]) * (X[k] - cd(0.0, 1.0) * X[dct::partner(n, k)]);
            for (int k = 0; k < n; ++k) worst_id = std::fmax(worst_id, std::abs(V2[k] - V[k]) / ref);
            for (int i = 0; i < n; ++i) {
                cd acc = 0.0;
                for (int k = 0; k < n; ++k) acc += V2[k] * std::polar(1.0, 2.0 * PI * (double)((i * k) % n) / n);
                v2[i] = acc / (double)n;
            }
            for (int i = 0; i < n; ++i) worst_id = std::fmax(worst_id, std::abs(v2[dct::perm(n, i)] - z[i]));

            // the column program of the kernel
            int radix[vx::MAX_STAGES + 2] = {0};
            const int ns = vx::factor(n, radix);
            if (ns < 0) continue;
            std::vector<cd> col(n), Xk(n);
            for (int p = 0; p < n; ++p) col[p] = z[vx::unperm(n, p)];
            int M = n;
            for (int s = 0; s < ns; ++s) {
                stage(col, n, radix[s], M / radix[s], false);
                M /= radix[s];
            }
            for (int k = 0; k < dct::owners(n); ++k) {
                const int kp = dct::partner(n, k), a = vx::pos_of_coef(n, ns, radix, k), b = vx::pos_of_coef(n, ns, radix, kp);
                const cd vk = col[a], vp = col[b];
                const cd xk = tab(f[k]) * vk + std::conj(tab(f[k])) * vp, xp = tab(f[kp]) * vp + std::conj(tab(f[kp])) * vk;
                Xk[k] = xk;
                Xk[kp] = xp;
                col[a] = k == 0 ? tab(g[0]) * xk : tab(g[k]) * (xk - cd(0.0, 1.0) * xp);
                if (kp != k) col[b] = tab(g[kp]) * (xp - cd(0.0, 1.0) * xk);
            }
            for (int k = 0; k < n; ++k) worst_col = std::fmax(worst_col, std::abs(Xk[k] - want[k]) / ref);
            M = 1;
            for (int s = ns - 1; s >= 0; --s) {
                stage(col, n, radix[s], M, true);
                M *= radix[s];
            }
            for (int p = 0; p < n; ++p) worst_col = std::fmax(worst_col, std::abs(col[p] / (double)n - z[vx::unperm(n, p)]));
        }
    }
    CHECK(worst_id < 1e-12, "the identities of p3d_dct_tables.hpp miss by %.3e", worst_id);
    CHECK(worst_col < 1e-12, "the column program misses by %.3e", worst_col);
    std::printf("%d lengths, largest LDS %zu bytes, identities %.2e, column program %.2e\n", nsmooth, worst_lds, worst_id, worst_col);
    if (fails) {
        std::printf("%d FAILURES\n", fails);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
