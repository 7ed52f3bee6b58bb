// Host-only check of csrc/p3d_dct_tables.hpp (run by tests/test_dct_tables_host.py, or by hand):
//   * fwd[k] = s_k exp(-i pi k / 2N) and inv[k] = exp(+i pi k / 2N) / (2 s_k) against their closed forms, both norms, N = 1 ... 40, and
//     fwd[k] * inv[k] = 1/2;
//   * perm() is a permutation of 0 ... N-1 that sends the even samples to the front in ascending and the odd ones to the back in descending order;
//   * the owners k = 0 ... N/2 with their partners cover every coefficient exactly once, partner() is an involution, and in two dimensions the
//     groups {k1, N1-k1} x {k2, N2-k2} cover every coefficient of an N1 x N2 slice exactly once when self-paired members are written once;
//   * the identities themselves in double precision on a random complex line: a naive DFT of the reordered line, combined with the tables'
//     closed forms, against the defining sum of the DCT-II, and the split followed by the inverse DFT restores the line.
// Prints "ALL OK" and returns 0, or the first failures and 1.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "p3d_dct_tables.hpp"

using namespace p3d;
typedef std::complex<double> cd;
static const double PI = 3.14159265358979323846264338327950288;
static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (++failures <= 20) {               \
                printf("FAILED %s: ", #cond);     \
                printf(__VA_ARGS__);              \
                printf("\n");                     \
            }                                     \
        }                                         \
    } while (0)

int main()
{
    unsigned rs = 12345u;
    auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return (double)(rs >> 8) / (double)(1u << 24) - 0.5; };
    for (int n = 1; n <= 40; ++n) {
        // ---- tables
        for (int norm = 0; norm < 2; ++norm) {
            std::vector<c32> fwd(n), inv(n);
            dct::build_tables(n, norm, fwd.data(), inv.data());
            for (int k = 0; k < n; ++k) {
                const double s = norm == dct::NORM_ORTHO ? (k == 0 ? std::sqrt(0.25 / n) : std::sqrt(0.5 / n)) : 1.0;
                const cd f = s * std::exp(cd(0.0, -PI * k / (2.0 * n))), v = std::exp(cd(0.0, PI * k / (2.0 * n))) / (2.0 * s);
                CHECK(std::fabs(fwd[k].x - f.real()) <= 6e-8 * std::abs(f) && std::fabs(fwd[k].y - f.imag()) <= 6e-8 * std::abs(f), "fwd n=%d k=%d norm=%d", n, k, norm);
                CHECK(std::fabs(inv[k].x - v.real()) <= 6e-8 * std::abs(v) && std::fabs(inv[k].y - v.imag()) <= 6e-8 * std::abs(v), "inv n=%d k=%d norm=%d", n, k, norm);
                const cd prod = cd(fwd[k].x, fwd[k].y) * cd(inv[k].x, inv[k].y);
                CHECK(std::abs(prod - cd(0.5, 0.0)) < 2e-7, "fwd * inv n=%d k=%d norm=%d", n, k, norm);
                CHECK(dct::scale(n, k, norm) == s, "scale n=%d k=%d norm=%d", n, k, norm);
            }
        }
        // ---- reordering
        std::vector<int> hit(n, 0);
        for (int i = 0; i < n; ++i) {
            const int p = dct::perm(n, i);
            CHECK(p >= 0 && p < n, "perm range n=%d i=%d", n, i);
            if (p >= 0 && p < n) ++hit[p];
            CHECK(p == ((i % 2 == 0) ? i / 2 : n - 1 - i / 2), "perm n=%d i=%d", n, i);
        }
        for (int p = 0; p < n; ++p) CHECK(hit[p] == 1, "perm covers n=%d p=%d: %d", n, p, hit[p]);
        // ---- groups along one axis
        CHECK(dct::owners(n) == n / 2 + 1, "owners n=%d", n);
        std::vector<int> cover(n, 0);
        for (int k = 0; k < dct::owners(n); ++k) {
            const int p = dct::partner(n, k);
            CHECK(p >= 0 && p < n && p == (n - k) % n, "partner n=%d k=%d", n, k);
            CHECK(dct::partner(n, p) == k, "partner involution n=%d k=%d", n, k);
            ++cover[k];
            if (p != k) ++cover[p];
            CHECK((p == k) == (k == 0 || 2 * k == n), "self-paired n=%d k=%d", n, k);
        }
        for (int k = 0; k < n; ++k) CHECK(cover[k] == 1, "groups cover n=%d k=%d: %d", n, k, cover[k]);
        // ---- groups of four in two dimensions, written as the group pass writes them
        for (int m = 1; m <= 40; m += (n % 3 == 0 ? 1 : 7)) {
            std::vector<int> c2((size_t)n * m, 0);
            for (int k1 = 0; k1 < dct::owners(n); ++k1)
                for (int k2 = 0; k2 < dct::owners(m); ++k2) {
                    const int p1 = dct::partner(n, k1), p2 = dct::partner(m, k2);
                    ++c2[(size_t)k1 * m + k2];
                    if (p2 != k2) ++c2[(size_t)k1 * m + p2];
                    if (p1 != k1) {
                        ++c2[(size_t)p1 * m + k2];
                        if (p2 != k2) ++c2[(size_t)p1 * m + p2];
                    }
                }
            for (size_t i = 0; i < c2.size(); ++i) CHECK(c2[i] == 1, "2-D groups n=%d m=%d i=%zu: %d", n, m, i, c2[i]);
        }
        // ---- the identities in double precision
        for (int norm = 0; norm < 2; ++norm) {
            std::vector<cd> z(n), v(n), V(n), X(n), W(n), back(n);
            for (int i = 0; i < n; ++i) z[i] = cd(rnd(), rnd());
            for (int i = 0; i < n; ++i) v[dct::perm(n, i)] = z[i];
            for (int k = 0; k < n; ++k) {
                cd acc = 0;
                for (int j = 0; j < n; ++j) acc += v[j] * std::exp(cd(0.0, -2.0 * PI * k * j / n));
                V[k] = acc;
            }
            for (int k = 0; k < n; ++k) {
                const cd f = dct::scale(n, k, norm) * std::exp(cd(0.0, -PI * k / (2.0 * n)));
                X[k] = f * V[k] + std::conj(f) * V[dct::partner(n, k)];
                cd def = 0;   // the defining sum of the DCT-II: 2 sum z[j] cos(pi k (2j + 1) / 2N), scaled
                for (int j = 0; j < n; ++j) def += z[j] * std::cos(PI * k * (2.0 * j + 1.0) / (2.0 * n));
                def *= 2.0 * dct::scale(n, k, norm);
                CHECK(std::abs(X[k] - def) < 1e-12 * (1.0 + std::abs(def)), "DCT-II n=%d k=%d norm=%d", n, k, norm);
            }
            for (int k = 0; k < n; ++k) {
                const cd u = std::exp(cd(0.0, PI * k / (2.0 * n))) / (2.0 * dct::scale(n, k, norm));
                W[k] = k == 0 ? u * X[0] : u * (X[k] - cd(0.0, 1.0) * X[dct::partner(n, k)]);
                CHECK(std::abs(W[k] - V[k]) < 1e-12 * (1.0 + std::abs(V[k])), "split n=%d k=%d norm=%d", n, k, norm);
            }
            for (int j = 0; j < n; ++j) {
                cd acc = 0;
                for (int k = 0; k < n; ++k) acc += W[k] * std::exp(cd(0.0, 2.0 * PI * k * j / n));
                back[j] = acc / (double)n;
            }
            for (int i = 0; i < n; ++i) CHECK(std::abs(back[dct::perm(n, i)] - z[i]) < 1e-12, "round trip n=%d i=%d norm=%d", n, i, norm);
        }
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ALL OK\n");
    return 0;
}
