// Host-only check of csrc/p3d_resident_dct_index.hpp, the index maps of the single-kernel DCT loop of the windowed jobs (run by
// tests/test_resident_dct_index_host.py, or by hand), for the eight routed window shapes:
//   * sample_of() is a bijection of every axis and the inverse of dct::perm;
//   * mask_bit() returns mask[i][j] of a random mask packed as patch_pack_kernel packs it (bit q of word (row, tl) = mask[row][tl + (n2 / 16) q]), and
//     held_bits() the bits of the natural samples behind the 16 reordered positions a thread holds;
//   * the slots of all threads partition the N1 x N2 coefficients: four distinct ones per slot, every coefficient in exactly one slot, coupled slots are
//     {k, N - k} pairs and the uncoupled slot holds the self-paired 0 and N/2;
//   * the group step as the kernel writes it (partner selection by pair1 / pair2), in double precision on 32 x 32 and 32 x 64: combine of the DFT of
//     the reordered window is the DCT-II by its defining sum, both norms, and split restores V.
// Prints "ALL OK" and returns 0, or the first failures and 1.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "p3d_resident_dct_index.hpp"

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

struct cdx {
    double x, y;
};
static cd of(cdx a) { return cd(a.x, a.y); }
static cd sub_ib_h(cd a, cd b) { return a - cd(0.0, 1.0) * b; }

// the group step of resident_dct_kernel on V [n1][n2], in double: combine (X returned through `spec`), then split back into V
static void group_step(int n1, int n2, int norm, std::vector<cd>& V, std::vector<cd>& spec, std::vector<int>& stored)
{
    std::vector<cdx> f1(n1), i1(n1), f2(n2), i2(n2);
    dct::build_tables(n1, norm, f1.data(), i1.data());
    dct::build_tables(n2, norm, f2.data(), i2.data());
    const int T = n1 * n2 / 16;
    for (int tid = 0; tid < T; ++tid)
        for (int g = 0; g < 4; ++g) {
            const rdct::Slot s = rdct::slot_of(n1, n2, tid, g);
            cd v00 = V[s.ra * n2 + s.ca], v01 = V[s.ra * n2 + s.cb], v10 = V[s.rb * n2 + s.ca], v11 = V[s.rb * n2 + s.cb];
            {
                const cd t2 = of(f2[s.ca]), t2p = of(f2[s.cb]), t1 = of(f1[s.ra]), t1p = of(f1[s.rb]);
                const cd y00 = v00 * t2 + (s.pair2 ? v01 : v00) * std::conj(t2), y01 = v01 * t2p + (s.pair2 ? v00 : v01) * std::conj(t2p);
                const cd y10 = v10 * t2 + (s.pair2 ? v11 : v10) * std::conj(t2), y11 = v11 * t2p + (s.pair2 ? v10 : v11) * std::conj(t2p);
                v00 = y00 * t1 + (s.pair1 ? y10 : y00) * std::conj(t1);
                v10 = y10 * t1p + (s.pair1 ? y00 : y10) * std::conj(t1p);
                v01 = y01 * t1 + (s.pair1 ? y11 : y01) * std::conj(t1);
                v11 = y11 * t1p + (s.pair1 ? y01 : y11) * std::conj(t1p);
            }
            spec[s.ra * n2 + s.ca] = v00; spec[s.ra * n2 + s.cb] = v01; spec[s.rb * n2 + s.ca] = v10; spec[s.rb * n2 + s.cb] = v11;
            {
                const cd u1 = of(i1[s.ra]), u1p = of(i1[s.rb]), u2 = of(i2[s.ca]), u2p = of(i2[s.cb]);
                const cd y00 = (s.pair1 ? sub_ib_h(v00, v10) : v00) * u1, y10 = sub_ib_h(v10, s.pair1 ? v00 : v10) * u1p;
                const cd y01 = (s.pair1 ? sub_ib_h(v01, v11) : v01) * u1, y11 = sub_ib_h(v11, s.pair1 ? v01 : v11) * u1p;
                v00 = (s.pair2 ? sub_ib_h(y00, y01) : y00) * u2;
                v01 = sub_ib_h(y01, s.pair2 ? y00 : y01) * u2p;
                v10 = (s.pair2 ? sub_ib_h(y10, y11) : y10) * u2;
                v11 = sub_ib_h(y11, s.pair2 ? y10 : y11) * u2p;
            }
            V[s.ra * n2 + s.ca] = v00; V[s.ra * n2 + s.cb] = v01; V[s.rb * n2 + s.ca] = v10; V[s.rb * n2 + s.cb] = v11;
            ++stored[s.ra * n2 + s.ca]; ++stored[s.ra * n2 + s.cb]; ++stored[s.rb * n2 + s.ca]; ++stored[s.rb * n2 + s.cb];
        }
}

int main()
{
    unsigned rs = 2463534242u;
    auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return (double)(rs >> 8) / (double)(1u << 24) - 0.5; };
    const int shapes[8][2] = {{32, 32}, {32, 64}, {64, 32}, {64, 64}, {32, 128}, {128, 32}, {64, 128}, {128, 64}};
    for (const auto& sh : shapes) {
        const int n1 = sh[0], n2 = sh[1], tpl = n2 / 16, T = n1 * n2 / 16;
        // ---- the sample map
        for (int n : {n1, n2}) {
            std::vector<int> hit(n, 0);
            for (int p = 0; p < n; ++p) {
                const int i = rdct::sample_of(n, p);
                CHECK(i >= 0 && i < n, "sample_of(%d, %d) = %d", n, p, i);
                if (i < 0 || i >= n) continue;
                ++hit[i];
                CHECK(dct::perm(n, i) == p, "perm(%d, sample_of(%d)) = %d", n, p, dct::perm(n, i));
            }
            for (int i = 0; i < n; ++i) CHECK(hit[i] == 1, "sample %d of %d is behind %d positions", i, n, hit[i]);
        }
        // ---- the mask bits, from words packed as patch_pack_kernel packs them
        std::vector<unsigned char> mask((size_t)n1 * n2);
        for (auto& m : mask) m = rnd() > 0.0;
        std::vector<uint16_t> words((size_t)n1 * tpl);
        for (int row = 0; row < n1; ++row)
            for (int tl = 0; tl < tpl; ++tl) {
                unsigned w = 0;
                for (int q = 0; q < 16; ++q)
                    if (mask[(size_t)row * n2 + tl + tpl * q]) w |= 1u << q;
                words[(size_t)row * tpl + tl] = (uint16_t)w;
            }
        for (int i = 0; i < n1; ++i)
            for (int j = 0; j < n2; ++j) CHECK(rdct::mask_bit(words.data(), n2, i, j) == mask[(size_t)i * n2 + j], "mask_bit %dx%d (%d, %d)", n1, n2, i, j);
        std::vector<int> held((size_t)n1 * n2, 0);
        for (int tid = 0; tid < T; ++tid) {
            const int r = tid / tpl, tl = tid % tpl;
            const unsigned bits = rdct::held_bits(words.data(), n1, n2, r, tl);
            for (int q = 0; q < 16; ++q) {
                const int i = rdct::sample_of(n1, r), j = rdct::sample_of(n2, tl + tpl * q);
                CHECK(((bits >> q) & 1u) == mask[(size_t)i * n2 + j], "held_bits %dx%d thread %d q %d", n1, n2, tid, q);
                ++held[(size_t)i * n2 + j];
            }
            CHECK(bits < 65536u, "held_bits %dx%d thread %d has high bits", n1, n2, tid);
        }
        for (size_t e = 0; e < held.size(); ++e) CHECK(held[e] == 1, "sample %zu of %dx%d is held by %d thread slots", e, n1, n2, held[e]);
        // ---- the slots
        std::vector<int> owned((size_t)n1 * n2, 0);
        for (int tid = 0; tid < T; ++tid)
            for (int g = 0; g < 4; ++g) {
                const rdct::Slot s = rdct::slot_of(n1, n2, tid, g);
                CHECK(s.ra >= 0 && s.ra < n1 && s.rb >= 0 && s.rb < n1 && s.ca >= 0 && s.ca < n2 && s.cb >= 0 && s.cb < n2, "slot %dx%d thread %d.%d out of range", n1, n2, tid, g);
                CHECK(s.ra != s.rb && s.ca != s.cb, "slot %dx%d thread %d.%d repeats an index", n1, n2, tid, g);
                if (s.pair1) CHECK(s.ra > 0 && s.rb == dct::partner(n1, s.ra), "rows (%d, %d) of %d", s.ra, s.rb, n1);
                else CHECK(s.ra == 0 && s.rb == n1 / 2, "self-paired rows (%d, %d) of %d", s.ra, s.rb, n1);
                if (s.pair2) CHECK(s.ca > 0 && s.cb == dct::partner(n2, s.ca), "columns (%d, %d) of %d", s.ca, s.cb, n2);
                else CHECK(s.ca == 0 && s.cb == n2 / 2, "self-paired columns (%d, %d) of %d", s.ca, s.cb, n2);
                if (failures) continue;
                ++owned[s.ra * n2 + s.ca]; ++owned[s.ra * n2 + s.cb]; ++owned[s.rb * n2 + s.ca]; ++owned[s.rb * n2 + s.cb];
            }
        for (size_t e = 0; e < owned.size(); ++e) CHECK(owned[e] == 1, "coefficient %zu of %dx%d is in %d slots", e, n1, n2, owned[e]);
    }
    // ---- the group step in double precision
    for (const auto& sh : {shapes[0], shapes[1]})
        for (int norm = 0; norm < 2 && !failures; ++norm) {
            const int n1 = sh[0], n2 = sh[1];
            std::vector<cd> z((size_t)n1 * n2), w(z.size()), V(z.size()), tmp(z.size()), X(z.size()), spec(z.size());
            for (auto& e : z) e = cd(rnd(), rnd());
            for (int r = 0; r < n1; ++r)
                for (int p = 0; p < n2; ++p) w[(size_t)r * n2 + p] = z[(size_t)rdct::sample_of(n1, r) * n2 + rdct::sample_of(n2, p)];
            for (int r = 0; r < n1; ++r)       // naive fft2 of the reordered window
                for (int k = 0; k < n2; ++k) {
                    cd a = 0;
                    for (int p = 0; p < n2; ++p) a += w[(size_t)r * n2 + p] * std::exp(cd(0.0, -2.0 * PI * k * p / n2));
                    tmp[(size_t)r * n2 + k] = a;
                }
            for (int k1 = 0; k1 < n1; ++k1)
                for (int k = 0; k < n2; ++k) {
                    cd a = 0;
                    for (int r = 0; r < n1; ++r) a += tmp[(size_t)r * n2 + k] * std::exp(cd(0.0, -2.0 * PI * k1 * r / n1));
                    V[(size_t)k1 * n2 + k] = a;
                }
            for (int i = 0; i < n1; ++i)       // DCT-II by its defining sum, axis 2 then axis 1
                for (int k = 0; k < n2; ++k) {
                    cd a = 0;
                    for (int j = 0; j < n2; ++j) a += z[(size_t)i * n2 + j] * (2.0 * dct::scale(n2, k, norm) * std::cos(PI * k * (2 * j + 1) / (2.0 * n2)));
                    tmp[(size_t)i * n2 + k] = a;
                }
            for (int k1 = 0; k1 < n1; ++k1)
                for (int k = 0; k < n2; ++k) {
                    cd a = 0;
                    for (int i = 0; i < n1; ++i) a += tmp[(size_t)i * n2 + k] * (2.0 * dct::scale(n1, k1, norm) * std::cos(PI * k1 * (2 * i + 1) / (2.0 * n1)));
                    X[(size_t)k1 * n2 + k] = a;
                }
            std::vector<cd> V2 = V;
            std::vector<int> stored(z.size(), 0);
            group_step(n1, n2, norm, V2, spec, stored);
            double ex = 0, ev = 0, nx = 0, nv = 0;
            for (size_t e = 0; e < z.size(); ++e) {
                ex += std::norm(spec[e] - X[e]); nx += std::norm(X[e]);
                ev += std::norm(V2[e] - V[e]); nv += std::norm(V[e]);
                CHECK(stored[e] == 1, "coefficient %zu stored %d times", e, stored[e]);
            }
            CHECK(std::sqrt(ex / nx) < 1e-12, "combine %dx%d norm %d: rel-L2 %.3e against the DCT-II sum", n1, n2, norm, std::sqrt(ex / nx));
            CHECK(std::sqrt(ev / nv) < 1e-12, "split %dx%d norm %d: rel-L2 %.3e against V", n1, n2, norm, std::sqrt(ev / nv));
        }
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("ALL OK\n");
    return 0;
}
