// The second half of the 32 x 32 transform with its exchange reads issued in groups (p3d_fft32.hpp: p32_half2) against the plain loop it
// replaced, restated here: the same operations on the same operands in every lane, so the results are compared BIT FOR BIT, both directions.
// (tests/test_fft32_batched_host.py builds and runs it; the host build of the header takes the same grouping over plain loads.)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "p3d_fft.hpp"
#include "p3d_fft32.hpp"

using namespace p3d;

// the loop p32_half2 was before the reads were grouped
template <int DIR>
void plain_half2(c32 (&v)[32], const c32* row, const c32* tw, int j)
{
    const c32* const q = row + j;
    v[0] = q[0];
    for (int t = 1; t < 32; ++t) {
        const c32 w = tw[(t - 1) * 32 + j];
        v[t] = DIR > 0 ? mul_conj(q[34 * t], w) : q[34 * t] * w;
    }
    dft32<DIR>(v);
}

int fails = 0;

template <int DIR>
void compare(const char* what, const std::vector<c32>& row, const std::vector<c32>& tw)
{
    int bad = 0;
    for (int j = 0; j < 32; ++j) {
        c32 a[32], b[32];
        for (int k = 0; k < 32; ++k) a[k] = b[k] = c32{123.0f + k, -7.0f * j};   // (both halves overwrite every register)
        p32_half2<DIR>(a, row.data(), tw.data(), j);
        plain_half2<DIR>(b, row.data(), tw.data(), j);
        if (std::memcmp(a, b, sizeof(a)) != 0) ++bad;
    }
    std::printf("%-28s dir=%+d lanes that differ: %d %s\n", what, DIR, bad, bad ? "FAIL" : "ok");
    if (bad) ++fails;
}

// every slot of the twiddled exchange a lane reads, once per lane: 32 x 32 values and 31 x 32 twiddles, nothing else and nothing twice --
// checked by poisoning: a buffer of NaNs with only the slots the plain loop names filled in must give the same bits (NaN payloads would show)
template <int DIR>
void compare_poisoned(std::mt19937& rng)
{
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<c32> tw(P32::TW), row(P32::LSTR);
    P32::build_tw(tw.data());
    const float nan = std::nanf("");
    for (auto& z : row) z = c32{nan, nan};
    for (int j = 0; j < 32; ++j)
        for (int t = 0; t < 32; ++t) row[34 * t + j] = c32{u(rng), u(rng)};
    int bad = 0;
    for (int j = 0; j < 32; ++j) {
        c32 a[32];
        p32_half2<DIR>(a, row.data(), tw.data(), j);
        for (int k = 0; k < 32; ++k)
            if (a[k].x != a[k].x || a[k].y != a[k].y) ++bad;
    }
    std::printf("%-28s dir=%+d values that read padding: %d %s\n", "padding slots untouched", DIR, bad, bad ? "FAIL" : "ok");
    if (bad) ++fails;
    compare<DIR>("poisoned padding", row, tw);
}

int main()
{
    std::vector<c32> tw(P32::TW);
    P32::build_tw(tw.data());
    std::mt19937 rng(20240607u);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::normal_distribution<float> g(0.0f, 1.0e3f);
    // seeded random rows, taken through the first half as the kernel does ...
    for (int rep = 0; rep < 8; ++rep) {
        std::vector<c32> row(P32::LSTR, c32{0.f, 0.f});
        for (int j = 0; j < 32; ++j) {
            c32 v[32];
            for (int k = 0; k < 32; ++k) v[k] = rep % 2 ? c32{g(rng), g(rng)} : c32{u(rng), u(rng)};
            if (rep % 4 < 2) p32_half1<FWD>(v, row.data(), j);
            else p32_half1<INV>(v, row.data(), j);
        }
        compare<FWD>("random row (first half)", row, tw);
        compare<INV>("random row (first half)", row, tw);
    }
    // ... and exchange buffers of raw random values
    for (int rep = 0; rep < 4; ++rep) {
        std::vector<c32> row(P32::LSTR);
        for (auto& z : row) z = c32{g(rng), u(rng)};
        compare<FWD>("random exchange buffer", row, tw);
        compare<INV>("random exchange buffer", row, tw);
    }
    // a row of zeros and negative zeros (signs of zero survive a product and tell a * w from a * conj(w))
    {
        std::vector<c32> row(P32::LSTR);
        for (size_t i = 0; i < row.size(); ++i) row[i] = c32{(i % 3) ? -0.0f : 0.0f, (i % 5) ? 0.0f : -0.0f};
        for (int i = 0; i < 40; ++i) row[(size_t)(rng() % row.size())] = c32{u(rng), -0.0f};
        compare<FWD>("zeros and negative zeros", row, tw);
        compare<INV>("zeros and negative zeros", row, tw);
    }
    compare_poisoned<FWD>(rng);
    compare_poisoned<INV>(rng);
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
