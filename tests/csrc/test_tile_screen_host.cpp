// The column pass's empty-tile screen (p3d_tile_screen.hpp) on the CPU: the SAME functions the kernel calls, on the values the SAME first pass
// (pass_compute<1024, FWD, 0>) leaves in the 64 threads of a column, summed in the kernel's order.  Whenever the screen declares a column empty
// at a threshold, (a) no coefficient of a double-precision transform of the column reaches the threshold's modulus, and (b) none of the
// coefficients the kernel's own float transform would have produced (the engine driven thread by thread, as tests/csrc/test_fft_host.cpp does)
// is kept by the threshold operator -- hard, soft and garrote restated from p3d_shrink.hpp.  Random columns, and the adversarial ones: a single
// spike, a constant column, all energy in one k_a (a pure tone, for which the bound is the exact peak), thresholds within 2^-9 of the peak and of
// the bound, complex thresholds, NaN / infinity in the data or the threshold, coefficients whose square overflows a float.
// (tests/test_tile_screen_host.py builds and runs it.)
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "p3d_fft.hpp"
#include "p3d_tile_screen.hpp"

using namespace p3d;
using cd = std::complex<double>;
constexpr int N = 1024;
using PL = Plan<N>;

template <int P, class MakeLds>
struct Emu {   // the forward transform, pass by pass (a barrier = the phase finished for all threads)
    static void run(std::vector<std::vector<c32>>& regs, MakeLds mk, TwCol tab)
    {
        for (int tl = 0; tl < PL::TPL; ++tl) {
            c32(&v)[PL::PPT] = *reinterpret_cast<c32(*)[PL::PPT]>(regs[tl].data());
            if constexpr (P > 0) canonical_gather<N>(v, mk(), tl);
            pass_compute<N, FWD, P>(v, tab, tl);
        }
        if constexpr (P + 1 < PL::NPASS) {
            for (int tl = 0; tl < PL::TPL; ++tl) {
                c32(&v)[PL::PPT] = *reinterpret_cast<c32(*)[PL::PPT]>(regs[tl].data());
                pass_scatter<N, FWD, P>(v, mk(), tl);
            }
            Emu<P + 1, MakeLds>::run(regs, mk, tab);
        }
    }
};

// lanes8_sum of the kernel: partner lane ^ 1, ^ 2, ^ 4 in units of 8 lanes; every lane ends with the same sum
static float tree8(const float* a)
{
    float x[8], y[8];
    for (int i = 0; i < 8; ++i) x[i] = a[i];
    for (int s = 1; s < 8; s <<= 1) {
        for (int i = 0; i < 8; ++i) y[i] = x[i] + x[i ^ s];
        for (int i = 0; i < 8; ++i) x[i] = y[i];
    }
    return x[0];
}

// the column sum U as the kernel forms it: threads 8w ... 8w + 7 of wavefront w first, then the 8 wavefronts
static float column_bound(const std::vector<c32>& x)
{
    float part[PL::TPL];
    for (int tl = 0; tl < PL::TPL; ++tl) {
        c32 v[PL::PPT];
        for (int q = 0; q < PL::PPT; ++q) v[q] = x[tl + PL::TPL * q];
        pass_compute<N, FWD, 0>(v, TwCol{nullptr}, tl);   // (the first pass reads no twiddles)
        part[tl] = screen_term(v);
    }
    float wave[8];
    for (int w = 0; w < 8; ++w) wave[w] = tree8(part + 8 * w);
    return tree8(wave);
}

// the operators of p3d_shrink.hpp, as decisions: does the coefficient survive?
static bool kept(c32 X, c32 tau, int op)
{
    const float p = X.x * X.x + X.y * X.y;
    const float m = std::sqrt(p);
    if (op == 0) {   // hard_limit reproduces "sqrtf(p) < tau", lexicographically, bit for bit
        if (!(tau.x >= 0.0f)) return true;
        const bool below = m < tau.x || (m == tau.x && tau.y > 0.0f);
        return !below;
    }
    if (m == 0.0f) return false;
    float gr, gi;
    if (op == 1) {
        const float r = 1.0f / m;
        gr = 1.0f - tau.x * r;
        gi = -tau.y * r;
    } else {
        const float r = 1.0f / (m * m);
        gr = 1.0f - (tau.x * tau.x - tau.y * tau.y) * r;
        gi = -(2.0f * tau.x * tau.y) * r;
    }
    return (gr > 0.0f) || (gr == 0.0f && gi >= 0.0f);
}

static int fails = 0, declared = 0, asked = 0;
static std::vector<cd> W(N);
static std::vector<c32> tab(ColTables<N>::slots());

struct Spectrum {
    float U;
    double peak;                 // max |X| of the double-precision transform
    std::vector<c32> Xf;         // the kernel's own coefficients
    bool finite;
};

static Spectrum analyse(const std::vector<c32>& x)
{
    Spectrum s;
    s.U = column_bound(x);
    s.finite = true;
    for (const c32& z : x) s.finite = s.finite && std::isfinite(z.x) && std::isfinite(z.y);
    s.peak = 0.0;
    if (s.finite) {
        for (int k = 0; k < N; ++k) {
            cd acc = 0;
            for (int n = 0; n < N; ++n) acc += cd(x[n].x, x[n].y) * W[(size_t)((long long)n * k % N)];
            s.peak = std::fmax(s.peak, std::abs(acc));
        }
    }
    std::vector<std::vector<c32>> regs(PL::TPL, std::vector<c32>(PL::PPT));
    for (int tl = 0; tl < PL::TPL; ++tl)
        for (int q = 0; q < PL::PPT; ++q) regs[tl][q] = x[tl + PL::TPL * q];
    std::vector<c32> lds(LdsRow::stride(N) + 1);
    auto mk = [&]() { return LdsRow{lds.data()}; };
    Emu<0, decltype(mk)>::run(regs, mk, TwCol{tab.data()});
    for (int tl = 0; tl < PL::TPL; ++tl)
        for (int q = 0; q < PL::PPT; ++q) s.Xf.push_back(regs[tl][q]);
    return s;
}

// one (column, threshold, operator): a column declared empty holds nothing that survives
static bool check_one(const char* what, const Spectrum& s, c32 tau, int op)
{
    ++asked;
    const float thr = screen_threshold(tau, op);
    if (!screen_proves_empty(s.U, thr)) return false;
    ++declared;
    bool ok = s.finite && s.peak < (double)thr;
    int nkept = 0;
    for (const c32& X : s.Xf) nkept += kept(X, tau, op) ? 1 : 0;
    ok = ok && nkept == 0;
    if (!ok) {
        std::printf("FAIL %-22s op=%d tau=(%.9g, %.9g) thr=%.9g U=%.9g peak=%.17g kept=%d\n", what, op, tau.x, tau.y, thr, s.U, s.peak, nkept);
        ++fails;
    }
    return true;
}

// thresholds around the peak and around the bound, real and complex, all three operators; returns how many declared the column empty
static int sweep(const char* what, const std::vector<c32>& x, bool must_declare_some)
{
    const Spectrum s = analyse(x);
    const float pk = (float)s.peak;
    const float scales[] = {0.5f, 1.0f - 0x1p-9f, 1.0f, 1.0f + 0x1p-11f, 1.0f + 0x1p-10f, 1.0f + 0x1p-9f, 1.0f + 0x1p-8f, 1.01f, 2.0f};
    int n = 0;
    for (float base : {pk, s.U})
        for (float sc : scales)
            for (int op = 0; op < 3; ++op) {
                const float t = base * sc;
                n += check_one(what, s, c32{t, 0.0f}, op);
                n += check_one(what, s, c32{t, 0.37f * t}, op);     // (the schedule scales a complex maximum: Im tau != 0 is the rule)
                n += check_one(what, s, c32{t, -0.9f * t}, op);
                n += check_one(what, s, c32{t, 1.5f * t}, op);      // garrote: Re(tau^2) < 0, nothing is zeroed by the modulus
            }
    if (must_declare_some && n == 0) {
        std::printf("FAIL %-22s the screen never declared this column empty (U=%.9g peak=%.9g)\n", what, s.U, s.peak);
        ++fails;
    }
    std::printf("%-24s U / peak = %-10.6g declared empty at %d thresholds\n", what, s.peak > 0 ? s.U / s.peak : 0.0, n);
    return n;
}

int main()
{
    for (int k = 0; k < N; ++k) W[k] = std::polar(1.0, -2.0 * M_PI * k / N);
    ColTables<N>::build(tab.data());
    std::mt19937 rng(20260717u);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::normal_distribution<float> g(0.0f, 1.0f);
    std::vector<c32> x(N);

    for (float amp : {1.0f, 1.0e3f, 1.0e-20f, 1.0e15f}) {
        for (auto& z : x) z = c32{amp * u(rng), amp * u(rng)};
        sweep("random uniform", x, true);
        for (auto& z : x) z = c32{amp * g(rng), amp * g(rng)};
        sweep("random normal", x, true);
    }
    // a sparse spectrum's column as the row pass leaves it: a few strong tones over a noise floor
    for (int rep = 0; rep < 4; ++rep) {
        for (int n = 0; n < N; ++n) {
            cd acc = cd(1e-3 * g(rng), 1e-3 * g(rng));
            for (int k : {3 + 17 * rep, 400 + rep, 1023 - rep}) acc += std::conj(W[(size_t)((long long)n * k % N)]) * (1.0 + 0.3 * rep);
            x[n] = c32{(float)acc.real(), (float)acc.imag()};
        }
        sweep("tones over noise", x, true);
    }
    for (int at : {0, 1, 63, 64, 517, 1023}) {   // a single spike: every |X[k]| equals it, and so does the bound
        for (auto& z : x) z = c32{0.f, 0.f};
        x[at] = c32{0.6f, -0.8f};
        sweep("single spike", x, true);
    }
    for (auto& z : x) z = c32{0.25f, -3.0f};   // a constant column: all of it in X[0]; the bound is exact again
    sweep("constant", x, true);
    // all energy in one k_a: a pure tone at k0 (S_b is non-zero at k0 mod 16 only and the bound IS |X[k0]|) and several tones sharing k_a with
    // phases that line their contributions up
    for (int k0 : {0, 5, 16 * 7 + 5, 1023}) {
        for (int n = 0; n < N; ++n) {
            const cd z = 1.7 * std::conj(W[(size_t)((long long)n * k0 % N)]);
            x[n] = c32{(float)z.real(), (float)z.imag()};
        }
        sweep("pure tone", x, true);
    }
    for (int n = 0; n < N; ++n) {
        cd acc = 0;
        for (int kb = 0; kb < 64; kb += 9) acc += std::conj(W[(size_t)((long long)n * (11 + 16 * kb) % N)]);
        x[n] = c32{(float)acc.real(), (float)acc.imag()};
    }
    sweep("one k_a, several k_b", x, true);
    for (auto& z : x) z = c32{0.f, 0.f};
    sweep("all zero", x, false);   // U = 0: any positive threshold empties it, and rightly
    // values that are not numbers: never declared empty, whatever the threshold
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        for (auto& z : x) z = c32{1e-3f * u(rng), 1e-3f * u(rng)};
        x[777] = c32{0.1f, bad};
        const Spectrum s = analyse(x);
        for (float t : {1.0f, 1.0e30f, std::numeric_limits<float>::infinity()})
            for (int op = 0; op < 3; ++op)
                if (screen_proves_empty(s.U, screen_threshold(c32{t, 0.f}, op))) {
                    std::printf("FAIL a column holding %g was declared empty at tau = %g (U = %g)\n", bad, t, s.U);
                    ++fails;
                }
    }
    // coefficients whose square overflows a float (|X| > 1.8e19) under a threshold that is larger still, or infinite: the operators see |X|^2 = inf, which is
    // not below any limit, and keep them -- so the screen must not answer there (checked like every case: nothing declared empty may hold a kept coefficient),
    // and must still answer for columns safely below that regime
    for (float amp : {1.0e14f, 3.0e15f, 1.0e17f, 3.0e18f, 1.0e20f, 1.0e30f}) {
        for (auto& z : x) z = c32{amp * u(rng), amp * u(rng)};
        const Spectrum s = analyse(x);
        int n = 0;
        for (float t : {1.0e22f, 1.0e30f, 3.0e38f, std::numeric_limits<float>::infinity()})
            for (int op = 0; op < 3; ++op) n += check_one("near the overflow", s, c32{t, 0.0f}, op);
        std::printf("%-24s amp = %-8g U = %-12g declared empty at %d thresholds\n", "near the overflow", amp, s.U, n);
        if (amp <= 1.0e14f && n == 0) {
            std::printf("FAIL columns of amplitude %g (U = %g) were never declared empty under huge thresholds\n", amp, s.U);
            ++fails;
        }
    }
    // thresholds whose real part is negative, zero or NaN: the hard and the soft operator zero nothing (but exact zeros) and the screen must not
    // answer; the garrote looks at Re(tau^2) alone and may (checked like every other case)
    for (auto& z : x) z = c32{1e-3f * u(rng), 1e-3f * u(rng)};
    {
        const Spectrum s = analyse(x);
        for (float t : {-1.0f, 0.0f, -0.0f, std::numeric_limits<float>::quiet_NaN()})
            for (int op = 0; op < 3; ++op)
                if (check_one("odd threshold", s, c32{t, 0.5f}, op) && op != 2) {
                    std::printf("FAIL declared empty at Re tau = %g, operator %d\n", t, op);
                    ++fails;
                }
    }
    std::printf("%d of %d (column, threshold, operator) cases declared empty\n", declared, asked);
    std::printf(fails ? "FAILED %d\n" : "ALL OK\n", fails);
    return fails ? 1 : 0;
}
