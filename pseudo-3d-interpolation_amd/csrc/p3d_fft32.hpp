// p3d_fft32.hpp -- the 1024-point transform as 32 x 32 (two in-register radix-32 butterflies around one exchange): constants, twiddle table and the
// two halves as one lane sees them.  Host-compilable (tests/csrc/test_fft_host.cpp drives the halves lane by lane on the CPU); the kernels that use it
// are in p3d_row_pipe32.hpp.
#pragma once

#include "p3d_fft.hpp"

namespace p3d {

struct P32 {
    static constexpr int N = 1024, ROWS = 16, THREADS = 512, UPB = 8;   // rows / threads / units (row pairs) per workgroup
    static constexpr int LSTR = 1024 + 2 * 32;   // a row's exchange buffer: butterfly j's 32 outputs at 34 j (two padding slots: 16-byte stores, banks spread)
    static constexpr int TW = 31 * 32;           // exp(-2 pi i t j / 1024), t = 1 ... 31, j = 0 ... 31 at (t - 1) * 32 + j; the inverse conjugates
    static constexpr size_t lds_bytes() { return sizeof(c32) * (TW + (size_t)ROWS * LSTR); }
    static void build_tw(c32* out)
    {
        for (int t = 1; t < 32; ++t)
            for (int j = 0; j < 32; ++j) {
                const double ang = -6.283185307179586476925286766559 * double(t) * double(j) / 1024.0;
                out[(t - 1) * 32 + j] = c32{float(__builtin_cos(ang)), float(__builtin_sin(ang))};
            }
    }
};

// ---- in-register radix-32 butterfly, natural order in and out: two radix-16 butterflies (even / odd inputs) and one radix-2 stage ----
// The stage's twiddles W32^k, k = 1 ... 15, are written with SEVEN complex constants: the inverse multiplies by the conjugate through the
// operand modifiers of the same instruction pair (mul_conj), and W32^(k + 8) = W32^k * (-+i) folds into the butterfly's sum (a -+ i b is
// one packed add).  A packed multiply takes its constant from a scalar register PAIR, the compiler keeps every distinct pair alive across the
// loop, and thirty of them -- one per (k, direction) -- pushed the kernel's mask words out of the scalar file into v_readlane traffic.
// multiply by a FORWARD twiddle w, or by its conjugate for the inverse (same instruction pair, the sign in the operand modifiers)
template <int DIR>
P3D_HD c32 mul_tw(c32 a, c32 w) { return DIR > 0 ? mul_conj(a, w) : a * w; }

// Dft<16, DIR> (p3d_fft.hpp) with its nine twiddles written on five forward constants shared by both directions (same reason as below;
// output k at position digit_rev<16>(k) as there).  Not the same roundings as Dft<16>: this kernel family has no bitwise contract with the others.
template <int DIR>
P3D_HD void dft16s(c32* a)
{
    constexpr float H = 0.70710678118654752440f, C = 0.92387953251128675613f, S = 0.38268343236508977173f;
    dft4<DIR>(a[0], a[4], a[8], a[12]);
    dft4<DIR>(a[1], a[5], a[9], a[13]);
    dft4<DIR>(a[2], a[6], a[10], a[14]);
    dft4<DIR>(a[3], a[7], a[11], a[15]);
    a[5] = mul_tw<DIR>(a[5], c32{C, -S});     // W16^1
    a[9] = mul_tw<DIR>(a[9], c32{H, -H});     // W16^2
    a[13] = mul_tw<DIR>(a[13], c32{S, -C});   // W16^3
    a[6] = mul_tw<DIR>(a[6], c32{H, -H});     // 2
    a[10] = mul_i<DIR>(a[10]);                // 4
    a[14] = mul_tw<DIR>(a[14], c32{-H, -H});  // 6
    a[7] = mul_tw<DIR>(a[7], c32{S, -C});     // 3
    a[11] = mul_tw<DIR>(a[11], c32{-H, -H});  // 6
    a[15] = mul_tw<DIR>(a[15], c32{-C, S});   // 9
    dft4<DIR>(a[0], a[1], a[2], a[3]);
    dft4<DIR>(a[4], a[5], a[6], a[7]);
    dft4<DIR>(a[8], a[9], a[10], a[11]);
    dft4<DIR>(a[12], a[13], a[14], a[15]);
}

template <int DIR>
P3D_HD void dft32(c32 (&x)[32])
{
    constexpr float C[8] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f, 0.70710678118654752440f, 0.55557023301960222474f,
                            0.38268343236508977173f, 0.19509032201612826785f};   // cos(k pi / 16)
    constexpr float S[8] = {0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f, 0.70710678118654752440f, 0.83146961230254523708f,
                            0.92387953251128675613f, 0.98078528040323044913f};   // sin(k pi / 16)
    c32 e[16], o[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) { e[m] = x[2 * m]; o[m] = x[2 * m + 1]; }
    dft16s<DIR>(e);
    dft16s<DIR>(o);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // outputs k, k + 16 (twiddle W32^k) and k + 8, k + 24 (twiddle W32^k * W32^8, W32^8 = DIR * i)
        const c32 ea = e[digit_rev<16>(k)], eb = e[digit_rev<16>(k + 8)];
        c32 oa = o[digit_rev<16>(k)], ob = o[digit_rev<16>(k + 8)];
        if (k != 0) {
            const c32 w{C[k], -S[k]};   // exp(-2 pi i k / 32); the inverse conjugates inside the product
            oa = mul_tw<DIR>(oa, w);
            ob = mul_tw<DIR>(ob, w);
        }
        x[k] = ea + oa;
        x[k + 16] = ea - oa;
        // eb + (DIR i) ob, eb - (DIR i) ob
        x[k + 8] = DIR > 0 ? add_ib(eb, ob) : sub_ib(eb, ob);
        x[k + 24] = DIR > 0 ? sub_ib(eb, ob) : add_ib(eb, ob);
    }
}

// The two halves of a 1024-point transform of one row, as one lane j (of 32) sees them; `row` is the row's exchange buffer.
//   first half:  A[j][k1] = sum_t x[j + 32 t] W32^(t k1)                                  -> row[34 j + k1]
//   second half: X[k1 + 32 k2] = sum_j (A[j][k1] W1024^(j k1)) W32^(j k2), lane = k1       -> register k2: canonical layout again
// (written apart so that tests/csrc can drive them lane by lane on the CPU)
template <int DIR>
P3D_HD void p32_half1(c32 (&v)[32], c32* row, int j)
{
    dft32<DIR>(v);
    c32* const p = row + 34 * j;
#pragma unroll
    for (int m = 0; m < 32; ++m) p[m] = v[m];
}
//
// The reads of the second half: v[0] = q[0], v[t] = q[34 t] * tw[32 (t - 1) + j] (times the conjugate for the inverse), q = row + j, then the
// butterfly.  Written as that loop of plain loads the compiler requests a (value, twiddle) pair, waits for it, multiplies and only then requests
// the next: thirty dependent trips to LDS per transform with one or two reads in flight, in a kernel that runs two wavefronts per SIMD
// (measured: 1 - 1.7 % of the headline job, profiles/rowpass_batched_exchange.txt).  So the reads are issued here by hand, in four GROUPS of eight values and their
// eight twiddles (eight ds_read2_b64), two groups ahead of the multiplications: sixteen reads are in flight before the first wait, and a
// transform waits four times.  LDS reads of a wavefront return in order, so `lgkmcnt(8)` behind the request of group g + 1 says group g has
// arrived (anything else the counter may still hold -- a scalar load from before -- only makes the wait longer).  The compiler does not know
// what an asm statement has in flight: the wait takes the group's registers as in-out operands, so whatever uses them depends on the wait.
// On the host the same grouping runs on plain loads (tests/csrc/test_fft32_batched_host.cpp compares it with that loop, bit for bit).
#if defined(__HIP_DEVICE_COMPILE__)
typedef float p32_two __attribute__((ext_vector_type(4)));   // two complex values: what one ds_read2_b64 returns
__device__ __forceinline__ c32 p32_lo(p32_two r) { return c32{r.x, r.y}; }
__device__ __forceinline__ c32 p32_hi(p32_two r) { return c32{r.z, r.w}; }
// base[A], base[B] (A, B < 256: the instruction's offsets count 8-byte units in eight bits)
template <int A, int B>
__device__ __forceinline__ p32_two p32_read2(const c32* base)
{
    static_assert(A >= 0 && A < 256 && B >= 0 && B < 256, "ds_read2_b64 offsets");
    const unsigned addr = (unsigned)(size_t)(const __attribute__((address_space(3))) c32*)base;
    p32_two r;
    asm volatile("ds_read2_b64 %0, %1 offset0:%2 offset1:%3" : "=v"(r) : "v"(addr), "n"(A), "n"(B) : "memory");
    return r;
}
// the eight reads of a group have arrived once at most LEFT younger ones are in flight
template <int LEFT>
__device__ __forceinline__ void p32_arrived(p32_two (&a)[4], p32_two (&w)[4])
{
    __builtin_amdgcn_sched_barrier(0);   // (the multiplications of the group before stay in front of this wait, under the reads just requested)
    asm volatile("s_waitcnt lgkmcnt(%[left])"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])
                 : [left] "n"(LEFT));
}
#else
struct p32_two { c32 lo, hi; };
inline c32 p32_lo(p32_two r) { return r.lo; }
inline c32 p32_hi(p32_two r) { return r.hi; }
template <int A, int B>
inline p32_two p32_read2(const c32* base) { return p32_two{base[A], base[B]}; }
template <int LEFT>
inline void p32_arrived(p32_two (&)[4], p32_two (&)[4]) {}
#endif
// request group G: the values t = 8 G ... 8 G + 7 of lane j (q = row + j: value t at q[34 t]) and their twiddles (twj = tw + j: twiddle t at
// twj[32 (t - 1)], t >= 1).  Pair i holds t = 8 G + 2 i and the one behind it; t = 0 has no twiddle, its slot takes a second copy of t = 1's.
template <int G>
P3D_HD void p32_request(p32_two (&a)[4], p32_two (&w)[4], const c32* q, const c32* twj)
{
    const c32* const qb = q + 34 * 8 * G;
    const c32* const wb = twj + (G == 0 ? 0 : 32 * (8 * G - 1));
    constexpr int D = G == 0 ? -32 : 0;
    a[0] = p32_read2<0, 34>(qb);
    a[1] = p32_read2<68, 102>(qb);
    a[2] = p32_read2<136, 170>(qb);
    a[3] = p32_read2<204, 238>(qb);
    w[0] = p32_read2<(D < 0 ? 0 : D), 32 + D>(wb);
    w[1] = p32_read2<64 + D, 96 + D>(wb);
    w[2] = p32_read2<128 + D, 160 + D>(wb);
    w[3] = p32_read2<192 + D, 224 + D>(wb);
}
// v[t] <- value * twiddle for the eight t of group G: the loop's operations, element by element
template <int DIR, int G>
P3D_HD void p32_twiddle(c32 (&v)[32], const p32_two (&a)[4], const p32_two (&w)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = 8 * G + 2 * i;
        if (t == 0) v[0] = p32_lo(a[0]);
        else v[t] = DIR > 0 ? mul_conj(p32_lo(a[i]), p32_lo(w[i])) : p32_lo(a[i]) * p32_lo(w[i]);
        v[t + 1] = DIR > 0 ? mul_conj(p32_hi(a[i]), p32_hi(w[i])) : p32_hi(a[i]) * p32_hi(w[i]);
    }
}
template <int DIR>
P3D_HD void p32_half2(c32 (&v)[32], const c32* row, const c32* tw, int j)
{
    const c32* const q = row + j;
    const c32* const twj = tw + j;
    p32_two a0[4], w0[4], a1[4], w1[4], a2[4], w2[4], a3[4], w3[4];
    p32_request<0>(a0, w0, q, twj);
    p32_request<1>(a1, w1, q, twj);
    p32_arrived<8>(a0, w0);
    p32_twiddle<DIR, 0>(v, a0, w0);
    p32_request<2>(a2, w2, q, twj);
    p32_arrived<8>(a1, w1);
    p32_twiddle<DIR, 1>(v, a1, w1);
    p32_request<3>(a3, w3, q, twj);
    p32_arrived<8>(a2, w2);
    p32_twiddle<DIR, 2>(v, a2, w2);
    p32_arrived<0>(a3, w3);
    p32_twiddle<DIR, 3>(v, a3, w3);
    dft32<DIR>(v);
}

}  // namespace p3d
