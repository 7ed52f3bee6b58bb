// p3d_f64.hpp -- what the double-precision units share beyond p3d_internal.hpp: the complex128 value type with its arithmetic, the threshold
// operators in NumPy's semantics, and the plan of the double-precision FFT loop (p3d_f64.hip), whose buffers the double-precision DCT loop
// (p3d_dct64.hip) runs on.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "p3d.h"
#include "p3d_generic.hpp"
#include "p3d_mix64.hpp"

namespace p3d {
namespace f64 {

struct __attribute__((aligned(16))) c64 {
    double x, y;
};
__device__ __forceinline__ c64 operator+(c64 a, c64 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ c64 operator-(c64 a, c64 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ c64 operator*(c64 a, c64 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ c64 operator*(c64 a, double s) { return {a.x * s, a.y * s}; }
// a +- i b
__device__ __forceinline__ c64 add_i(c64 a, c64 b) { return {a.x - b.y, a.y + b.x}; }
__device__ __forceinline__ c64 sub_i(c64 a, c64 b) { return {a.x + b.y, a.y - b.x}; }

// threshold_operator.py:9-112 on one coefficient, NumPy's semantics for a complex tau (lexicographic comparisons)
__device__ __forceinline__ c64 shrink64(c64 X, c64 tau, int op)
{
    const double m = hypot(X.x, X.y);   // np.absolute
    if (op == 0) {                      // hard: where(|X| < tau, 0, X)
        const bool below = m < tau.x || (m == tau.x && 0.0 < tau.y);
        return below ? c64{0.0, 0.0} : X;
    }
    if (m == 0.0) return c64{0.0, 0.0};   // 1 - tau / 0 = -inf: clipped to 0
    double gr, gi;
    if (op == 1) {          // soft: X * clip(1 - tau / |X|, 0)
        gr = 1.0 - tau.x / m;
        gi = -tau.y / m;
    } else {                // garrote: X * clip(1 - tau^2 / |X|^2, 0)
        const double m2 = m * m;
        gr = 1.0 - (tau.x * tau.x - tau.y * tau.y) / m2;
        gi = -(2.0 * tau.x * tau.y) / m2;
    }
    const bool keep = (gr > 0.0) || (gr == 0.0 && gi >= 0.0);   // lexicographic max(g, 0)
    return keep ? X * c64{gr, gi} : c64{0.0, 0.0};
}

constexpr int F64_MAX_PASSES = 16;
struct Fft64 {
    int n, nf;
    int f[F64_MAX_PASSES];    // radices; 2, 3, 4, 5, 7, 8, 9: in-register butterflies, anything else: direct sums
    int ns[F64_MAX_PASSES];   // product of the earlier radices = distance of a butterfly's outputs
    unsigned mg[F64_MAX_PASSES];   // j / ns = umulhi(j, mg) for j < 2^16 (ns > 1)
};

constexpr int F64_THREADS = 512;

}  // namespace f64
}  // namespace p3d

struct p3d_plan64 {
    using c64 = p3d::f64::c64;
    using Fft64 = p3d::f64::Fft64;
    using GenPlan = p3d::GenPlan;
    static constexpr int F64_THREADS = p3d::f64::F64_THREADS;
    int device = 0, nil = 0, nxl = 0, max_slices = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    GenPlan gcol{}, grow{};
    c64 *tw_col = nullptr, *tw_row = nullptr, *work = nullptr, *tau = nullptr;
    void *st_x = nullptr, *st_out = nullptr;
    double *mask = nullptr, *partial = nullptr, *sums = nullptr, *spart = nullptr;
    size_t mask_cap = 0, mask_stride = 0;   // elements of `mask` (one slice until the first P3D_FLAG_MASK_PER_SLICE job); the stride of the job in progress
    int* done = nullptr;
    size_t tau_cap = 0, sums_cap = 0;
    static constexpr int BLOCKS = 64;
    size_t per() const { return (size_t)nil * nxl; }
    // fused passes (col64_kernel / row64_kernel): tiles of ln_col columns / ln_row rows, the twiddle table in LDS where it fits
    bool fused = false;
    Fft64 fcol{}, frow{};
    int ln_col = 0, ln_row = 0, tw_col_lds = 0, tw_row_lds = 0, thr_col = F64_THREADS, thr_row = F64_THREADS;
    size_t lds_col = 0, lds_row = 0;
    // passes on the mixed-radix register engine (p3d_mix64.hip) where the axis' length has a plan: chosen per axis, same work buffer
    const p3d::mix64::Entry *mcol = nullptr, *mrow = nullptr;
    c64 *tw_mcol = nullptr, *tw_mrow = nullptr;
    c64* dct_tab = nullptr;            // transform_kind = 'DCT' (p3d_dct64.hip), built by the first DCT call: [2 norms][fwd nil | inv nil | fwd nxl | inv nxl] in double
    unsigned char* nzflag = nullptr;   // both passes on the register engine: [max_slices][tiles_col] tile flags of the sparse shortcut
    bool sparse = false;               // ... in use for the job in progress
    // order statistics of the spectrum (p3d_select64.hip), allocated by the first job that needs them: the percentile operators' select state
    // ([niter][nslices] records and weights), histogram and moduli; the histogram of the 'data-driven' sort
    uint64_t *pct_sel = nullptr, *pct_mod = nullptr;
    double* pct_frac = nullptr;
    unsigned *pct_hist = nullptr, *sort_hist = nullptr;
    size_t pct_sel_cap = 0, pct_mod_cap = 0, pct_frac_cap = 0, pct_hist_cap = 0, sort_hist_cap = 0;
    int sorted_slices = 0;             // p3d_pocs64_sorted_spectrum: `work` holds the sorted order keys of that many slices (0: none)
    // the observed cube and the result of the job in progress: the caller's own device buffers where it passed such, else the staging buffers
    const void* cur_x = nullptr;
    void* cur_out = nullptr;
    int tiles_col() const { return (nxl + ln_col - 1) / ln_col; }
    int tiles_row() const { return (nil + ln_row - 1) / ln_row; }
};
