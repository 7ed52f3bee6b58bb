// p3d_resident_dct_job.hpp -- the single-kernel POCS loop of the windowed jobs with scipy.fft.dctn / idctn (type 2, norm 'backward' or 'ortho') as the
// transform: the frame of resident_kernel (p3d_resident_job.hpp: a workgroup per job, 16 points per thread, the slice in registers and LDS for all
// iterations, the same sums, early exit and per-job mask words) around the DCT identities of p3d_dct_tables.hpp.
//
//   * The iterate lives in REORDERED sample order on both axes for the whole job, so that fft2 of it is the V of the identities.  The reordering is
//     folded into the global addresses of the one load of x and the one store of out; the mask bits of the held positions are gathered once, from the
//     words patch_pack_kernel packs in natural order (p3d_resident_dct_index.hpp).
//   * Between the forward and the inverse column transform V is staged through the slice buffer (free at that point) and every thread takes four slots
//     of four coefficients {ra, rb} x {ca, cb}: combine V -> X, threshold X, split X -> V', the arithmetic of dct_group_kernel<DCT_FUSED> expression for
//     expression (same factors, same -ffp-contract=off).  A coupled pair (k, N - k) of an axis is one slot index; the self-paired 0 and N/2 share one,
//     as two groups of one -- so a slot always holds four DISTINCT coefficients and stores each exactly once, in place: no barrier between a slot's loads
//     and its stores.
//   * Scaling: the tables' inverse factors carry 1/4 (backward), ifft2's 1 / (N1 N2) is a.scale as in the FFT loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_fft.hpp"
#include "p3d_resident_dct.hpp"
#include "p3d_resident_dct_index.hpp"
#include "p3d_resident_job.hpp"
#include "p3d_shrink.hpp"

namespace p3d {

template <int N1, int N2>
constexpr size_t resident_dct_lds_bytes()
{
    return resident_lds_bytes<N1, N2>() + sizeof(c32) * 2 * (N1 + N2);   // + the factor tables of one norm
}

template <int N1, int N2, int OP>
__global__ __launch_bounds__(N1* N2 / 16) void resident_dct_kernel(const ResidentDctArgs da)
{
    const ResidentArgs& a = da.r;
    constexpr int T = N1 * N2 / 16, TPL2 = N2 / 16, TPL1 = N1 / 16, PPT = 16;
    constexpr int P = LdsRow::stride(N2);
    static_assert(Plan<N1>::PPT == 16 && Plan<N2>::PPT == 16 && T <= 512 && T >= 64, "16 points per thread, one workgroup per job, at most 8192 points");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    c32* twr = reinterpret_cast<c32*>(smem_raw);
    c32* twc = twr + PassTables<N2>::slots();
    c32* buf = twc + ColTables<N1>::slots();
    double* rows = reinterpret_cast<double*>(buf + (size_t)N1 * P);   // per-row sums of |x|, then [N1] the slice's sum
    c32* fac = reinterpret_cast<c32*>(rows + N1 + 8);                 // fwd N1 | inv N1 | fwd N2 | inv N2
    const c32 *f1 = fac, *i1 = fac + N1, *f2 = fac + 2 * N1, *i2 = fac + 2 * N1 + N2;

    const int tid = threadIdx.x;
    const int slice = blockIdx.x;
    const int r = tid / TPL2, tl = tid % TPL2;      // row phase: thread tl of buffer row r holds buffer columns tl + TPL2 q
    const int c = tid % N2, tl1 = tid / N2;         // column phase: thread tl1 of buffer column c holds buffer rows tl1 + TPL1 q
    for (int i = tid; i < PassTables<N2>::slots(); i += T) twr[i] = a.tw_row[i];
    for (int i = tid; i < ColTables<N1>::slots(); i += T) twc[i] = a.tw_col[i];
    for (int i = tid; i < 2 * (N1 + N2); i += T) fac[i] = da.fac[i];
    const TwOrdered tw_r{twr};
    const TwCol tw_c{twc};
    const LdsColPitch<P> lcol{buf + c + (c >> 4)};

    const int state = a.done[slice];   // < 0: all-zero window, handed back untouched
    if (state < 0) {
        const size_t base = ((size_t)slice * N1 + r) * N2 + tl;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            if (a.dtype == 0) reinterpret_cast<c32*>(a.out)[base + TPL2 * q] = c32{0.f, 0.f};
            else reinterpret_cast<float*>(a.out)[base + TPL2 * q] = 0.f;
        }
        return;
    }
    __syncthreads();

    // the sum of |x| over the job, in the order of resident_kernel
    auto slice_sum = [&](float acc) {
        double ws = (double)acc;
#pragma unroll
        for (int o = TPL2 / 2; o > 0; o >>= 1) ws += __shfl_down(ws, o, TPL2);
        if (tl == 0) rows[r] = ws;
        __syncthreads();
        if (tid < 64) {
            double t = 0.0;
            if constexpr (N1 > 64) t = rows[tid] + rows[tid + 64];
            else if (tid < N1) t = rows[tid];
            constexpr int W0 = N1 >= 64 ? 32 : N1 / 2;
#pragma unroll
            for (int o = W0; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
            if (tid == 0) rows[N1] = t;
        }
        __syncthreads();
        return rows[N1];
    };

    // buffer position (r, tl + TPL2 q) holds natural sample (sample_of(N1, r), sample_of(N2, tl + TPL2 q)): the one load of x, the one store of out
    const size_t row0 = ((size_t)slice * N1 + rdct::sample_of(N1, r)) * N2;
    auto at = [&](int q) -> size_t { return row0 + rdct::sample_of(N2, tl + TPL2 * q); };
    c32 xo[PPT], v[PPT];
    const unsigned mbits = rdct::held_bits(a.bits + (size_t)(slice % a.mask_period) * a.bits_stride, N1, N2, r, tl);
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const c32 x = a.dtype == 0 ? reinterpret_cast<const c32*>(a.x)[at(q)] : c32{reinterpret_cast<const float*>(a.x)[at(q)], 0.f};
        xo[q] = x;
        acc += res_abs(x);
        v[q] = x;
    }
    double prev = slice_sum(acc);
    if (tid == 0) a.sums[slice] = prev;

    int done_at = 0;
    for (int k = 0; k < a.niter; ++k) {
        int tl_k = tl, tl1_k = tl1;   // (addresses recomputed per iteration, as in resident_kernel)
        asm volatile("" : "+v"(tl_k), "+v"(tl1_k));
        const LdsRow lrow{buf + (tid / TPL2) * P};
        // ---- fft2 of the reordered iterate: V ----
        line_fft<N2, FWD, true>(v, lrow, tw_r, tl_k);
#pragma unroll
        for (int q = 0; q < PPT; ++q) lrow.at(tl_k + TPL2 * q) = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPT; ++q) v[q] = lcol.at(tl1_k + TPL1 * q);
        line_fft<N1, FWD, false>(v, lcol, tw_c, tl1_k);
        // ---- V through the slice buffer; combine -> threshold -> split per slot (dct_group_kernel<DCT_FUSED>) ----
        __syncthreads();   // every thread is done gathering from the buffer
#pragma unroll
        for (int q = 0; q < PPT; ++q) lcol.at(tl1_k + TPL1 * q) = v[q];
        __syncthreads();
        {
            const Shrink shr(a.tau[(size_t)slice * a.niter + k], OP);
            int tid_k = tid;
            asm volatile("" : "+v"(tid_k));
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const rdct::Slot s = rdct::slot_of(N1, N2, tid_k, g);
                c32* const pa = buf + s.ra * P;
                c32* const pb = buf + s.rb * P;
                const int ca = s.ca + (s.ca >> 4), cb = s.cb + (s.cb >> 4);
                c32 v00 = pa[ca], v01 = pa[cb], v10 = pb[ca], v11 = pb[cb];
                {   // combine: axis 2, then axis 1; a self-paired index is its own partner
                    const c32 t2 = f2[s.ca], t2p = f2[s.cb], t1 = f1[s.ra], t1p = f1[s.rb];
                    const c32 y00 = v00 * t2 + mul_conj(s.pair2 ? v01 : v00, t2), y01 = v01 * t2p + mul_conj(s.pair2 ? v00 : v01, t2p);
                    const c32 y10 = v10 * t2 + mul_conj(s.pair2 ? v11 : v10, t2), y11 = v11 * t2p + mul_conj(s.pair2 ? v10 : v11, t2p);
                    v00 = y00 * t1 + mul_conj(s.pair1 ? y10 : y00, t1);
                    v10 = y10 * t1p + mul_conj(s.pair1 ? y00 : y10, t1p);
                    v01 = y01 * t1 + mul_conj(s.pair1 ? y11 : y01, t1);
                    v11 = y11 * t1p + mul_conj(s.pair1 ? y01 : y11, t1p);
                }
                v00 = shr(v00); v01 = shr(v01); v10 = shr(v10); v11 = shr(v11);
                {   // split: axis 1, then axis 2; index 0 has no partner term, N/2 is its own partner
                    const c32 u1 = i1[s.ra], u1p = i1[s.rb], u2 = i2[s.ca], u2p = i2[s.cb];
                    const c32 y00 = (s.pair1 ? sub_ib(v00, v10) : v00) * u1, y10 = sub_ib(v10, s.pair1 ? v00 : v10) * u1p;
                    const c32 y01 = (s.pair1 ? sub_ib(v01, v11) : v01) * u1, y11 = sub_ib(v11, s.pair1 ? v01 : v11) * u1p;
                    v00 = (s.pair2 ? sub_ib(y00, y01) : y00) * u2;
                    v01 = sub_ib(y01, s.pair2 ? y00 : y01) * u2p;
                    v10 = (s.pair2 ? sub_ib(y10, y11) : y10) * u2;
                    v11 = sub_ib(y11, s.pair2 ? y10 : y11) * u2p;
                }
                pa[ca] = v00; pa[cb] = v01; pb[ca] = v10; pb[cb] = v11;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPT; ++q) v[q] = lcol.at(tl1_k + TPL1 * q);
        // ---- ifft2 ----
        line_fft<N1, INV, false>(v, lcol, tw_c, tl1_k);
        __syncthreads();   // every thread is done gathering from the buffer
#pragma unroll
        for (int q = 0; q < PPT; ++q) lcol.at(tl1_k + TPL1 * q) = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPT; ++q) v[q] = lrow.at(tl_k + TPL2 * q);
        line_fft<N2, INV, true>(v, lrow, tw_r, tl_k);
        // ---- re-insertion (POCS.py:616-619) and cost (POCS.py:622) ----
        acc = 0.f;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            c32 xn = v[q] * a.scale;
            const float m = (float)((mbits >> q) & 1u);
            const float w = 1.0f - a.alpha * m;
            xn = axpby(xn, w, xo[q], a.alpha);
            acc += res_abs(xn);
            v[q] = xn;
        }
        const double cur = slice_sum(acc);
        if (tid == 0) a.sums[(size_t)(k + 1) * a.nslices + slice] = cur;
        const double d = cur - prev;
        const double cost = (d * d) / (cur * cur);
        prev = cur;
        if (a.eps > 0.0 && k > 2 && cost < a.eps) {   // uniform over the workgroup (POCS.py:631)
            done_at = k + 1;
            break;
        }
    }
    if (tid == 0) a.done[slice] = done_at;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        if (a.dtype == 0) reinterpret_cast<c32*>(a.out)[at(q)] = v[q];
        else reinterpret_cast<float*>(a.out)[at(q)] = v[q].x;   // np.real(), POCS.py:656
    }
}

}  // namespace p3d
