// p3d_mistie.hip -- step 7 of the workflow (the reference's mistie_correction_segy.py): where the 2-D lines of a survey cross, which shot point of
// either line lies nearest to the crossing, and by how many samples the two lines' (envelope) traces are apart there.
//
//   mistie_tilebox_kernel  bounding box of every tile of TILE consecutive segments of a line (one wavefront per tile, min / max by shuffles).
//   mistie_cross_kernel    one wavefront per (line pair, tile of line i); a lane owns one segment of line i.  The tiles of line j are culled 64 at a
//                          time: every lane compares one tile box with the box of the wave's own tile, the ballot is the list of tiles to visit;
//                          the segments of a visited tile are read at wave-uniform addresses.  All arithmetic in double.  The side of a vertex V
//                          relative to the line through a segment (P, R) is side(V) = (V - P) x R, a function of the three points alone, so two
//                          consecutive segments agree about their shared vertex and a crossing through a vertex is neither lost nor doubled:
//                            proper / touching   the ends of B lie on opposite sides of A (or on it) and the ends of A on opposite sides of B;
//                                                the point is the vertex itself where a side is exactly 0, else A0 + t (A1 - A0), t = e0 / (e0 - e1)
//                            collinear           both ends of B on the line of A: the two ends of the overlap (one point when they coincide),
//                                                always vertices
//                            zero-length         a segment without length is a point and hits what it lies on.
//                          Hits are appended through a (vector) atomic counter to a buffer of given capacity; the counter goes on counting beyond it,
//                          so the caller learns the capacity a second call needs.  The order of the records is not defined: callers sort.
//   mistie_nearest_kernel  one wavefront per (crossing, side): every lane walks the line's vertices with stride 64 keeping its first minimum of
//                          sqrt(dx^2 + dy^2), then a lexicographic (distance, index) minimum over the wave -- np.argmin's first minimum.
//   mistie_xcorr_kernel    one workgroup of 256 per crossing.  The samples of the two windows at which neither trace is exactly 0 are compacted in
//                          order (ballots, wave counts through LDS) into LDS (template LDS = true: 2 n floats, windows of up to
//                          P3D_MISTIE_LDS_SAMPLES) or into a caller's buffer in global memory (LDS = false).  A thread owns whole lags of
//                          scipy.signal.correlate(a, b, 'same') -- cc[k] = sum_l a[l + k - n / 2] b[l] -- and sums them in l order in double (the
//                          product of two floats is exact in double, so the fused multiply-add rounds like the sum alone), keeping the first
//                          maximum and the first minimum of its lags; a lexicographic reduction over the workgroup, then the reference's rule
//                          (arg max if |max| >= |min| else arg min; shift = n / 2 - k).  Pearson's r from centred double sums.  Both forms run the
//                          same operations in the same order on the same values: equal results.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int WAVE = 64;
constexpr int TILE = 64;                        // segments per tile: one per lane
constexpr int XC_BS = 256;                      // workgroup of the correlation kernel
constexpr int XC_WAVES = XC_BS / WAVE;
constexpr int LDS_SAMPLES = P3D_MISTIE_LDS_SAMPLES;
constexpr unsigned MAX_GRID_Y = 65535;

struct Box {
    double x0, y0, x1, y1;
};

struct Pt {
    double x, y;
};

__device__ inline Pt vertex(const double* __restrict__ xy, long long v) { return Pt{xy[2 * v], xy[2 * v + 1]}; }
__device__ inline double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }
__device__ inline bool straddles(double a, double b) { return (a <= 0.0 && b >= 0.0) || (a >= 0.0 && b <= 0.0); }

// ---- tile boxes ------------------------------------------------------------------------------------------------------------------------------
// tile t of line L (tile_off[L] <= t < tile_off[L + 1]) holds segments (t - tile_off[L]) * TILE ... of the line
__device__ inline int owner_of(const long long* __restrict__ off, int n, long long t)
{
    int lo = 0, hi = n;                         // the last L with off[L] <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(WAVE) mistie_tilebox_kernel(const double* __restrict__ xy, const long long* __restrict__ line_off,
                                                              const long long* __restrict__ tile_off, int nlines, Box* __restrict__ box)
{
    const long long t = blockIdx.x;
    const int lane = threadIdx.x;
    const int L = owner_of(tile_off, nlines, t);
    const long long v0 = line_off[L], nseg = line_off[L + 1] - v0 - 1;
    const long long s = (t - tile_off[L]) * TILE + lane;
    double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    if (s < nseg) {
        const Pt a = vertex(xy, v0 + s), b = vertex(xy, v0 + s + 1);
        x0 = fmin(a.x, b.x);
        x1 = fmax(a.x, b.x);
        y0 = fmin(a.y, b.y);
        y1 = fmax(a.y, b.y);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        x0 = fmin(x0, __shfl_xor(x0, d));
        y0 = fmin(y0, __shfl_xor(y0, d));
        x1 = fmax(x1, __shfl_xor(x1, d));
        y1 = fmax(y1, __shfl_xor(y1, d));
    }
    if (lane == 0) box[t] = Box{x0, y0, x1, y1};
}

// ---- crossings -------------------------------------------------------------------------------------------------------------------------------
// the points (0, 1 or 2) at which segment A0 A1 meets segment B0 B1
__device__ inline int segment_hits(Pt a0, Pt a1, Pt b0, Pt b1, Pt& h0, Pt& h1)
{
    const double rx = a1.x - a0.x, ry = a1.y - a0.y, sx = b1.x - b0.x, sy = b1.y - b0.y;
    const bool apoint = rx == 0.0 && ry == 0.0, bpoint = sx == 0.0 && sy == 0.0;
    if (apoint && bpoint) {
        h0 = a0;
        return a0.x == b0.x && a0.y == b0.y ? 1 : 0;
    }
    if (apoint) {                               // the point A0 on the segment B
        const double px = a0.x - b0.x, py = a0.y - b0.y, along = px * sx + py * sy;
        h0 = a0;
        return cross2(px, py, sx, sy) == 0.0 && along >= 0.0 && along <= sx * sx + sy * sy ? 1 : 0;
    }
    const double d0 = cross2(b0.x - a0.x, b0.y - a0.y, rx, ry), d1 = cross2(b1.x - a0.x, b1.y - a0.y, rx, ry);   // sides of B's ends of the line of A
    if (bpoint) {                               // the point B0 on the segment A
        const double along = (b0.x - a0.x) * rx + (b0.y - a0.y) * ry;
        h0 = b0;
        return d0 == 0.0 && along >= 0.0 && along <= rx * rx + ry * ry ? 1 : 0;
    }
    if (d0 == 0.0 && d1 == 0.0) {               // collinear: positions along A in units of 1 / |r|^2
        const double rr = rx * rx + ry * ry;
        const double p0 = (b0.x - a0.x) * rx + (b0.y - a0.y) * ry, p1 = (b1.x - a0.x) * rx + (b1.y - a0.y) * ry;
        const double blo = fmin(p0, p1), bhi = fmax(p0, p1);
        const double lo = fmax(0.0, blo), hi = fmin(rr, bhi);
        if (lo > hi) return 0;
        // either end of the overlap is an end of A or an end of B
        h0 = lo == 0.0 ? a0 : (blo == p0 ? b0 : b1);
        h1 = hi == rr ? a1 : (bhi == p0 ? b0 : b1);
        return lo == hi ? 1 : 2;
    }
    if (!straddles(d0, d1)) return 0;
    const double e0 = cross2(a0.x - b0.x, a0.y - b0.y, sx, sy), e1 = cross2(a1.x - b0.x, a1.y - b0.y, sx, sy);   // sides of A's ends of the line of B
    if (!straddles(e0, e1)) return 0;
    if (e0 == 0.0) h0 = a0;
    else if (e1 == 0.0) h0 = a1;
    else if (d0 == 0.0) h0 = b0;
    else if (d1 == 0.0) h0 = b1;
    else {
        const double t = e0 / (e0 - e1);
        h0 = Pt{a0.x + t * rx, a0.y + t * ry};
    }
    return 1;
}

__device__ inline bool boxes_meet(const Box& a, const Box& b) { return a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1; }

__global__ void __launch_bounds__(WAVE) mistie_cross_kernel(const double* __restrict__ xy, const long long* __restrict__ line_off,
                                                            const long long* __restrict__ tile_off, const Box* __restrict__ box,
                                                            const int* __restrict__ pairs, p3d_mistie_hit* __restrict__ rec, unsigned long long cap,
                                                            unsigned long long* __restrict__ counter)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int li = pairs[2 * pair], lj = pairs[2 * pair + 1];
    const long long vi = line_off[li], nsi = line_off[li + 1] - vi - 1, vj = line_off[lj], nsj = line_off[lj + 1] - vj - 1;
    const long long ti0 = tile_off[li], nti = tile_off[li + 1] - ti0, tj0 = tile_off[lj], ntj = tile_off[lj + 1] - tj0;
    for (long long ti = blockIdx.y; ti < nti; ti += gridDim.y) {
        const Box mine = box[ti0 + ti];
        const long long si = ti * TILE + lane;
        const bool live = si < nsi;
        Pt a0 = Pt{0.0, 0.0}, a1 = a0;
        if (live) {
            a0 = vertex(xy, vi + si);
            a1 = vertex(xy, vi + si + 1);
        }
        for (long long tb = 0; tb < ntj; tb += WAVE) {
            const long long tj = tb + lane;
            unsigned long long visit = __ballot(tj < ntj && boxes_meet(mine, box[tj0 + tj]));
            while (visit) {
                const int bit = __ffsll((long long)visit) - 1;
                visit &= visit - 1;
                const long long q0 = (tb + bit) * TILE;
                const int qn = (int)min((long long)TILE, nsj - q0);
                Pt b0 = vertex(xy, vj + q0);                     // wave-uniform addresses
                for (int q = 0; q < qn; ++q) {
                    const Pt b1 = vertex(xy, vj + q0 + q + 1);
                    Pt h0 = Pt{0.0, 0.0}, h1 = h0;
                    const int nh = live ? segment_hits(a0, a1, b0, b1, h0, h1) : 0;
                    if (nh > 0) {
                        const unsigned long long slot = atomicAdd(counter, (unsigned long long)nh);
                        if (slot < cap) rec[slot] = p3d_mistie_hit{pair, (int)si, (int)(q0 + q), 0, h0.x, h0.y};
                        if (nh > 1 && slot + 1 < cap) rec[slot + 1] = p3d_mistie_hit{pair, (int)si, (int)(q0 + q), 1, h1.x, h1.y};
                    }
                    b0 = b1;
                }
            }
        }
    }
}

// ---- nearest vertex ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) mistie_nearest_kernel(const double* __restrict__ xy, const long long* __restrict__ line_off, int nlines,
                                                              const double* __restrict__ pts, const int* __restrict__ lines, int* __restrict__ idx,
                                                              double* __restrict__ dist)
{
    const long long w = blockIdx.x;             // crossing * 2 + side
    const int lane = threadIdx.x;
    const int L = lines[w];
    double best = INFINITY;
    int at = INT_MAX;
    if (L >= 0 && L < nlines) {
        const double px = pts[2 * (w >> 1)], py = pts[2 * (w >> 1) + 1];
        const long long v0 = line_off[L], nv = line_off[L + 1] - v0;
        for (long long v = lane; v < nv; v += WAVE) {
            const double dx = xy[2 * (v0 + v)] - px, dy = xy[2 * (v0 + v) + 1] - py;
            const double d = sqrt(dx * dx + dy * dy);
            if (d < best || at == INT_MAX) {    // ascending v: a later equal distance does not replace
                best = d;
                at = (int)v;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(at, d);
        if (oa != INT_MAX && (at == INT_MAX || ob < best || (ob == best && oa < at))) {
            best = ob;
            at = oa;
        }
    }
    if (lane == 0) {
        idx[w] = at == INT_MAX ? -1 : at;       // a line without vertices
        dist[w] = best;
    }
}

// ---- windowed cross-correlation ----------------------------------------------------------------------------------------------------------------
struct Extreme {
    double v;
    int k;
};

// BIG: the larger value wins, else the smaller; among equal values the lower index
template <bool BIG>
__device__ inline bool beats(double ov, int ok, double v, int k)
{
    if (ok == INT_MAX) return false;
    if (k == INT_MAX) return true;
    return (BIG ? ov > v : ov < v) || (ov == v && ok < k);
}

template <bool BIG>
__device__ inline Extreme block_extreme(Extreme e, Extreme* __restrict__ stage)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double ov = __shfl_xor(e.v, d);
        const int ok = __shfl_xor(e.k, d);
        if (beats<BIG>(ov, ok, e.v, e.k)) e = Extreme{ov, ok};
    }
    __syncthreads();
    if (lane == 0) stage[wave] = e;
    __syncthreads();
    e = stage[0];
#pragma unroll
    for (int w = 1; w < XC_WAVES; ++w)
        if (beats<BIG>(stage[w].v, stage[w].k, e.v, e.k)) e = stage[w];
    return e;
}

__device__ inline double block_sum(double v, double* __restrict__ stage)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if (lane == 0) stage[wave] = v;
    __syncthreads();
    double s = stage[0];
#pragma unroll
    for (int w = 1; w < XC_WAVES; ++w) s += stage[w];
    return s;
}

// status: 0 = fine, 1 = no sample left after the zeros were dropped, 2 = the two windows differ in length, 3 = a window outside the trace or longer
// than max_len
template <bool LDS>
__global__ void __launch_bounds__(XC_BS) mistie_xcorr_kernel(const float* __restrict__ a, const float* __restrict__ b, int ns,
                                                             const int* __restrict__ ranges, int max_len, float* __restrict__ work, int* __restrict__ shift,
                                                             double* __restrict__ coeff, int* __restrict__ count, int* __restrict__ status)
{
    extern __shared__ float compact[];          // LDS form: [2][len]
    __shared__ int wave_count[XC_WAVES];
    __shared__ double sum_stage[XC_WAVES];
    __shared__ Extreme ext_stage[XC_WAVES];
    const long long c = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int a_lo = ranges[4 * c], a_len = ranges[4 * c + 1], b_lo = ranges[4 * c + 2], b_len = ranges[4 * c + 3];
    int bad = 0;
    if (a_lo < 0 || b_lo < 0 || a_len < 0 || b_len < 0 || (long long)a_lo + a_len > ns || (long long)b_lo + b_len > ns) bad = 3;
    else if (a_len != b_len) bad = 2;
    else if (a_len > max_len) bad = 3;                             // longer than the caller said: never a write outside the LDS
    else if (a_len == 0) bad = 1;
    if (bad) {                                  // block-uniform
        if (tid == 0) {
            shift[c] = 0;
            coeff[c] = 0.0;
            count[c] = 0;
            status[c] = bad;
        }
        return;
    }
    const int len = a_len;
    const float* __restrict__ ta = a + c * ns + a_lo;
    const float* __restrict__ tb = b + c * ns + b_lo;
    float* __restrict__ ca = LDS ? compact : work + c * 2 * ns;
    float* __restrict__ cb = ca + (LDS ? len : ns);

    // the samples at which neither trace is 0, in order
    int n = 0;
    for (int k0 = 0; k0 < len; k0 += XC_BS) {
        const int k = k0 + tid;
        float va = 0.0f, vb = 0.0f;
        if (k < len) {
            va = ta[k];
            vb = tb[k];
        }
        const bool keep = k < len && va != 0.0f && vb != 0.0f;
        const unsigned long long word = __ballot(keep);
        __syncthreads();
        if (lane == 0) wave_count[wave] = __popcll(word);
        __syncthreads();
        int before = n;
#pragma unroll
        for (int w = 0; w < XC_WAVES; ++w) {
            if (w < wave) before += wave_count[w];
            n += wave_count[w];
        }
        if (keep) {
            const int at = before + __popcll(word & ((1ull << lane) - 1ull));
            ca[at] = va;
            cb[at] = vb;
        }
    }
    __syncthreads();                            // the compacted traces are complete (a workgroup sees its own global writes after the barrier)
    if (n == 0) {
        if (tid == 0) {
            shift[c] = 0;
            coeff[c] = 0.0;
            count[c] = 0;
            status[c] = 1;
        }
        return;
    }

    // cc[k] = sum over l of a[l + k - n / 2] b[l], k = 0 ... n - 1
    const int half = n / 2;
    Extreme big = Extreme{0.0, INT_MAX}, small = big;
    for (int k = tid; k < n; k += XC_BS) {
        const int lag = k - half;
        const int l0 = max(0, -lag), l1 = min(n, n - lag);
        double acc = 0.0;
        for (int l = l0; l < l1; ++l) acc = fma((double)ca[l + lag], (double)cb[l], acc);
        if (big.k == INT_MAX || acc > big.v) big = Extreme{acc, k};
        if (small.k == INT_MAX || acc < small.v) small = Extreme{acc, k};
    }
    big = block_extreme<true>(big, ext_stage);
    small = block_extreme<false>(small, ext_stage);

    // Pearson's r of the compacted traces from centred sums
    double sa = 0.0, sb = 0.0;
    for (int l = tid; l < n; l += XC_BS) {
        sa += (double)ca[l];
        sb += (double)cb[l];
    }
    const double ma = block_sum(sa, sum_stage) / (double)n, mb = block_sum(sb, sum_stage) / (double)n;
    double saa = 0.0, sbb = 0.0, sab = 0.0;
    for (int l = tid; l < n; l += XC_BS) {
        const double da = (double)ca[l] - ma, db = (double)cb[l] - mb;
        saa += da * da;
        sbb += db * db;
        sab += da * db;
    }
    saa = block_sum(saa, sum_stage);
    sbb = block_sum(sbb, sum_stage);
    sab = block_sum(sab, sum_stage);
    if (tid == 0) {
        const int k = fabs(big.v) >= fabs(small.v) ? big.k : small.k;
        double r = sab / (sqrt(saa) * sqrt(sbb));                  // NaN for a constant trace, as scipy.stats.pearsonr
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
        shift[c] = half - k;
        coeff[c] = r;
        count[c] = n;
        status[c] = 0;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
int check_lines(const long long* line_off, int nlines)
{
    if (!line_off) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (nlines < 1) return fail(P3D_ERR_INVALID, "at least one line is needed, got %d", nlines);
    if (line_off[0] != 0) return fail(P3D_ERR_INVALID, "the vertex offsets must start at 0, got %lld", line_off[0]);
    for (int L = 0; L < nlines; ++L) {
        const long long nv = line_off[L + 1] - line_off[L];
        if (nv < 0) return fail(P3D_ERR_INVALID, "the vertex offsets must ascend (line %d)", L);
        if (nv > INT_MAX) return fail(P3D_ERR_UNSUPPORTED, "line %d has %lld vertices, more than an int32 index reaches", L, nv);
    }
    return P3D_OK;
}

int cross_dev(const double* xy, const long long* line_off, int nlines, const int* pairs, int npairs, p3d_mistie_hit* rec, size_t cap, size_t* needed)
{
    if (int rc = check_lines(line_off, nlines)) return rc;
    if (!needed || npairs < 0 || (npairs > 0 && !pairs) || (cap > 0 && !rec)) return fail(P3D_ERR_INVALID, "NULL buffer or negative count");
    *needed = 0;
    if (npairs == 0) return P3D_OK;
    if (!xy) return fail(P3D_ERR_INVALID, "NULL buffer");
    std::vector<long long> tile_off(nlines + 1, 0);
    long long most = 0;
    for (int L = 0; L < nlines; ++L) {
        const long long nseg = std::max(line_off[L + 1] - line_off[L] - 1, 0ll), nt = (nseg + TILE - 1) / TILE;
        tile_off[L + 1] = tile_off[L] + nt;
    }
    for (int p = 0; p < npairs; ++p) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || j >= nlines || i >= j) return fail(P3D_ERR_INVALID, "pair %d is (%d, %d): 0 <= i < j < %d is required", p, i, j, nlines);
        most = std::max(most, tile_off[i + 1] - tile_off[i]);
    }
    const long long ntiles = tile_off[nlines];
    if (ntiles == 0 || most == 0) return P3D_OK;
    if (ntiles > 0x7fffffffll) return fail(P3D_ERR_UNSUPPORTED, "too many segment tiles for one launch (%lld)", ntiles);
    const size_t noff = (size_t)(nlines + 1) * sizeof(long long);
    DevBuf dline, dtile, dbox, dpairs, dcount;
    P3D_TRY(hipMalloc(&dline.p, noff));
    P3D_TRY(hipMalloc(&dtile.p, noff));
    P3D_TRY(hipMalloc(&dbox.p, (size_t)ntiles * sizeof(Box)));
    P3D_TRY(hipMalloc(&dpairs.p, (size_t)npairs * 2 * sizeof(int)));
    P3D_TRY(hipMalloc(&dcount.p, sizeof(unsigned long long)));
    P3D_TRY(hipMemcpy(dline.p, line_off, noff, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dtile.p, tile_off.data(), noff, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dpairs.p, pairs, (size_t)npairs * 2 * sizeof(int), hipMemcpyHostToDevice));
    P3D_TRY(hipMemset(dcount.p, 0, sizeof(unsigned long long)));
    mistie_tilebox_kernel<<<(unsigned)ntiles, WAVE, 0, 0>>>(xy, (const long long*)dline.p, (const long long*)dtile.p, nlines, (Box*)dbox.p);
    P3D_TRY(hipGetLastError());
    const dim3 grid((unsigned)npairs, (unsigned)std::min<long long>(most, MAX_GRID_Y));
    mistie_cross_kernel<<<grid, WAVE, 0, 0>>>(xy, (const long long*)dline.p, (const long long*)dtile.p, (const Box*)dbox.p, (const int*)dpairs.p, rec,
                                              (unsigned long long)cap, (unsigned long long*)dcount.p);
    P3D_TRY(hipGetLastError());
    unsigned long long got = 0;
    P3D_TRY(hipMemcpy(&got, dcount.p, sizeof got, hipMemcpyDeviceToHost));
    *needed = (size_t)got;
    return P3D_OK;
}

int nearest_dev(const double* xy, const long long* line_off, int nlines, const double* pts, const int* lines, size_t k, int* idx, double* dist)
{
    if (int rc = check_lines(line_off, nlines)) return rc;
    if (k == 0) return P3D_OK;
    if (!xy || !pts || !lines || !idx || !dist) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (2 * k > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "too many crossings for one launch (%zu)", k);
    const size_t noff = (size_t)(nlines + 1) * sizeof(long long);
    DevBuf doff;
    P3D_TRY(hipMalloc(&doff.p, noff));
    P3D_TRY(hipMemcpy(doff.p, line_off, noff, hipMemcpyHostToDevice));
    mistie_nearest_kernel<<<(unsigned)(2 * k), WAVE, 0, 0>>>(xy, (const long long*)doff.p, nlines, pts, lines, idx, dist);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());              // before the offsets go
    return P3D_OK;
}

int check_xcorr(size_t ncross, int ns, int path)
{
    if (ns < 1) return fail(P3D_ERR_INVALID, "traces need at least 1 sample, got %d", ns);
    if (ncross > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "too many crossings for one launch (%zu)", ncross);
    if (path != P3D_MISTIE_PATH_AUTO && path != P3D_MISTIE_PATH_LDS && path != P3D_MISTIE_PATH_GLOBAL)
        return fail(P3D_ERR_INVALID, "unknown path %d", path);
    return P3D_OK;
}

// max_len: the longest window of the batch (the host knows the windows it made)
int xcorr_dev(const float* a, const float* b, size_t ncross, int ns, const int* ranges, int max_len, int path, float* work, int* shift, double* coeff, int* count,
              int* status)
{
    if (ncross == 0) return P3D_OK;
    if (!a || !b || !ranges || !shift || !coeff || !count || !status) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (max_len < 0 || max_len > ns) return fail(P3D_ERR_INVALID, "the longest window (%d samples) does not fit traces of %d samples", max_len, ns);
    if (path == P3D_MISTIE_PATH_LDS && max_len > LDS_SAMPLES)
        return fail(P3D_ERR_UNSUPPORTED, "windows of up to %d samples fit the LDS, got %d", LDS_SAMPLES, max_len);
    const bool lds = path == P3D_MISTIE_PATH_LDS || (path == P3D_MISTIE_PATH_AUTO && max_len <= LDS_SAMPLES);
    if (lds) {
        mistie_xcorr_kernel<true><<<(unsigned)ncross, XC_BS, (size_t)2 * std::max(max_len, 1) * sizeof(float), 0>>>(a, b, ns, ranges, max_len, nullptr, shift, coeff,
                                                                                                                  count, status);
        P3D_TRY(hipGetLastError());
        return P3D_OK;
    }
    DevBuf own;
    if (!work) {
        P3D_TRY(hipMalloc(&own.p, ncross * 2 * (size_t)ns * sizeof(float)));
        work = (float*)own.p;
    }
    mistie_xcorr_kernel<false><<<(unsigned)ncross, XC_BS, 0, 0>>>(a, b, ns, ranges, max_len, work, shift, coeff, count, status);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());              // before an own work buffer goes
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_mistie_cross_dev(int device, const double* xy_dev, const long long* line_off, int nlines, const int* pairs, int npairs, p3d_mistie_hit* hits_dev,
                         size_t capacity, size_t* needed)
{
    if (int rc = use_device(device)) return rc;
    if (int rc = cross_dev(xy_dev, line_off, nlines, pairs, npairs, hits_dev, capacity, needed)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_mistie_nearest_dev(int device, const double* xy_dev, const long long* line_off, int nlines, const double* points_dev, const int* lines_dev,
                           size_t ncross, int* index_dev, double* dist_dev)
{
    if (int rc = use_device(device)) return rc;
    if (int rc = nearest_dev(xy_dev, line_off, nlines, points_dev, lines_dev, ncross, index_dev, dist_dev)) return rc;
    return P3D_OK;
}

int p3d_mistie_xcorr_dev(int device, const float* a_dev, const float* b_dev, size_t ncross, int ns, const int* ranges_dev, int max_len, int path,
                         float* work_dev, int* shift_dev, double* coeff_dev, int* n_dev, int* status_dev)
{
    if (int rc = check_xcorr(ncross, ns, path)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = xcorr_dev(a_dev, b_dev, ncross, ns, ranges_dev, max_len, path, work_dev, shift_dev, coeff_dev, n_dev, status_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_mistie_cross(int device, const double* xy, const long long* line_off, int nlines, const int* pairs, int npairs, p3d_mistie_hit* hits, size_t capacity,
                     size_t* needed)
{
    if (int rc = check_lines(line_off, nlines)) return rc;
    if (!xy && line_off[nlines] > 0) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nxy = (size_t)line_off[nlines] * 2 * sizeof(double);
    DevBuf dxy, drec;
    P3D_TRY(hipMalloc(&dxy.p, std::max(nxy, sizeof(double))));
    P3D_TRY(hipMalloc(&drec.p, std::max(capacity, (size_t)1) * sizeof(p3d_mistie_hit)));
    if (nxy) P3D_TRY(hipMemcpy(dxy.p, xy, nxy, hipMemcpyHostToDevice));
    if (int rc = cross_dev((const double*)dxy.p, line_off, nlines, pairs, npairs, (p3d_mistie_hit*)drec.p, capacity, needed)) return rc;
    const size_t got = std::min(*needed, capacity);
    if (got) {
        if (!hits) return fail(P3D_ERR_INVALID, "NULL buffer");
        P3D_TRY(hipMemcpy(hits, drec.p, got * sizeof(p3d_mistie_hit), hipMemcpyDeviceToHost));
    }
    return P3D_OK;
}

int p3d_mistie_nearest(int device, const double* xy, const long long* line_off, int nlines, const double* points, const int* lines, size_t ncross, int* index,
                       double* dist)
{
    if (int rc = check_lines(line_off, nlines)) return rc;
    if (ncross == 0) return P3D_OK;
    if (!xy || !points || !lines || !index || !dist) return fail(P3D_ERR_INVALID, "NULL buffer");
    for (size_t w = 0; w < 2 * ncross; ++w)
        if (lines[w] < 0 || lines[w] >= nlines) return fail(P3D_ERR_INVALID, "crossing %zu names line %d of %d", w / 2, lines[w], nlines);
    if (int rc = use_device(device)) return rc;
    const size_t nxy = (size_t)line_off[nlines] * 2 * sizeof(double);
    DevBuf dxy, dpts, dlines, didx, ddist;
    P3D_TRY(hipMalloc(&dxy.p, std::max(nxy, sizeof(double))));
    P3D_TRY(hipMalloc(&dpts.p, ncross * 2 * sizeof(double)));
    P3D_TRY(hipMalloc(&dlines.p, ncross * 2 * sizeof(int)));
    P3D_TRY(hipMalloc(&didx.p, ncross * 2 * sizeof(int)));
    P3D_TRY(hipMalloc(&ddist.p, ncross * 2 * sizeof(double)));
    if (nxy) P3D_TRY(hipMemcpy(dxy.p, xy, nxy, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dpts.p, points, ncross * 2 * sizeof(double), hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dlines.p, lines, ncross * 2 * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = nearest_dev((const double*)dxy.p, line_off, nlines, (const double*)dpts.p, (const int*)dlines.p, ncross, (int*)didx.p,
                             (double*)ddist.p))
        return rc;
    P3D_TRY(hipMemcpy(index, didx.p, ncross * 2 * sizeof(int), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(dist, ddist.p, ncross * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_mistie_xcorr(int device, const float* a, const float* b, size_t ncross, int ns, const int* ranges, int path, int* shift, double* coeff, int* n,
                     int* status)
{
    if (int rc = check_xcorr(ncross, ns, path)) return rc;
    if (ncross == 0) return P3D_OK;
    if (!a || !b || !ranges || !shift || !coeff || !n || !status) return fail(P3D_ERR_INVALID, "NULL buffer");
    int max_len = 0;
    for (size_t c = 0; c < ncross; ++c) {       // windows outside the trace get their status from the kernel, which reads nothing there
        const int la = ranges[4 * c + 1], lb = ranges[4 * c + 3];
        if (la >= 0 && la <= ns) max_len = std::max(max_len, la);
        if (lb >= 0 && lb <= ns) max_len = std::max(max_len, lb);
    }
    if (int rc = use_device(device)) return rc;
    const size_t nsec = ncross * (size_t)ns * sizeof(float);
    DevBuf da, db, dr, ds, dc, dn, dst;
    P3D_TRY(hipMalloc(&da.p, nsec));
    P3D_TRY(hipMalloc(&db.p, nsec));
    P3D_TRY(hipMalloc(&dr.p, ncross * 4 * sizeof(int)));
    P3D_TRY(hipMalloc(&ds.p, ncross * sizeof(int)));
    P3D_TRY(hipMalloc(&dc.p, ncross * sizeof(double)));
    P3D_TRY(hipMalloc(&dn.p, ncross * sizeof(int)));
    P3D_TRY(hipMalloc(&dst.p, ncross * sizeof(int)));
    P3D_TRY(hipMemcpy(da.p, a, nsec, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(db.p, b, nsec, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dr.p, ranges, ncross * 4 * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = xcorr_dev((const float*)da.p, (const float*)db.p, ncross, ns, (const int*)dr.p, max_len, path, nullptr, (int*)ds.p, (double*)dc.p, (int*)dn.p,
                           (int*)dst.p))
        return rc;
    P3D_TRY(hipMemcpy(shift, ds.p, ncross * sizeof(int), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(coeff, dc.p, ncross * sizeof(double), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(n, dn.p, ncross * sizeof(int), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(status, dst.p, ncross * sizeof(int), hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
