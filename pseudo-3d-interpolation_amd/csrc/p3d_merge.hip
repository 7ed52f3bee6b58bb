// p3d_merge.hip -- step 1 of the workflow (the reference's merge_segys.py, which leaves the work to pandas and segyio): the device part of merging
// short SEG-Y files with their neighbours.  A record is a 240-byte trace header followed by the samples, `reclen` bytes in all; the records of a
// group of files lie back to back on the device.  Both kernels only move, compare and interpolate words, so their results are bit-identical to the
// NumPy restatement (tests/helpers/merge_numpy.py); the word arithmetic is that of p3d_merge_words.hpp.
//
//   merge_keys_kernel      one wavefront per record, four records per workgroup.  Lanes 0 ... 59 each load one dword of the header (240 coalesced bytes;
//                          four byte loads each where the records are not 4-byte aligned).  Per record: TRACE_SEQUENCE_LINE (bytes 1-4) and two 64-bit
//                          fingerprints of the header, which the host uses to find duplicates: lane l turns its dword d into the term
//                          splitmix64((l + 1) << 32 | d) (the lane number makes the fingerprint sensitive to the order of the dwords), and the terms
//                          are combined with an XOR butterfly over the wave.  The second fingerprint leaves out dword 1 (bytes 5-8,
//                          TRACE_SEQUENCE_FILE): with XOR as the combination it is the first one XOR lane 1's term.
//   merge_records_kernel   the output records.  Row r with src[r] >= 0 is record src[r] moved verbatim but for bytes 5-8 = big-endian r + 1; a row with
//                          src[r] < 0 is a gap: every header word is interp_word between the records in rows lo_row[r] < r < hi_row[r], bytes 5-8 are
//                          r + 1 and the samples are zero bytes.  The output is cut into units of W = 16, 4 or 1 bytes (the widest that divides reclen
//                          and both base addresses) and numbered flat over all rows, so short records fill a workgroup as well as long ones; a thread
//                          owns UNITS units a workgroup's width apart and issues their loads before the first store.  A unit of a gap header is built
//                          halfword by halfword: every header word starts at an even byte, so a halfword belongs to one word.
// Row and record numbers are ints; everything multiplied by a record length is size_t (nout * reclen may pass 4 GiB).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "p3d.h"
#include "p3d_host.hpp"
#include "p3d_merge_words.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int WAVE = 64;
constexpr int BS = 256;
constexpr int UNITS = 4;
constexpr int HDR_BYTES = p3d_merge::HDR_BYTES;
constexpr int HDR_DWORDS = HDR_BYTES / 4;
constexpr int MAX_RECLEN = HDR_BYTES + 4 * 65535;

__device__ inline uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(BS) merge_keys_kernel(const unsigned char* __restrict__ rec, int n, size_t reclen, int* __restrict__ tracl,
                                                        uint64_t* __restrict__ fp_full, uint64_t* __restrict__ fp_sub)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long k = (long long)blockIdx.x * (BS / WAVE) + threadIdx.x / WAVE;
    if (k >= n) return;                                            // wave-uniform
    const unsigned char* h = rec + (size_t)k * reclen;
    uint32_t d = 0;
    uint64_t term = 0;
    if (lane < HDR_DWORDS) {
        if constexpr (ALIGNED) {
            d = reinterpret_cast<const uint32_t*>(h)[lane];
        } else {
            const unsigned char* p = h + 4 * lane;
            d = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        term = splitmix64(((uint64_t)(lane + 1) << 32) | d);
    }
    uint64_t full = term;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) full ^= __shfl_xor(full, s);
    const uint64_t term1 = __shfl(term, 1);
    if (lane == 0) {
        tracl[k] = (int)__builtin_bswap32(d);
        fp_full[k] = full;
        fp_sub[k] = full ^ term1;
    }
}

// halfword of a gap header at even byte `i`, as it lies in memory (the byte at the lower address in the low bits)
__device__ inline uint32_t gap_halfword(const unsigned char* __restrict__ ha, const unsigned char* __restrict__ hb, int a, int b, int r, int i)
{
    int off, width;
    p3d_merge::word_of_byte(i, off, width);
    const uint32_t v = (uint32_t)p3d_merge::interp_word(p3d_merge::load_be(ha + off, width), p3d_merge::load_be(hb + off, width), a, b, r);
    const uint32_t be = (v >> (8 * (width - 2 - (i - off)))) & 0xFFFFu;   // the two bytes at i, i + 1 as a big-endian number
    return ((be >> 8) | (be << 8)) & 0xFFFFu;
}

// the little-endian dword of a gap header at byte i (a multiple of 4)
__device__ inline uint32_t gap_dword(const unsigned char* __restrict__ ha, const unsigned char* __restrict__ hb, int a, int b, int r, int i)
{
    if (i == 4) return __builtin_bswap32((uint32_t)(r + 1));
    return gap_halfword(ha, hb, a, b, r, i) | (gap_halfword(ha, hb, a, b, r, i + 2) << 16);
}

template <int W>
struct Unit;
template <>
struct Unit<16> {
    using type = uint4;
};
template <>
struct Unit<4> {
    using type = uint32_t;
};
template <>
struct Unit<1> {
    using type = unsigned char;
};

template <int W>
__global__ void __launch_bounds__(BS) merge_records_kernel(const unsigned char* __restrict__ in, size_t reclen, unsigned units_per_rec, size_t total,
                                                           bool small, const int* __restrict__ src, const int* __restrict__ lo_row,
                                                           const int* __restrict__ hi_row, unsigned char* __restrict__ out)
{
    using T = typename Unit<W>::type;
    const size_t base = (size_t)blockIdx.x * (BS * UNITS) + threadIdx.x;
    T v[UNITS];
    int row[UNITS], u[UNITS], s[UNITS];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const size_t i = base + (size_t)k * BS;
        v[k] = T{};
        s[k] = -1;
        row[k] = -1;
        u[k] = 0;
        if (i >= total) continue;
        if (small) {                                               // fewer than 2^32 units: divide in 32 bits
            const uint32_t q = (uint32_t)i / units_per_rec;
            row[k] = (int)q;
            u[k] = (int)((uint32_t)i - q * units_per_rec);
        } else {
            const size_t q = i / units_per_rec;
            row[k] = (int)q;
            u[k] = (int)(i - q * units_per_rec);
        }
        s[k] = src[row[k]];
        if (s[k] >= 0) v[k] = *reinterpret_cast<const T*>(in + (size_t)s[k] * reclen + (size_t)u[k] * W);
    }
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        if (row[k] < 0) continue;
        const int r = row[k], byte = u[k] * W;                     // byte < HDR_BYTES wherever it is used as an int
        T w = v[k];
        if (s[k] >= 0) {
            if constexpr (W == 16) {
                if (u[k] == 0) w.y = __builtin_bswap32((uint32_t)(r + 1));
            } else if constexpr (W == 4) {
                if (u[k] == 1) w = __builtin_bswap32((uint32_t)(r + 1));
            } else {
                if (u[k] >= 4 && u[k] < 8) w = (unsigned char)((uint32_t)(r + 1) >> (8 * (7 - u[k])));
            }
        } else if ((unsigned)u[k] < (unsigned)(HDR_BYTES / W)) {   // a gap's header; the units behind it stay zero
            const int a = lo_row[r], b = hi_row[r];
            const unsigned char* ha = in + (size_t)src[a] * reclen;
            const unsigned char* hb = in + (size_t)src[b] * reclen;
            if constexpr (W == 16) {
                uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
                // One dword at a time: four double divisions in flight would cost registers.  With the loop rolled, `d[j] = x` would index the
                // array by a run-time value and the compiler would put it into scratch memory; the selects below keep every element in a register.
                for (int j = 0; j < 4; ++j) {
                    const uint32_t x = gap_dword(ha, hb, a, b, r, byte + 4 * j);
                    d[0] = j == 0 ? x : d[0];
                    d[1] = j == 1 ? x : d[1];
                    d[2] = j == 2 ? x : d[2];
                    d[3] = j == 3 ? x : d[3];
                }
                w = make_uint4(d[0], d[1], d[2], d[3]);
            } else if constexpr (W == 4) {
                w = gap_dword(ha, hb, a, b, r, byte);
            } else {
                const uint32_t d = gap_dword(ha, hb, a, b, r, byte & ~3);
                w = (unsigned char)(d >> (8 * (byte & 3)));
            }
        }
        *reinterpret_cast<T*>(out + (size_t)r * reclen + (size_t)u[k] * W) = w;
    }
}

int check_keys(int n, int reclen)
{
    if (n < 0) return fail(P3D_ERR_INVALID, "%d records", n);
    if (reclen < HDR_BYTES || reclen > MAX_RECLEN)
        return fail(P3D_ERR_INVALID, "records of %d bytes: a 240-byte header and at most 65535 samples of 4 bytes (240 ... %d)", reclen, MAX_RECLEN);
    return P3D_OK;
}

// every entry of the plan, before anything is launched
int check_plan(int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row)
{
    if (int rc = check_keys(nsrc, reclen)) return rc;
    if (nsrc < 1 || nout < 1) return fail(P3D_ERR_INVALID, "%d input records, %d output rows", nsrc, nout);
    if (!src || !lo_row || !hi_row) return fail(P3D_ERR_INVALID, "NULL plan");
    for (int r = 0; r < nout; ++r)
        if (src[r] < -1 || src[r] >= nsrc) return fail(P3D_ERR_INVALID, "row %d: source record %d outside -1 ... %d", r, src[r], nsrc - 1);
    if (src[0] < 0 || src[nout - 1] < 0) return fail(P3D_ERR_INVALID, "the first and the last output row cannot be gaps");
    for (int r = 0; r < nout; ++r) {
        if (src[r] >= 0) continue;
        const int a = lo_row[r], b = hi_row[r];
        if (!(a >= 0 && a < r && r < b && b < nout)) return fail(P3D_ERR_INVALID, "gap row %d: neighbours %d and %d do not enclose it inside 0 ... %d", r, a, b, nout - 1);
        if (src[a] < 0 || src[b] < 0) return fail(P3D_ERR_INVALID, "gap row %d: neighbour rows %d and %d must hold records", r, a, b);
    }
    return P3D_OK;
}

int run_keys(const unsigned char* rec, int n, int reclen, int* tracl, uint64_t* fp_full, uint64_t* fp_sub)
{
    if (!rec || !tracl || !fp_full || !fp_sub) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (((uintptr_t)tracl & 3) || (((uintptr_t)fp_full | (uintptr_t)fp_sub) & 7)) return fail(P3D_ERR_INVALID, "misaligned key buffers");
    const unsigned blocks = (unsigned)(((long long)n + BS / WAVE - 1) / (BS / WAVE));
    if ((((uintptr_t)rec | (uintptr_t)reclen) & 3) == 0) {
        merge_keys_kernel<true><<<blocks, BS, 0, 0>>>(rec, n, (size_t)reclen, tracl, fp_full, fp_sub);
    } else {
        merge_keys_kernel<false><<<blocks, BS, 0, 0>>>(rec, n, (size_t)reclen, tracl, fp_full, fp_sub);
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

template <int W>
int launch_records(const unsigned char* in, int reclen, int nout, const int* plan_dev, unsigned char* out)
{
    const unsigned units_per_rec = (unsigned)(reclen / W);
    const size_t total = (size_t)nout * units_per_rec, per_block = (size_t)BS * UNITS, blocks = (total + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "group too large for one launch (%zu workgroups)", blocks);
    merge_records_kernel<W><<<(unsigned)blocks, BS, 0, 0>>>(in, (size_t)reclen, units_per_rec, total, total < (1ull << 32), plan_dev, plan_dev + nout,
                                                           plan_dev + 2 * (size_t)nout, out);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

// the records on the DEVICE, the (checked) plan on the HOST; synchronises, since the plan's device copy is freed on return
int run_records(const unsigned char* in, int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row, unsigned char* out)
{
    if (!in || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    const size_t nin = (size_t)nsrc * reclen, nob = (size_t)nout * reclen;
    if (in < out + nob && out < in + nin) return fail(P3D_ERR_INVALID, "the merged records must not overlap the input records");
    std::vector<int> plan(3 * (size_t)nout);
    for (int r = 0; r < nout; ++r) {
        plan[r] = src[r];
        plan[(size_t)nout + r] = src[r] < 0 ? lo_row[r] : r;       // rows that hold a record never read their neighbours
        plan[2 * (size_t)nout + r] = src[r] < 0 ? hi_row[r] : r;
    }
    DevBuf dplan;
    P3D_TRY(hipMalloc(&dplan.p, plan.size() * sizeof(int)));
    P3D_TRY(hipMemcpy(dplan.p, plan.data(), plan.size() * sizeof(int), hipMemcpyHostToDevice));
    const uintptr_t align = (uintptr_t)in | (uintptr_t)out | (uintptr_t)reclen;
    int rc;
    if ((align & 15) == 0) {
        rc = launch_records<16>(in, reclen, nout, (const int*)dplan.p, out);
    } else if ((align & 3) == 0) {
        rc = launch_records<4>(in, reclen, nout, (const int*)dplan.p, out);
    } else {
        rc = launch_records<1>(in, reclen, nout, (const int*)dplan.p, out);
    }
    if (rc) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_merge_keys_dev(int device, const unsigned char* records_dev, int n, int reclen, int* tracl_dev, uint64_t* fp_full_dev, uint64_t* fp_sub_dev)
{
    if (int rc = check_keys(n, reclen)) return rc;
    if (n == 0) return P3D_OK;
    if (int rc = use_device(device)) return rc;
    if (int rc = run_keys(records_dev, n, reclen, tracl_dev, fp_full_dev, fp_sub_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_merge_keys(int device, const unsigned char* records, int n, int reclen, int* tracl, uint64_t* fp_full, uint64_t* fp_sub)
{
    if (int rc = check_keys(n, reclen)) return rc;
    if (n == 0) return P3D_OK;
    if (!records || !tracl || !fp_full || !fp_sub) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nin = (size_t)n * reclen;
    DevBuf drec, dtracl, dfull, dsub;
    P3D_TRY(hipMalloc(&drec.p, nin));
    P3D_TRY(hipMalloc(&dtracl.p, (size_t)n * sizeof(int)));
    P3D_TRY(hipMalloc(&dfull.p, (size_t)n * sizeof(uint64_t)));
    P3D_TRY(hipMalloc(&dsub.p, (size_t)n * sizeof(uint64_t)));
    P3D_TRY(hipMemcpy(drec.p, records, nin, hipMemcpyHostToDevice));
    if (int rc = run_keys((const unsigned char*)drec.p, n, reclen, (int*)dtracl.p, (uint64_t*)dfull.p, (uint64_t*)dsub.p)) return rc;
    P3D_TRY(hipMemcpy(tracl, dtracl.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(fp_full, dfull.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(fp_sub, dsub.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_merge_records_dev(int device, const unsigned char* records_dev, int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row,
                          unsigned char* out_dev)
{
    if (int rc = check_plan(nsrc, reclen, nout, src, lo_row, hi_row)) return rc;
    if (int rc = use_device(device)) return rc;
    return run_records(records_dev, nsrc, reclen, nout, src, lo_row, hi_row, out_dev);
}

int p3d_merge_records(int device, const unsigned char* records, int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row,
                      unsigned char* out)
{
    if (int rc = check_plan(nsrc, reclen, nout, src, lo_row, hi_row)) return rc;
    if (!records || !out) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nin = (size_t)nsrc * reclen, nob = (size_t)nout * reclen;
    DevBuf din, dout;
    P3D_TRY(hipMalloc(&din.p, nin));
    P3D_TRY(hipMalloc(&dout.p, nob));
    P3D_TRY(hipMemcpy(din.p, records, nin, hipMemcpyHostToDevice));
    if (int rc = run_records((const unsigned char*)din.p, nsrc, reclen, nout, src, lo_row, hi_row, (unsigned char*)dout.p)) return rc;
    P3D_TRY(hipMemcpy(out, dout.p, nob, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
