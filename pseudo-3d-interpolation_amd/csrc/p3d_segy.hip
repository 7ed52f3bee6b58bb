// p3d_segy.hip -- steps 9 and 16 of the workflow (the reference's cnv_segy2netcdf.py and cube_cnv_netcdf2segy_3D.py, which leave the work to
// segysak / segyio): coding between big-endian SEG-Y trace records and float32 sections on the device, one pass each way.  A record is a 240-byte
// header followed by ns samples.  The word-level conversions are those of p3d_segy_codec.hpp, bit-identical to functions/segy.py.
//
//   segy_encode_kernel   float32 section -> records of 60 + ns big-endian words.  A workgroup (4 wavefronts) owns a tile of 64 traces x 64 record
//                        words and writes 64 runs of 256 contiguous bytes.  Words 0 ... 59 of a record are the shared template overlaid, byte by
//                        byte, with the per-trace columns (a table of 60 x 4 column numbers and shifts, made on the host, says where each byte
//                        comes from); the words behind them are the samples in format 1 (IBM) or 5 (IEEE).  Trace-major sections [ntr][ns] are read
//                        as they are written, 256 bytes a run.  Slice-major sections [ns][ntr] first go through LDS: the tile is read along ntr (64
//                        rows of 256 bytes), converted, and put down as tile[word][trace] with rows of 65 words, so the write phase's reads along
//                        `word` fall into 64 different banks.  Records start at 16-byte boundaries exactly when ns % 4 == 0: then (WIDE) a lane
//                        owns four consecutive words (16-byte store, 16-byte load from a trace-major section; 60 % 4 == 0, so a quad is all header
//                        or all samples), otherwise one word.
//   segy_decode_kernel   records of formats 1, 2, 3, 5, 8 -> float32 [ntr][ns], a thread per output sample (4-byte loads for the 4-byte formats,
//                        2- and 1-byte loads for formats 3 and 8, whose records are only 2- / 1-byte aligned), or (WIDE: a 4-byte format and
//                        ns % 4 == 0) per four samples with 16-byte loads and stores.  The workgroups behind those of the samples scrape the header
//                        words: a thread per trace reads each of up to 16 words byte by byte and writes words[k][trace].
// Trace and sample numbers are ints, everything multiplied by a record or trace length is 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "p3d.h"
#include "p3d_host.hpp"
#include "p3d_segy_codec.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int BS = 256;
constexpr int WAVE = 64;
constexpr int TILE = 64;
constexpr int HDR_BYTES = 240;
constexpr int HDR_WORDS = HDR_BYTES / 4;
constexpr uint32_t FROM_TEMPLATE = 0xFFu;

// where the four bytes of header word j come from: a column number (or FROM_TEMPLATE) and the right shift of the column's value, a byte each,
// the byte at the lowest address in the low bits
struct HeaderMap {
    uint32_t col[HDR_WORDS], shift[HDR_WORDS];
};

struct FieldTable {
    int n, off[P3D_SEGY_MAX_COLUMNS], width[P3D_SEGY_MAX_COLUMNS], is_signed[P3D_SEGY_MAX_COLUMNS];
};

__device__ inline uint32_t header_word(const HeaderMap& map, const uint32_t* __restrict__ tmpl, const int* __restrict__ values, int ntr, int x, int j)
{
    uint32_t w = tmpl[j];
    const uint32_t col = map.col[j];
    if (col != 0xFFFFFFFFu) {
        const uint32_t shift = map.shift[j];
#pragma unroll
        for (int b = 0; b < 32; b += 8) {
            const uint32_t c = (col >> b) & 0xFFu;
            if (c != FROM_TEMPLATE) {
                const uint32_t v = (uint32_t)values[(long long)c * ntr + x];
                w = (w & ~(0xFFu << b)) | (((v >> ((shift >> b) & 0xFFu)) & 0xFFu) << b);
            }
        }
    }
    return w;
}

// the big-endian sample word of float bits f, as the little-endian word that is stored
__device__ inline uint32_t sample_word(uint32_t f, int fmt) { return p3d_segy::bswap32(fmt == 1 ? p3d_segy::ieee2ibm(f) : f); }

template <int LAYOUT, bool WIDE>
__global__ void __launch_bounds__(BS) segy_encode_kernel(const uint32_t* __restrict__ in, int ntr, int ns, int fmt, const uint32_t* __restrict__ tmpl,
                                                         const int* __restrict__ values, const HeaderMap map, uint32_t* __restrict__ out)
{
    constexpr bool SLICE = LAYOUT == P3D_SEGY_SLICE_MAJOR;
    __shared__ uint32_t tile[SLICE ? TILE : 1][TILE + 1];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int x0 = blockIdx.x * TILE, j0 = blockIdx.y * TILE, nw = HDR_WORDS + ns;

    if constexpr (SLICE) {
        const int x = x0 + lane;
        for (int r = wave; r < TILE; r += BS / WAVE) {
            const int j = j0 + r;
            if (j >= HDR_WORDS && j < nw && x < ntr) tile[r][lane] = sample_word(in[(long long)(j - HDR_WORDS) * ntr + x], fmt);
        }
        __syncthreads();
    }

    if constexpr (WIDE) {                                          // nw % 4 == 0: a quad inside the tile is inside the record
        const int q = 4 * (lane & 15), j = j0 + q;
        for (int t = wave * 4 + (lane >> 4); t < TILE; t += BS / 16) {
            const int x = x0 + t;
            if (x >= ntr || j >= nw) continue;
            uint4 v;
            if (j < HDR_WORDS) {
                v = make_uint4(header_word(map, tmpl, values, ntr, x, j), header_word(map, tmpl, values, ntr, x, j + 1),
                               header_word(map, tmpl, values, ntr, x, j + 2), header_word(map, tmpl, values, ntr, x, j + 3));
            } else if constexpr (SLICE) {
                v = make_uint4(tile[q][t], tile[q + 1][t], tile[q + 2][t], tile[q + 3][t]);
            } else {
                const uint4 s = *reinterpret_cast<const uint4*>(in + (long long)x * ns + (j - HDR_WORDS));
                v = make_uint4(sample_word(s.x, fmt), sample_word(s.y, fmt), sample_word(s.z, fmt), sample_word(s.w, fmt));
            }
            *reinterpret_cast<uint4*>(out + (long long)x * nw + j) = v;
        }
    } else {
        const int j = j0 + lane;
        for (int t = wave; t < TILE; t += BS / WAVE) {
            const int x = x0 + t;
            if (x >= ntr || j >= nw) continue;
            uint32_t w;
            if (j < HDR_WORDS) {
                w = header_word(map, tmpl, values, ntr, x, j);
            } else if constexpr (SLICE) {
                w = tile[lane][t];
            } else {
                w = sample_word(in[(long long)x * ns + (j - HDR_WORDS)], fmt);
            }
            out[(long long)x * nw + j] = w;
        }
    }
}

// flat sample number -> (trace, sample); sections below 2^32 samples divide in 32 bits
__device__ inline void split(long long i, int ns, bool small, long long& x, int& s)
{
    if (small) {
        const uint32_t xi = (uint32_t)i / (uint32_t)ns;
        x = xi;
        s = (int)((uint32_t)i - xi * (uint32_t)ns);
    } else {
        x = i / ns;
        s = (int)(i - x * ns);
    }
}

// the float bits of the 4-byte sample stored as little-endian word w
__device__ inline uint32_t decode_word(uint32_t w, int fmt)
{
    const uint32_t v = p3d_segy::bswap32(w);
    return fmt == 1 ? p3d_segy::ibm2ieee(v) : fmt == 2 ? __float_as_uint((float)(int32_t)v) : v;
}

template <bool WIDE>
__global__ void __launch_bounds__(BS) segy_decode_kernel(const unsigned char* __restrict__ rec, int ntr, int ns, int fmt, int bps, unsigned sample_blocks,
                                                         bool small, const FieldTable fields, uint32_t* __restrict__ out, int* __restrict__ words)
{
    const long long reclen = HDR_BYTES + (long long)ns * bps;
    if (blockIdx.x >= sample_blocks) {                             // the header words: a thread per trace
        const long long x = (long long)(blockIdx.x - sample_blocks) * BS + threadIdx.x;
        if (x >= ntr) return;
        const unsigned char* h = rec + x * reclen;
        for (int k = 0; k < fields.n; ++k) {
            const unsigned char* p = h + fields.off[k];
            uint32_t v = ((uint32_t)p[0] << 8) | p[1];
            if (fields.width[k] == 4) {
                v = (v << 16) | ((uint32_t)p[2] << 8) | p[3];
            } else if (fields.is_signed[k]) {
                v = (uint32_t)(int32_t)(int16_t)v;
            }
            words[(long long)k * ntr + x] = (int)v;
        }
        return;
    }
    const long long total = (long long)ntr * ns;
    long long x;
    int s;
    if constexpr (WIDE) {                                          // 4-byte samples, ns % 4 == 0: quads stay inside a trace and are 16-byte aligned
        const long long i = ((long long)blockIdx.x * BS + threadIdx.x) * 4;
        if (i >= total) return;
        split(i, ns, small, x, s);
        const uint4 w = *reinterpret_cast<const uint4*>(rec + x * reclen + HDR_BYTES + 4 * s);
        *reinterpret_cast<uint4*>(out + i) = make_uint4(decode_word(w.x, fmt), decode_word(w.y, fmt), decode_word(w.z, fmt), decode_word(w.w, fmt));
    } else {
        const long long i = (long long)blockIdx.x * BS + threadIdx.x;
        if (i >= total) return;
        split(i, ns, small, x, s);
        const unsigned char* p = rec + x * reclen + HDR_BYTES + (long long)s * bps;
        uint32_t f;
        if (bps == 4) {
            f = decode_word(*reinterpret_cast<const uint32_t*>(p), fmt);
        } else if (bps == 2) {
            const uint16_t h = *reinterpret_cast<const uint16_t*>(p);
            f = __float_as_uint((float)(int16_t)(uint16_t)((h << 8) | (h >> 8)));
        } else {
            f = __float_as_uint((float)(int8_t)*p);
        }
        out[i] = f;
    }
}

int bytes_per_sample(int fmt) { return fmt == 1 || fmt == 2 || fmt == 5 ? 4 : fmt == 3 ? 2 : fmt == 8 ? 1 : 0; }

int check_shape(int ntr, int ns)
{
    if (ntr < 0) return fail(P3D_ERR_INVALID, "%d traces", ntr);
    if (ns < 1 || ns > 65535) return fail(P3D_ERR_INVALID, "%d samples per trace: the 16-bit sample count of SEG-Y holds 1 ... 65535", ns);
    return P3D_OK;
}

// offset and width of every header word: inside the 240 bytes, 2 or 4 bytes wide, no byte claimed twice
int check_words(const int* desc, int stride, int n, const char* what)
{
    if (n < 0 || n > P3D_SEGY_MAX_COLUMNS) return fail(P3D_ERR_INVALID, "%d %ss (at most %d)", n, what, P3D_SEGY_MAX_COLUMNS);
    if (n && !desc) return fail(P3D_ERR_INVALID, "NULL %s table", what);
    bool used[HDR_BYTES] = {};
    for (int c = 0; c < n; ++c) {
        const int off = desc[c * stride], width = desc[c * stride + 1];
        if (width != 2 && width != 4) return fail(P3D_ERR_INVALID, "%s %d: a width of %d bytes (2 or 4)", what, c, width);
        if (off < 0 || off + width > HDR_BYTES) return fail(P3D_ERR_INVALID, "%s %d: bytes %d ... %d leave the %d-byte trace header", what, c, off, off + width - 1, HDR_BYTES);
        for (int b = off; b < off + width; ++b) {
            if (used[b]) return fail(P3D_ERR_INVALID, "%s %d overlaps another at byte %d", what, c, b);
            used[b] = true;
        }
    }
    return P3D_OK;
}

int check_encode(int ntr, int ns, int layout, int fmt, const int* columns, int ncol, HeaderMap* map)
{
    if (int rc = check_shape(ntr, ns)) return rc;
    if (fmt != 1 && fmt != 5) return fail(P3D_ERR_INVALID, "sample format %d cannot be written (1: IBM, 5: IEEE)", fmt);
    if (layout != P3D_SEGY_TRACE_MAJOR && layout != P3D_SEGY_SLICE_MAJOR) return fail(P3D_ERR_INVALID, "layout %d (0: trace-major, 1: slice-major)", layout);
    if (int rc = check_words(columns, 2, ncol, "column")) return rc;
    for (int j = 0; j < HDR_WORDS; ++j) {
        map->col[j] = 0xFFFFFFFFu;
        map->shift[j] = 0;
    }
    for (int c = 0; c < ncol; ++c) {
        const int off = columns[2 * c], width = columns[2 * c + 1];
        for (int k = 0; k < width; ++k) {                          // byte k of the big-endian word: bits 8 (width - 1 - k) and up of the value
            const int b = off + k, lo = 8 * (b & 3);
            map->col[b >> 2] = (map->col[b >> 2] & ~(0xFFu << lo)) | ((uint32_t)c << lo);
            map->shift[b >> 2] |= (uint32_t)(8 * (width - 1 - k)) << lo;
        }
    }
    return P3D_OK;
}

int check_decode(int ntr, int ns, int fmt, const int* fields, int nf, FieldTable* table)
{
    if (int rc = check_shape(ntr, ns)) return rc;
    if (!bytes_per_sample(fmt)) return fail(P3D_ERR_INVALID, "sample format %d cannot be read (1, 2, 3, 5, 8)", fmt);
    if (int rc = check_words(fields, 3, nf, "header word")) return rc;
    table->n = nf;
    for (int k = 0; k < nf; ++k) {
        table->off[k] = fields[3 * k];
        table->width[k] = fields[3 * k + 1];
        table->is_signed[k] = fields[3 * k + 2] != 0;
    }
    return P3D_OK;
}

template <int LAYOUT>
void launch_encode(bool wide, dim3 grid, const uint32_t* in, int ntr, int ns, int fmt, const uint32_t* tmpl, const int* values, const HeaderMap& map,
                   uint32_t* out)
{
    if (wide) {
        segy_encode_kernel<LAYOUT, true><<<grid, BS, 0, 0>>>(in, ntr, ns, fmt, tmpl, values, map, out);
    } else {
        segy_encode_kernel<LAYOUT, false><<<grid, BS, 0, 0>>>(in, ntr, ns, fmt, tmpl, values, map, out);
    }
}

int encode_dev(const float* section, int ntr, int ns, int layout, int fmt, const unsigned char* tmpl, const HeaderMap& map, int ncol, const int* values,
               unsigned char* records)
{
    if (!section || !tmpl || !records || (ncol && !values)) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (((uintptr_t)section | (uintptr_t)records) & 15) return fail(P3D_ERR_INVALID, "the section and the records must start at 16-byte boundaries");
    if ((uintptr_t)tmpl & 3) return fail(P3D_ERR_INVALID, "the header template must start at a 4-byte boundary");
    const int nw = HDR_WORDS + ns;
    const dim3 grid((unsigned)(((long long)ntr + TILE - 1) / TILE), (unsigned)((nw + TILE - 1) / TILE));
    const bool wide = ns % 4 == 0;
    if (layout == P3D_SEGY_SLICE_MAJOR) {
        launch_encode<P3D_SEGY_SLICE_MAJOR>(wide, grid, (const uint32_t*)section, ntr, ns, fmt, (const uint32_t*)tmpl, values, map, (uint32_t*)records);
    } else {
        launch_encode<P3D_SEGY_TRACE_MAJOR>(wide, grid, (const uint32_t*)section, ntr, ns, fmt, (const uint32_t*)tmpl, values, map, (uint32_t*)records);
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

int decode_dev(const unsigned char* records, int ntr, int ns, int fmt, const FieldTable& table, float* samples, int* words)
{
    if (!records || !samples || (table.n && !words)) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (((uintptr_t)records | (uintptr_t)samples) & 15) return fail(P3D_ERR_INVALID, "the records and the section must start at 16-byte boundaries");
    const int bps = bytes_per_sample(fmt);
    const bool wide = bps == 4 && ns % 4 == 0;
    const long long total = (long long)ntr * ns, per_block = wide ? 4ll * BS : BS;
    const long long sample_blocks = (total + per_block - 1) / per_block, blocks = sample_blocks + (table.n ? ((long long)ntr + BS - 1) / BS : 0);
    if (blocks > 0x7fffffffll) return fail(P3D_ERR_UNSUPPORTED, "section too large for one launch (%lld workgroups)", blocks);
    const bool small = total < (1ll << 32);
    if (wide) {
        segy_decode_kernel<true><<<(unsigned)blocks, BS, 0, 0>>>(records, ntr, ns, fmt, bps, (unsigned)sample_blocks, small, table, (uint32_t*)samples, words);
    } else {
        segy_decode_kernel<false><<<(unsigned)blocks, BS, 0, 0>>>(records, ntr, ns, fmt, bps, (unsigned)sample_blocks, small, table, (uint32_t*)samples, words);
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_segy_encode_dev(int device, const float* section_dev, int ntr, int ns, int layout, int fmt, const unsigned char* template_dev, const int* columns,
                        int ncol, const int* values_dev, unsigned char* records_dev)
{
    HeaderMap map;
    if (int rc = check_encode(ntr, ns, layout, fmt, columns, ncol, &map)) return rc;
    if (ntr == 0) return P3D_OK;
    if (int rc = use_device(device)) return rc;
    if (int rc = encode_dev(section_dev, ntr, ns, layout, fmt, template_dev, map, ncol, values_dev, records_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_segy_encode(int device, const float* section, int ntr, int ns, int layout, int fmt, const unsigned char* tmpl, const int* columns, int ncol,
                    const int* values, unsigned char* records)
{
    HeaderMap map;
    if (int rc = check_encode(ntr, ns, layout, fmt, columns, ncol, &map)) return rc;
    if (ntr == 0) return P3D_OK;
    if (!section || !tmpl || !records || (ncol && !values)) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nin = (size_t)ntr * ns * sizeof(float), nout = (size_t)ntr * (HDR_BYTES + 4 * (size_t)ns), nval = (size_t)ncol * ntr * sizeof(int);
    DevBuf din, dtmpl, dval, dout;
    P3D_TRY(hipMalloc(&din.p, nin));
    P3D_TRY(hipMalloc(&dtmpl.p, HDR_BYTES));
    P3D_TRY(hipMalloc(&dout.p, nout));
    P3D_TRY(hipMemcpy(din.p, section, nin, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dtmpl.p, tmpl, HDR_BYTES, hipMemcpyHostToDevice));
    if (ncol) {
        P3D_TRY(hipMalloc(&dval.p, nval));
        P3D_TRY(hipMemcpy(dval.p, values, nval, hipMemcpyHostToDevice));
    }
    if (int rc = encode_dev((const float*)din.p, ntr, ns, layout, fmt, (const unsigned char*)dtmpl.p, map, ncol, (const int*)dval.p, (unsigned char*)dout.p))
        return rc;
    P3D_TRY(hipMemcpy(records, dout.p, nout, hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_segy_decode_dev(int device, const unsigned char* records_dev, int ntr, int ns, int fmt, const int* fields, int nf, float* samples_dev, int* words_dev)
{
    FieldTable table;
    if (int rc = check_decode(ntr, ns, fmt, fields, nf, &table)) return rc;
    if (ntr == 0) return P3D_OK;
    if (int rc = use_device(device)) return rc;
    if (int rc = decode_dev(records_dev, ntr, ns, fmt, table, samples_dev, words_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_segy_decode(int device, const unsigned char* records, int ntr, int ns, int fmt, const int* fields, int nf, float* samples, int* words)
{
    FieldTable table;
    if (int rc = check_decode(ntr, ns, fmt, fields, nf, &table)) return rc;
    if (ntr == 0) return P3D_OK;
    if (!records || !samples || (nf && !words)) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (int rc = use_device(device)) return rc;
    const size_t nin = (size_t)ntr * (HDR_BYTES + (size_t)ns * bytes_per_sample(fmt)), nout = (size_t)ntr * ns * sizeof(float), nwords = (size_t)nf * ntr * sizeof(int);
    DevBuf din, dout, dwords;
    P3D_TRY(hipMalloc(&din.p, nin));
    P3D_TRY(hipMalloc(&dout.p, nout));
    P3D_TRY(hipMemcpy(din.p, records, nin, hipMemcpyHostToDevice));
    if (nf) P3D_TRY(hipMalloc(&dwords.p, nwords));
    if (int rc = decode_dev((const unsigned char*)din.p, ntr, ns, fmt, table, (float*)dout.p, (int*)dwords.p)) return rc;
    P3D_TRY(hipMemcpy(samples, dout.p, nout, hipMemcpyDeviceToHost));
    if (nf) P3D_TRY(hipMemcpy(words, dwords.p, nwords, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
