// Host-only driver of csrc/p3d_merge_words.hpp.  tests/test_merge_words_host.py compares what it writes with tests/helpers/merge_numpy.py.
//
//     test_merge_words_host <cases.bin> <interp.bin> <headers.bin> <words.bin> <restored.bin> <tables.bin>
//
// cases.bin     int32 [n][5]: va, vb, a, b, r        -> interp.bin    int32 [n]: interp_word(va, vb, a, b, r)
// headers.bin   uint8 [m][240]                       -> words.bin     int32 [m][91]: load_be of every word_at(j)
//                                                    -> restored.bin  uint8 [m][240]: store_be of those words into a buffer of 0xEE bytes
// tables.bin    int32: 91 x (offset, width) of word_at, then 240 x (offset, width) of word_of_byte
#include <cstdint>
#include <cstdio>
#include <vector>

#include "p3d_merge_words.hpp"

template <class T>
static bool slurp(const char* path, std::vector<T>& v)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    T buf[4096];
    for (size_t n; (n = fread(buf, sizeof(T), 4096, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

template <class T>
static bool dump(const char* path, const std::vector<T>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    using namespace p3d_merge;
    if (argc != 7) {
        fprintf(stderr, "usage: %s cases.bin interp.bin headers.bin words.bin restored.bin tables.bin\n", argv[0]);
        return 2;
    }
    std::vector<int32_t> cases;
    std::vector<unsigned char> headers;
    if (!slurp(argv[1], cases) || !slurp(argv[3], headers) || cases.size() % 5 || headers.size() % HDR_BYTES) {
        fprintf(stderr, "cannot read the input\n");
        return 2;
    }
    const size_t n = cases.size() / 5, m = headers.size() / HDR_BYTES;
    std::vector<int32_t> interp(n), words(m * NWORDS), tables;
    for (size_t i = 0; i < n; ++i) {
        const int32_t* c = &cases[5 * i];
        interp[i] = interp_word(c[0], c[1], c[2], c[3], c[4]);
    }
    std::vector<unsigned char> restored(headers.size(), 0xEE);
    for (size_t x = 0; x < m; ++x)
        for (int j = 0; j < NWORDS; ++j) {
            int off, width;
            word_at(j, off, width);
            if (off < 0 || (width != 2 && width != 4) || off + width > HDR_BYTES) {
                fprintf(stderr, "word %d: offset %d, width %d\n", j, off, width);
                return 1;
            }
            words[x * NWORDS + j] = load_be(&headers[x * HDR_BYTES + off], width);
            store_be(&restored[x * HDR_BYTES + off], width, words[x * NWORDS + j]);
        }
    for (int j = 0; j < NWORDS; ++j) {
        int off, width;
        word_at(j, off, width);
        tables.push_back(off);
        tables.push_back(width);
    }
    for (int i = 0; i < HDR_BYTES; ++i) {
        int off, width;
        word_of_byte(i, off, width);
        tables.push_back(off);
        tables.push_back(width);
    }
    if (!dump(argv[2], interp) || !dump(argv[4], words) || !dump(argv[5], restored) || !dump(argv[6], tables)) {
        fprintf(stderr, "cannot write the results\n");
        return 2;
    }
    printf("ALL OK %zu cases %zu headers\n", n, m);
    return 0;
}
