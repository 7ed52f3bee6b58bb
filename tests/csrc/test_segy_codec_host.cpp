// Host-only driver of csrc/p3d_segy_codec.hpp: reads 32-bit words from a file and writes, for every word, ieee2ibm(word) and ibm2ieee(word) to
// two files of the same length.  tests/test_segy_codec_host.py compares them with functions/segy.py.
//
//     test_segy_codec_host <words.bin> <encoded.bin> <decoded.bin>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "p3d_segy_codec.hpp"

static bool dump(const char* path, const std::vector<uint32_t>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(uint32_t), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s words.bin encoded.bin decoded.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint32_t> in;
    uint32_t buf[4096];
    for (size_t n; (n = fread(buf, sizeof(uint32_t), 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(f);
    std::vector<uint32_t> enc(in.size()), dec(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
        enc[i] = p3d_segy::ieee2ibm(in[i]);
        dec[i] = p3d_segy::ibm2ieee(in[i]);
    }
    if (!dump(argv[2], enc) || !dump(argv[3], dec)) {
        fprintf(stderr, "cannot write the results\n");
        return 2;
    }
    printf("ALL OK %zu words\n", in.size());
    return 0;
}
