// p3d_resident_dct_index.hpp -- index maps of the single-kernel DCT loop of the windowed jobs (p3d_resident_dct_job.hpp).
// Host and device; no HIP header needed, so a plain C++ program can check it (tests/csrc/test_resident_dct_index_host.cpp).
//
// The iterate of a job lives in the REORDERED order of p3d_dct_tables.hpp on both axes for the whole job: position p of an axis of length N holds
// the natural sample sample_of(N, p), the inverse of dct::perm.  The packed mask words stay in the natural order patch_pack_kernel writes
// (ResidentArgs::bits), so the bit of a held position is looked up through the same map.
//
// The group step owns the N1 x N2 coefficients in N1 N2 / 4 slots of FOUR DISTINCT coefficients {ra, rb} x {ca, cb}.  Per axis of length N, slot
// index s = 1 ... N/2 - 1 is the coupled pair (s, N - s) of the DCT identities; s = 0 takes the two self-paired indices 0 and N/2 together, which a
// slot treats as two groups of one.  (N/2) (N/2) slots of four: every coefficient in exactly one of them.
#pragma once
#include <stdint.h>

#include "p3d_dct_tables.hpp"

namespace p3d {
namespace rdct {

// the natural sample behind reordered position p: dct::perm(n, sample_of(n, p)) == p
P3D_HD int sample_of(int n, int p) { return p < (n + 1) / 2 ? 2 * p : 2 * (n - 1 - p) + 1; }

// mask[i][j] of a window packed as patch_pack_kernel packs it: bit q of word (i, tl) is mask[i][tl + (n2 / 16) q]
P3D_HD unsigned mask_bit(const uint16_t* words, int n2, int i, int j)
{
    const int tpl = n2 / 16;
    return ((unsigned)words[i * tpl + j % tpl] >> (j / tpl)) & 1u;
}

// the 16 bits of the thread that holds row position r and column positions tl + (n2 / 16) q, q = 0 ... 15
P3D_HD unsigned held_bits(const uint16_t* words, int n1, int n2, int r, int tl)
{
    const int i = sample_of(n1, r);
    unsigned w = 0;
    for (int q = 0; q < 16; ++q) w |= mask_bit(words, n2, i, sample_of(n2, tl + (n2 / 16) * q)) << q;
    return w;
}

struct Slot {
    int ra, rb, ca, cb;   // the slot's coefficients are (ra, ca), (ra, cb), (rb, ca), (rb, cb)
    bool pair1, pair2;    // the two rows / columns are a coupled pair (k, N - k); false: the self-paired 0 and N/2
};

// slot g (0 ... 3) of thread tid in a workgroup of n1 n2 / 16 threads: consecutive threads take consecutive columns
P3D_HD Slot slot_of(int n1, int n2, int tid, int g)
{
    const int slot = tid + (n1 * n2 / 16) * g;
    const int s1 = slot / (n2 / 2), s2 = slot % (n2 / 2);
    Slot s;
    s.pair1 = s1 != 0;
    s.pair2 = s2 != 0;
    s.ra = s1;
    s.rb = s1 ? n1 - s1 : n1 / 2;
    s.ca = s2;
    s.cb = s2 ? n2 - s2 : n2 / 2;
    return s;
}

}  // namespace rdct
}  // namespace p3d
