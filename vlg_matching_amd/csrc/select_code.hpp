// Select inside one block: the last step of every select (select.hpp), written so that a CPU program compiles it too
// (tests/select_code_check.cpp), like the block code of rrr_code.hpp.
//   select32 / select224    the k-th one of a word / of the seven data words of a 256-bit super-block (common.hpp: Block), by popcounts --
//                           what select_support_mcl does inside its last 64-bit word (include/sdsl/select_support_mcl.hpp:347-400,
//                           bits::sel); the k-th zero is the k-th one of the complemented words
//   rrr_select63            the k-th one / zero of the rrr-63 block (class, offset) of an index (rrr_code.hpp: numbered by halves): a
//                           binary search over the position through rrr_dec63, six decodes (rrr_vector.hpp:638-700 walks the block
//                           bit by bit instead)
//   rrr_select63_seq        the same for a block of the stand-alone rrr bit-vector (K6), which keeps the reference's bit-by-bit numbering
//                           (rrr_helper.hpp:411-460): one pass over the bits against the binomial table
// k counts from 1 and must not exceed the number of such bits in the block.
#pragma once
#include "rrr_code.hpp"

namespace vlg {

// position of the k-th one of w, 1 <= k <= popcount(w): five halvings
VLG_HD uint32_t select32(uint32_t w, uint32_t k)
{
    uint32_t pos = 0, c;
    c = (uint32_t)__builtin_popcount(w & 0xFFFFu); if (k > c) { k -= c; w >>= 16; pos += 16; }
    c = (uint32_t)__builtin_popcount(w & 0xFFu);   if (k > c) { k -= c; w >>= 8;  pos += 8; }
    c = (uint32_t)__builtin_popcount(w & 0xFu);    if (k > c) { k -= c; w >>= 4;  pos += 4; }
    c = (uint32_t)__builtin_popcount(w & 0x3u);    if (k > c) { k -= c; w >>= 2;  pos += 2; }
    c = w & 1u;                                    if (k > c) { pos += 1; }
    return pos;
}

// position (0 .. 223) of the k-th one of the 224 bits w0 .. w6, 1 <= k <= their popcount: the running popcounts pick the word with
// comparisons and conditional moves (no indexed register access), select32 finishes
VLG_HD uint32_t select224(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6, uint32_t k)
{
    const uint32_t p1 = (uint32_t)__builtin_popcount(w0), p2 = p1 + (uint32_t)__builtin_popcount(w1), p3 = p2 + (uint32_t)__builtin_popcount(w2),
                   p4 = p3 + (uint32_t)__builtin_popcount(w3), p5 = p4 + (uint32_t)__builtin_popcount(w4), p6 = p5 + (uint32_t)__builtin_popcount(w5);
    uint32_t word = w0, before = 0, at = 0;
    if (k > p1) { word = w1; before = p1; at = 32; }
    if (k > p2) { word = w2; before = p2; at = 64; }
    if (k > p3) { word = w3; before = p3; at = 96; }
    if (k > p4) { word = w4; before = p4; at = 128; }
    if (k > p5) { word = w5; before = p5; at = 160; }
    if (k > p6) { word = w6; before = p6; at = 192; }
    return at + select32(word, k - before);
}

// position (0 .. 62) of the k-th `bit` of the block (cls, o) of rrr_code.hpp, 1 <= k <= (bit ? cls : 63 - cls): the largest position with
// fewer than k such bits in front of it
VLG_HD uint32_t rrr_select63(const RrrTables& t, uint32_t cls, uint64_t o, uint32_t bit, uint32_t k)
{
    uint32_t lo = 0;
    for (uint32_t st = 32; st; st >>= 1) {
        const uint32_t p = lo + st;
        if (p > 62) continue;
        uint32_t b;
        const uint32_t r1 = rrr_dec63(t, cls, o, p, b);
        if ((bit ? r1 : p - r1) < k) lo = p;
    }
    return lo;
}

// the same for (cls, nr) numbered bit by bit as rrr_vector<63> numbers it (binom: C(n, k) at [n * 64 + k], n, k < 64)
VLG_HD uint32_t rrr_select63_seq(const uint64_t* binom, uint32_t cls, uint64_t nr, uint32_t bit, uint32_t k)
{
    uint32_t left = cls, seen = 0;
    for (uint32_t b = 0; b < 63; ++b) {
        uint32_t one = 0;
        if (left) {
            const uint32_t nn = 63 - b;                       // bits not yet decided; the block has `left` ones among them
            if (left == nn) one = 1;
            else { const uint64_t c = binom[(nn - 1) * 64 + left]; if (nr >= c) { nr -= c; one = 1; } }
        }
        left -= one;
        seen += (one == bit);
        if (seen == k) return b;
    }
    return 62;
}

}  // namespace vlg
