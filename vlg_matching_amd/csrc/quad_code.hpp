// The 4-ary image of the byte index's wavelet tree ("quad image"), written so that a CPU program compiles it too
// (tests/quad_code_check.cpp, tests/quad_tree_check.cpp), like rrr_code.hpp and select_code.hpp.
//
// One quad node per inner node v of the Huffman-shaped tree at EVEN depth.  At position p of v the digit is b1 << 1 | b2:
//   b1 = v's bit at p,  b2 = the bit of child[b1] at rank_{b1}(v, p)  (0 where child[b1] is a leaf: the digit b1 << 1 | 1 never occurs).
// The children of a digit are v's grandchildren, or that leaf; the position inside a child is the number of equal digits before p --
// the number two binary steps give, so C[c] + pos is unchanged.
//
//   quad block   32 bytes, 32-byte aligned: { u32 cnt[3] = digits 0, 1, 2 of THIS NODE before the block, u32 w[5] = 80 digits, digit k in
//                bits 2k, 2k + 1 of w[k / 16] }.  Digit 3's count is (block start) - cnt[0] - cnt[1] - cnt[2].  A node starts on a block
//                boundary and owns size / 80 + 1 blocks: one rank = one aligned 32-byte read, as on the binary image.
//   quad node    { first block, child[4] }: a child word is a quad node id, or kQuadLeaf | comp; kQuadOne is set where the digit spends ONE
//                binary level (its first bit ends in a leaf), so that a walk counts the levels the binary walk counts; kQuadNone for a
//                digit that never occurs.
#pragma once
#include <vector>
#include "rrr_code.hpp"

namespace vlg {

constexpr uint32_t kQuadDigits = 80;
constexpr uint32_t kQuadLeaf = 0x80000000u;                  // (= kLeafFlag of the binary node table)
constexpr uint32_t kQuadOne = 0x40000000u;
constexpr uint32_t kQuadNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxQuadNodes = 256;                      // at most sigma - 1 = 255 inner nodes

struct alignas(32) QuadBlock {
    uint32_t cnt[3];
    uint32_t w[5];
};
struct alignas(16) QNode {                                   // (32 bytes; 16-byte aligned like DNode, so that a std::vector may hold it)
    uint32_t base;
    uint32_t child[4];
    uint32_t pad[3];
};

// 16 digits of a word that equal d, as the low bit of every pair
VLG_HD uint32_t quad_equal_pairs(uint32_t w, uint32_t rep)
{
    const uint32_t x = w ^ rep;                              // a pair of zeros where the digit is d
    return ~(x | (x >> 1)) & 0x55555555u;
}

// The digit at `off` (0 .. 79) of a block and how many digits equal to it the NODE has before it (`start` = the block's first position
// in the node = 80 * its number): the words in front of off's word count whole, off's word below off.
template <typename pos_t>
VLG_HD pos_t quad_rank_digit(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, pos_t start,
                             uint32_t off, uint32_t& digit)
{
    const uint32_t k = off >> 4, sh = (off & 15u) * 2u;
    const uint32_t w01 = k & 1u ? w1 : w0, w23 = k & 1u ? w3 : w2;
    const uint32_t w03 = k & 2u ? w23 : w01;
    const uint32_t word = k & 4u ? w4 : w03;
    const uint32_t d = (word >> sh) & 3u;
    const uint32_t rep = d * 0x55555555u;
    const uint32_t p1 = (uint32_t)__builtin_popcount(quad_equal_pairs(w0, rep)), p2 = p1 + (uint32_t)__builtin_popcount(quad_equal_pairs(w1, rep)),
                   p3 = p2 + (uint32_t)__builtin_popcount(quad_equal_pairs(w2, rep)), p4 = p3 + (uint32_t)__builtin_popcount(quad_equal_pairs(w3, rep));
    const uint32_t q01 = k & 1u ? p1 : 0u, q23 = k & 1u ? p3 : p2;
    const uint32_t q03 = k & 2u ? q23 : q01;
    const uint32_t before = k & 4u ? p4 : q03;
    const uint32_t in_word = (uint32_t)__builtin_popcount(quad_equal_pairs(word, rep) & ((1u << sh) - 1u));
    const uint32_t c01 = d & 1u ? c1 : c0;
    const pos_t in_front = d == 3u ? start - (pos_t)c0 - (pos_t)c1 - (pos_t)c2 : (pos_t)(d & 2u ? c2 : c01);
    digit = d;
    return in_front + (pos_t)(before + in_word);
}

// ---- the collapse of the binary node table (host) ------------------------------------------------------------------------------------
// Node: anything with child[2] in the device layout (DNode: a node id, or kQuadLeaf | comp).  node_size[v]: bits of inner node v;
// leaf_count[comp]: occurrences of the symbol.  -> the quad nodes in BFS order of the binary ids (quad node 0 = the root), the binary
// node each one images, its size, and whether every digit count fits 32 bits (an index where one does not gets no image).
struct QuadPlan {
    std::vector<QNode> nodes;
    std::vector<uint32_t> bin;
    std::vector<uint64_t> size;
    uint64_t n_blocks = 0;
    bool fits = true;
};
template <class Node>
inline bool quad_collapse(const Node* dn, const uint64_t* node_size, uint32_t n_nodes, const uint64_t* leaf_count, QuadPlan& q)
{
    q = QuadPlan();
    if (n_nodes < 3) return false;                           // sigma = 1: nothing to walk
    std::vector<uint32_t> id(n_nodes, kQuadNone);            // binary id -> quad id
    q.bin.push_back(0);
    id[0] = 0;
    for (size_t t = 0; t < q.bin.size(); ++t) {              // (children lie behind their parent: the list grows in BFS order)
        const Node& v = dn[q.bin[t]];
        for (int b1 = 0; b1 < 2; ++b1) {
            if (v.child[b1] & kQuadLeaf) continue;
            if (v.child[b1] >= n_nodes) return false;
            const Node& m = dn[v.child[b1]];
            for (int b2 = 0; b2 < 2; ++b2) {
                const uint32_t g = m.child[b2];
                if (g & kQuadLeaf) continue;
                if (g >= n_nodes || id[g] != kQuadNone || q.bin.size() >= kMaxQuadNodes) return false;
                id[g] = (uint32_t)q.bin.size();
                q.bin.push_back(g);
            }
        }
    }
    auto count_of = [&](uint32_t ch) { return ch & kQuadLeaf ? leaf_count[ch & ~kQuadLeaf] : node_size[ch]; };
    uint64_t blk = 0;
    for (size_t t = 0; t < q.bin.size(); ++t) {
        const Node& v = dn[q.bin[t]];
        QNode qn{};
        if (blk > 0xFFFFFFFFull) q.fits = false;
        qn.base = (uint32_t)blk;
        for (int b1 = 0; b1 < 2; ++b1) {
            const uint32_t m = v.child[b1];
            if (m & kQuadLeaf) {
                qn.child[b1 * 2] = m | kQuadOne;
                qn.child[b1 * 2 + 1] = kQuadNone;
                if (count_of(m) > 0xFFFFFFFFull) q.fits = false;
                continue;
            }
            for (int b2 = 0; b2 < 2; ++b2) {
                const uint32_t g = dn[m].child[b2];
                qn.child[b1 * 2 + b2] = g & kQuadLeaf ? g : id[g];
                if (count_of(g) > 0xFFFFFFFFull) q.fits = false;
            }
        }
        q.nodes.push_back(qn);
        q.size.push_back(node_size[q.bin[t]]);
        blk += node_size[q.bin[t]] / kQuadDigits + 1;
    }
    if (blk > 0xFFFFFFFFull) q.fits = false;
    q.n_blocks = blk;
    return true;
}

}  // namespace vlg
