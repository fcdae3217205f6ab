// Select on the device (vlg_hip.h: vlg_select_support, vlg_bit_select_batch, vlg_wt_select_batch, vlg_int_select_batch, vlg_psi_batch):
// select_support_mcl<1> / <0> on a bit-vector (include/sdsl/select_support_mcl.hpp:347-400), select_support_rrr (rrr_vector.hpp:638-700),
// wt_pc::select (wt_pc.hpp:415-442), wt_int::select (wt_int.hpp:442-480) and csa.psi[i] (suffix_array_helper.hpp:322-332) on the BWT of
// an index.  A vlg_select_support is a handle beside its source, like vlg_text_access: it owns the hints below and reads the source's
// super-blocks as they are -- no blob changes.  kernels.hip instantiates the bodies on the Huffman-shaped tree and on the stand-alone
// bit-vectors, int_index.hpp on the wavelet matrix.
//
// What the handle keeps in HBM:
//   nodes   one SelNode per bit-vector the source has: the tree's nodes (byte index; leaves unused), the matrix's levels (integer
//           index), or one (a bit-vector).  Sizes come from the symbol counts (C and the tree, n and Z), not from DNode.size_lo.
//   hints   4-byte words.  For node v and each bit value, entry j is the node-relative super-block that holds the node's
//           (j * sample + 1)-th one (zero), j = 0 .. ceil(count / sample) - 1, and one closing entry holds the node's last
//           super-block: ceil(ones / sample) + ceil(zeros / sample) + 2 words per node, size / sample + O(1) -- 1/16 of a plain
//           bit-vector's bytes at sample = 512.  The counts in the super-blocks are node-relative and increase inside a node, so the
//           hints are built in one pass, one lane per super-block: a lane writes every hint whose rank lies in (count before its
//           super-block, count before the next one].  The zeros past a node's last bit (the padding of its last super-block) are not
//           counted -- zeros before super-block b are min(b * bits, size) minus the ones -- so no hint points into them.
//   leaf_up (byte index) for every compact symbol the inner node above its leaf and the bit that leads to it.
//
// One bit-select (device_rank.hpp: PlainBV::select, RrrBV::select) reads two neighbouring hints, finds the super-block between them
// (halving while more than eight are left, then eight independent count reads), and selects inside it (select_code.hpp).  At
// sample = 512 and density 1/2 two hints lie five super-blocks apart: hint, counts, block -- three dependent reads where a rank is one.
// A select on the BWT climbs from the symbol's leaf to the root, one bit-select per level (wt_pc.hpp:429-440): select1 in the parent
// when the node is its right child, select0 otherwise; on the matrix select1 of p - Z[l] + 1 or select0 of p + 1 per level.
#pragma once
#include "common.hpp"
#include "device_rank.hpp"

namespace vlg {

constexpr uint32_t kSelectSampleDefault = 512, kSelectSampleMin = 64, kSelectSampleMax = 1u << 16;
constexpr uint32_t kSelNoParent = 0xFFFFFFFFu;

struct SelNode {
    uint64_t size, ones;          // bits of the node, ones among them
    uint64_t h1, h0;              // first hint of the ones / of the zeros in `hints`
    uint32_t base;                // first super-block (plain) or header (rrr) of the node in the source
    uint32_t nb;                  // super-blocks of the node: size / 224 + 1, or size / 2016 + 1
    uint32_t up;                  // byte index: 2 * parent + (the bit that leads here); kSelNoParent at the root
    uint32_t pad;
};

// what a select kernel receives (by value) beside the source's view
struct SelView {
    const SelNode* nodes;
    const uint32_t* hints;
    const uint32_t* leaf_up;      // byte index: [sigma] 2 * node + bit of the leaf of compact symbol c
    uint32_t shift;               // sample = 1 << shift
    uint32_t n_nodes;
};

__host__ __device__ inline uint64_t select_hint_count(uint64_t bits, uint32_t shift) { return ((bits + (1ull << shift) - 1) >> shift) + 1; }

// what the hint pass reads of super-block b of a node: ones before it
struct PlainCounts {
    const Block* blocks;
    static constexpr uint32_t kBits = kBlockBits;
    __device__ __forceinline__ uint64_t ones_before(uint32_t base, uint32_t b) const { return blocks[(uint64_t)base + b].cnt; }
};
struct RrrCounts {
    const uint4* hdr;
    static constexpr uint32_t kBits = kRrrSuperBits;
    __device__ __forceinline__ uint64_t ones_before(uint32_t base, uint32_t b) const { return hdr[2 * ((uint64_t)base + b)].x; }
};

// The hint pass.  list: the nodes that have a bit-vector, first[q]: super-blocks of list[0 .. q) (n_list + 1 words); global super-block
// g belongs to the last q with first[q] <= g.
template <class Counts>
__device__ __forceinline__ void select_build_hints(const Counts& src, const SelNode* __restrict__ nodes, const uint32_t* __restrict__ list,
                                                   const uint64_t* __restrict__ first, uint32_t n_list, uint32_t shift, uint32_t* __restrict__ hints)
{
    const uint64_t total = first[n_list];
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_list;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (first[mid] <= g) lo = mid; else hi = mid; }
        const SelNode nd = nodes[list[lo]];
        const uint32_t b = (uint32_t)(g - first[lo]);
        const uint64_t one_a = src.ones_before(nd.base, b), one_b = b + 1 < nd.nb ? src.ones_before(nd.base, b + 1) : nd.ones;
        const uint64_t bit_a = (uint64_t)b * Counts::kBits, bit_b = bit_a + Counts::kBits;
        const uint64_t zero_a = (bit_a < nd.size ? bit_a : nd.size) - one_a, zero_b = (bit_b < nd.size ? bit_b : nd.size) - one_b;
        const uint64_t s = 1ull << shift;
        // hint j wants rank j * s + 1 in (a, b]:  j >= ceil(a / s)  and  j * s < b
        // (j stays inside the node's share of `hints` even if the counts of a damaged source disagree with the node's totals)
        const uint64_t last1 = select_hint_count(nd.ones, shift) - 1, last0 = select_hint_count(nd.size - nd.ones, shift) - 1;
        for (uint64_t j = (one_a + s - 1) >> shift; (j << shift) < one_b && j < last1; ++j) hints[nd.h1 + j] = b;
        for (uint64_t j = (zero_a + s - 1) >> shift; (j << shift) < zero_b && j < last0; ++j) hints[nd.h0 + j] = b;
        if (b + 1 == nd.nb) {
            hints[nd.h1 + last1] = b;
            hints[nd.h0 + last0] = b;
        }
    }
}

// select_support_mcl<bit>::select(k) on node 0 of a handle made from a bit-vector; k = 0 or k past the last such bit gives the size
template <class BV, class View>
__device__ __forceinline__ uint64_t bit_select(const View& iv, const typename BV::Shared& sh, const SelView& sv, uint32_t bit, uint64_t k)
{
    const SelNode nd = sv.nodes[0];
    const uint64_t have = bit ? nd.ones : nd.size - nd.ones;
    if (k == 0 || k > have) return nd.size;
    return BV::select(iv, sh, nd.base, sv.hints + (bit ? nd.h1 : nd.h0), sv.shift, bit, k);
}

// wt_pc::select(k, c) for the compact symbol c of a byte index, 1 <= k <= C[c + 1] - C[c]: from the leaf to the root (wt_pc.hpp:429-440)
template <class BV>
__device__ __forceinline__ uint64_t byte_select(const IndexView& iv, const typename BV::Shared& sh, const SelView& sv, uint32_t c, uint64_t k)
{
    if (iv.sigma == 1) return k - 1;                          // (only the sentinel: the tree has no bit-vector)
    uint32_t up = sv.leaf_up[c];
    uint64_t p = k - 1;
    for (uint32_t guard = 0; up != kSelNoParent && guard < kMaxNodes; ++guard) {
        const uint32_t bit = up & 1u;
        const SelNode nd = sv.nodes[up >> 1];
        p = BV::select(iv, sh, nd.base, sv.hints + (bit ? nd.h1 : nd.h0), sv.shift, bit, p + 1);
        up = nd.up;
    }
    return p;
}

// wt_int::select(k, c) for the compact symbol c of an integer index, 1 <= k <= C[c + 1] - C[c], on the wavelet matrix: symbol c starts at
// C[c] - D[c] in the last arrangement; level l maps a position back by select1(p - Z[l] + 1) where bit l of c is set, else select0(p + 1)
template <class BV, class Lds>
__device__ __forceinline__ uint64_t int_select(const IntView& v, const Lds& s, const SelView& sv, uint32_t c, uint64_t k)
{
    uint64_t p = v.C[c] - v.D[c] + k - 1;
    for (uint32_t l = v.n_levels; l-- > 0;) {
        const uint32_t bit = (c >> (v.n_levels - 1 - l)) & 1u;
        const SelNode nd = sv.nodes[l];
        p = BV::select(v, s.sh, nd.base, sv.hints + (bit ? nd.h1 : nd.h0), sv.shift, bit, bit ? p - s.Z[l] + 1 : p + 1);
    }
    return p;
}

// F[i]: the compact symbol c with C[c] <= i < C[c + 1] (i < n = C[sigma])
template <class CArray>
__device__ __forceinline__ uint32_t first_column(const CArray& C, uint64_t sigma, uint64_t i)
{
    uint64_t lo = 0, hi = sigma;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (C[mid] <= i) lo = mid; else hi = mid; }
    return (uint32_t)lo;
}

}  // namespace vlg
