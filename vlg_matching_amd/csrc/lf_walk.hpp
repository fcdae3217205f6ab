// The LF step as a policy: LF(i) = C[c] + rank_c(i) with c = bwt[i] read on the way (suffix_array_helper.hpp:336-349), on the byte
// index's Huffman-shaped tree (ByteWalk: inverse_select of wt_pc.hpp:385-402), on that tree's quad image (QuadWalk: two levels per
// read, quad_code.hpp; the locate family only) and on the integer index's wavelet matrix (IntWalk: wt_int.hpp:405-430 restated on the
// matrix, int_index.hpp).  Every kernel that walks LF -- the locate family (sweep_kernels.hpp), the unsampling and ISA-sample walks,
// text access (extract.hpp) -- takes one of them; a walk is written here and nowhere else.
//   View, Lds, stage(lds, view)   what the walk reads, its LDS block, and how a workgroup fills it (ends with a barrier)
//   n(), sigma(), degenerate()    degenerate: only the sentinel exists (n = 1), there is nothing to walk and LF(0) = 0
//   lf(i, c, n_lv)                one whole step: LF(i), c = the compact symbol read, n_lv += binary tree levels (super-blocks of the binary walk)
//   lf(i, c)                      the same for text access: no count, and the degenerate index answered
//   Cursor, level(k, i, c, n_lv)  the step one super-block read at a time, for the kernels whose lanes refill: i is the SA index while
//                                 k.at_root(); a call that returns true has finished a step -- i = LF(i), c = the symbol, k at the root
//   sym(c)                        the original symbol of compact symbol c (comp2char)
#pragma once
#include <type_traits>
#include "device_rank.hpp"
#include "quad_code.hpp"

namespace vlg {

// kWide: node-relative positions need more than 32 bits (n > 2^32, or VLG_FORCE_POS64); otherwise a whole step stays in 32-bit arithmetic
template <class BV, bool kWide>
struct ByteWalk {
    using View = IndexView;
    using Lds = WalkLds<BV>;
    static constexpr bool kPlainTree = std::is_same<BV, PlainBV>::value;      // (sweep_first_pair reads the tree's blocks itself)
    static constexpr bool kStageLists = true;                // round 0 of the sweep keeps its lists in LDS (sweep_kernels.hpp: ListStage)
    const IndexView& iv;
    const WalkLds<BV>& s;
    const uint8_t* c2c = nullptr;                            // comp2char in LDS (extract only)
    static __device__ __forceinline__ void stage(Lds& s, const View& iv) { stage_walk(s, iv); }
    __device__ __forceinline__ uint64_t n() const { return iv.n; }
    __device__ __forceinline__ uint32_t sigma() const { return iv.sigma; }
    __device__ __forceinline__ bool degenerate() const { return iv.sigma == 1; }

    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c, uint32_t& n_lv) const
    {
        using walk_t = typename std::conditional<kWide, uint64_t, uint32_t>::type;      // node-relative positions: < n
        uint32_t v = 0;
        walk_t pos = (walk_t)i;
        for (;;) {                                           // inverse_select: wt_pc.hpp:385-402
            const DNode nd = s.nodes[v];
            uint32_t bit;
            walk_t r1;
            BV::rank_bit(iv, s.sh, nd.base, pos, r1, bit);
            ++n_lv;
            pos = bit ? r1 : pos - r1;
            const uint32_t ch = bit ? nd.child[1] : nd.child[0];      // (a select, not an indexed read: the node stays in registers)
            if (ch & kLeafFlag) { c = ch & ~kLeafFlag; break; }
            v = ch;
        }
        return s.C[c] + (uint64_t)pos;                       // LF: suffix_array_helper.hpp:341-348
    }
    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c) const
    {
        if (degenerate()) { c = 0; return 0; }
        uint32_t n_lv = 0;
        return lf(i, c, n_lv);
    }

    struct Cursor {
        uint32_t node = 0;
        __device__ __forceinline__ bool at_root() const { return node == 0; }
    };
    // one level of inverse_select: the bit and the rank come from the same block
    __device__ __forceinline__ bool level(Cursor& k, uint64_t& i, uint32_t& c, uint32_t& n_lv) const
    {
        const DNode nd = s.nodes[k.node];
        uint32_t bit;
        uint64_t r1;
        BV::rank_bit(iv, s.sh, nd.base, i, r1, bit);
        ++n_lv;
        const uint64_t ni = bit ? r1 : i - r1;
        const uint32_t ch = bit ? nd.child[1] : nd.child[0];
        if (ch & kLeafFlag) {                                // reached the symbol: LF = C[c] + rank
            c = ch & ~kLeafFlag;
            i = s.C[c] + ni;
            k.node = 0;
            return true;
        }
        i = ni;
        k.node = ch;
        return false;
    }

    __device__ __forceinline__ uint8_t sym(uint32_t c) const { return c2c[c]; }
};

// The same step on the quad image of the tree (quad_code.hpp): one 32-byte read takes two binary levels -- the digit at the position and
// the equal digits in front of it -- so a symbol of code length len costs ceil(len / 2) dependent reads instead of len.  n_lv still counts
// BINARY levels, as the reference does: a digit adds 2, or 1 where its first bit ends in a leaf (kQuadOne), and a finished step has
// added the symbol's code length.  The quad node table sits in LDS beside C (the same 10 KiB the binary walk stages).
struct QuadLds {
    QNode nodes[kMaxQuadNodes];
    uint64_t C[257];
};
static_assert(kQuadLeaf == kLeafFlag, "a leaf child word reads the same in both node tables");
template <bool kWide>
struct QuadWalk {
    using View = IndexView;
    using Lds = QuadLds;
    using walk_t = typename std::conditional<kWide, uint64_t, uint32_t>::type;      // node-relative positions: < n
    static constexpr bool kPlainTree = false;                // (sweep_first_pair reads binary blocks itself)
    static constexpr bool kStageLists = true;
    const IndexView& iv;
    const QuadLds& s;
    const uint8_t* c2c = nullptr;
    static __device__ __forceinline__ void stage(Lds& s, const View& iv)
    {
        for (uint32_t i = threadIdx.x; i < iv.n_qnodes; i += blockDim.x) s.nodes[i] = iv.qnodes[i];
        for (uint32_t i = threadIdx.x; i <= iv.sigma; i += blockDim.x) s.C[i] = iv.C[i];
        __syncthreads();
    }
    __device__ __forceinline__ uint64_t n() const { return iv.n; }
    __device__ __forceinline__ uint32_t sigma() const { return iv.sigma; }
    __device__ __forceinline__ bool degenerate() const { return iv.sigma == 1; }     // (such an index has no image; kept for the surface)

    // one quad level from position pos of quad node v: -> the child word, pos = the position inside the child
    template <typename P>
    __device__ __forceinline__ uint32_t digit_step(uint32_t v, P& pos, uint32_t& n_lv) const
    {
        const P blk = pos / kQuadDigits;
        const uint32_t off = (uint32_t)(pos - blk * kQuadDigits);
        const uint4* p = reinterpret_cast<const uint4*>(iv.qblocks + ((uint64_t)s.nodes[v].base + blk));
        const uint4 a = p[0], b = p[1];
        uint32_t d;
        pos = quad_rank_digit<P>(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, blk * kQuadDigits, off, d);
        const uint32_t ch = s.nodes[v].child[d];
        n_lv += 2u - ((ch >> 30) & 1u);
        return ch;
    }

    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c, uint32_t& n_lv) const
    {
        uint32_t v = 0;
        walk_t pos = (walk_t)i;
        for (;;) {
            const uint32_t ch = digit_step(v, pos, n_lv);
            if (ch & kQuadLeaf) { c = ch & ~(kQuadLeaf | kQuadOne); break; }
            v = ch;
        }
        return s.C[c] + (uint64_t)pos;                       // LF: suffix_array_helper.hpp:341-348
    }
    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c) const
    {
        if (degenerate()) { c = 0; return 0; }
        uint32_t n_lv = 0;
        return lf(i, c, n_lv);
    }

    struct Cursor {
        uint32_t node = 0;
        __device__ __forceinline__ bool at_root() const { return node == 0; }
    };
    __device__ __forceinline__ bool level(Cursor& k, uint64_t& i, uint32_t& c, uint32_t& n_lv) const
    {
        walk_t pos = (walk_t)i;
        const uint32_t ch = digit_step(k.node, pos, n_lv);
        if (ch & kQuadLeaf) {                                // reached the symbol: LF = C[c] + rank
            c = ch & ~(kQuadLeaf | kQuadOne);
            i = s.C[c] + (uint64_t)pos;
            k.node = 0;
            return true;
        }
        i = pos;
        k.node = ch;
        return false;
    }

    __device__ __forceinline__ uint8_t sym(uint32_t c) const { return c2c[c]; }
};

// what every workgroup that walks the matrix keeps in LDS: the zeros per level and whatever the bit-vector policy needs (BV: PlainBV or
// RrrBV of device_rank.hpp, reading the IntView as they read the byte index's IndexView; level l is "node" l * stride)
template <class BV>
struct IntLds {
    uint64_t Z[kMaxIntLevels];
    typename BV::Shared sh;
};
template <class BV>
__device__ __forceinline__ void stage_int(IntLds<BV>& s, const IntView& v)
{
    if (threadIdx.x < v.n_levels) s.Z[threadIdx.x] = v.Z[threadIdx.x];
    BV::stage(s.sh, v);
    __syncthreads();
}

// A position maps to the next level by  bit ? Z[l] + rank1(p) : p - rank1(p);  the bits read on the way down are the compact symbol,
// and D[c] + (the position in the last arrangement) = C[c] + rank_c(i).
template <class BV>
struct IntWalk {
    using View = IntView;
    using Lds = IntLds<BV>;
    static constexpr bool kPlainTree = false;
    // Round 0 stages its lists on plain levels only.  With the rrr tables in LDS (23 296 B) the 4 104 B of ListStage leave five instead of
    // seven workgroups per CU, and the kernel lives on its waves.  Measured on a word-level text of 2^27 tokens (Zipf over 50 000 words,
    // 10^5 queries x 3 x 2 tokens), locate kernels per batch against the hand-written integer kernels in the same session: staged
    // +0.5 ms (34.1-34.2 against 33.6-33.7), not staged +0.2 ms (34.06-34.10 against 33.86-33.93).  On plain levels (264 -> 4 408 B, no
    // workgroup lost) the shared kernels with staging take 11.5-11.6 ms against 12.3-12.9.
    static constexpr bool kStageLists = std::is_same<BV, PlainBV>::value;
    const IntView& iv;
    const IntLds<BV>& s;
    static __device__ __forceinline__ void stage(Lds& s, const View& iv) { stage_int(s, iv); }
    __device__ __forceinline__ uint64_t n() const { return iv.n; }
    __device__ __forceinline__ uint32_t sigma() const { return (uint32_t)iv.sigma; }
    __device__ __forceinline__ bool degenerate() const { return iv.n_levels == 0; }

    struct Cursor {
        uint32_t lvl = 0, code = 0;
        __device__ __forceinline__ bool at_root() const { return lvl == 0; }
    };
    __device__ __forceinline__ bool level(Cursor& k, uint64_t& i, uint32_t& c, uint32_t& n_lv) const
    {
        uint32_t bit;
        uint64_t r1;
        BV::rank_bit(iv, s.sh, (uint32_t)(k.lvl * iv.stride), i, r1, bit);
        ++n_lv;
        i = bit ? s.Z[k.lvl] + r1 : i - r1;
        k.code = (k.code << 1) | bit;
        if (++k.lvl < iv.n_levels) return false;
        c = k.code;
        i = iv.D[c] + i;                                     // LF: suffix_array_helper.hpp:341-348
        k = Cursor();
        return true;
    }
    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c, uint32_t& n_lv) const
    {
        Cursor k;
        while (!level(k, i, c, n_lv)) {}
        return i;
    }
    __device__ __forceinline__ uint64_t lf(uint64_t i, uint32_t& c) const
    {
        if (degenerate()) { c = 0; return 0; }
        uint32_t n_lv = 0;
        return lf(i, c, n_lv);
    }

    __device__ __forceinline__ uint32_t sym(uint32_t c) const { return iv.comp2char[c]; }      // (sigma up to 2^32: not staged)
};

}  // namespace vlg
