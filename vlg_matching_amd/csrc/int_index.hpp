// FM-index of an INTEGER text on the device: csa_wt<wt_int<>, dens, ., sa_order_sa_sampling, ., int_alphabet<>>.
// Internal to search.hip's translation unit; included exactly once, behind wtsa.hpp (whose builder kernels it shares).  The launchers
// at the end pick plain or rrr levels and the sampling through shape_dispatch.hpp, the sweep through bind_sweep (sweep_kernels.hpp).
//   int_alphabet (char2comp / comp2char / C)   include/sdsl/csa_alphabet_strategy.hpp:394-470, 496-536
//   wt_int::rank / inverse_select on the BWT   include/sdsl/wt_int.hpp:370-395, 405-430
//   LF, csa[i], backward_search, locate        suffix_array_helper.hpp:336-349, csa_wt.hpp:335-348, suffix_array_algorithm.hpp:250-326, 604-619
//
// HBM layout (ONE allocation, like the byte index; IntHeader in common.hpp):
//   levels  the BWT as a wavelet MATRIX over the COMPACT symbols (comp = rank of the symbol in the sorted alphabet, the sentinel 0
//           first): level l is one bit-vector of n bits -- bit l (from the top) of every symbol in the arrangement of that level, which is
//           the previous level's stably partitioned by its bit, zeros first -- cut into the 256-bit super-blocks of K1 {224 bits, ones
//           before}.  The reference keeps the raw symbols in a level-wise wt_int whose nodes are intervals: a rank there reads three
//           positions per level (node start, position, node end: wt_int.hpp:381-384).  In the matrix a position maps to the next level
//           by  bit ? Z[l] + rank1(p) : p - rank1(p)  (Z[l] = zeros of level l): ONE super-block read per level for rank and for
//           inverse_select alike, and the answers are the same numbers (divergence of layout only; tests compare rank, LF, csa[i],
//           intervals and tuples with the reference structure restated on the CPU).
//   Z       levels words; D[c] = C[c] - (first position of symbol c in the last arrangement), so that
//           C[c] + rank_c(i) = D[c] + walk(i, c)  and  LF(i) = D[c] + walk(i) with c read off the bits on the way;
//   C       sigma + 1 words; comp2char: sigma symbols ascending (queries are mapped by binary search); samples: SA[0], SA[d], ...
//   marked  (text_order_sa_sampling only, made by vlg_index_resample: csa_sampling_strategy.hpp:127-246) the byte index's marks over the
//           SA indices; samples are then SA[i] / d of the marked i in ascending i
// Limits: symbols are uint32_t, none of them 0 (construct() refuses a 0 symbol: include/sdsl/construct.hpp:36-45); n <= 2^32 / 5
// (the suffix sorter sees five bytes per symbol).
#pragma once
#include "extract.hpp"
#include "select.hpp"
#include "sweep_kernels.hpp"

namespace {

void bind_int_view(vlg_index* idx)
{
    const uint8_t* b = reinterpret_cast<const uint8_t*>(idx->d_blob);
    const IntHeader& h = idx->ihdr;
    IntView& v = idx->iview;
    v.bv_kind = (uint32_t)h.bv_kind; v.sampling = (uint32_t)h.sampling;
    v.blocks = h.bv_kind == kBvPlain ? reinterpret_cast<const Block*>(b + h.off_levels) : nullptr;
    v.rrr_hdr = h.bv_kind == kBvRrr63 ? reinterpret_cast<const uint4*>(b + h.off_rrr_hdr) : nullptr;
    v.rrr_stream = h.bv_kind == kBvRrr63 ? reinterpret_cast<const uint64_t*>(b + h.off_rrr_stream) : nullptr;
    v.rrr_tables = h.bv_kind == kBvRrr63 ? reinterpret_cast<const RrrTables*>(b + h.off_binom) : nullptr;
    v.stride = h.bv_kind == kBvRrr63 ? h.n_sb : h.nb;
    v.Z = reinterpret_cast<const uint64_t*>(b + h.off_Z);
    v.D = reinterpret_cast<const uint64_t*>(b + h.off_D);
    v.C = reinterpret_cast<const uint64_t*>(b + h.off_C);
    v.comp2char = reinterpret_cast<const uint32_t*>(b + h.off_c2c);
    v.samples = reinterpret_cast<const uint32_t*>(b + h.off_samples);
    v.n = h.n; v.nb = h.nb; v.sigma = h.sigma; v.n_samples = h.n_samples; v.n_levels = h.levels; v.dens = h.dens;
    v.marked = h.sampling == kSamplingTextOrder ? reinterpret_cast<const Block*>(b + h.off_marked) : nullptr;
    // what the generic entry points read from the byte header
    BlobHeader& g = idx->hdr;
    memset(&g, 0, sizeof g);
    g.magic = kIntBlobMagic; g.total_bytes = h.total_bytes; g.n = h.n; g.sigma = (uint32_t)std::min<uint64_t>(h.sigma, 0xFFFFFFFFull);
    g.dens = h.dens; g.n_samples = h.n_samples; g.sample_bytes = 4; g.bv_kind = h.bv_kind == kBvRrr63 ? VLG_BV_INT_MATRIX_RRR63 : VLG_BV_INT_MATRIX;
    g.n_blocks = (h.bv_kind == kBvRrr63 ? h.n_sb : h.nb) * h.levels; g.n_rrr_sb = h.n_sb * h.levels; g.rrr_stream_words = h.rrr_words;
    g.max_code_len = h.levels; g.wt_bits = h.n * h.levels;
    g.sampling = (uint32_t)h.sampling; g.off_marked = h.off_marked;
    idx->is_int = true;
}

// int_alphabet::char2comp (csa_alphabet_strategy.hpp:421-437): 0 for a symbol that does not occur
__device__ __forceinline__ uint32_t int_char2comp(const IntView& v, uint32_t sym)
{
    uint64_t lo = 0, hi = v.sigma;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (v.comp2char[mid] < sym) lo = mid + 1; else hi = mid; }
    return lo < v.sigma && v.comp2char[lo] == sym ? (uint32_t)lo : 0u;
}

// position of (the first i symbols' share of) symbol c in the last arrangement: D[c] + this = C[c] + rank_c(i)
template <class BV>
__device__ __forceinline__ uint64_t int_walk(const IntView& v, const IntLds<BV>& s, uint64_t p, uint32_t c, uint32_t& levels)
{
    for (uint32_t l = 0; l < v.n_levels; ++l) {
        const uint64_t r1 = BV::rank(v, s.sh, (uint32_t)(l * v.stride), p);
        ++levels;
        p = ((c >> (v.n_levels - 1 - l)) & 1) ? s.Z[l] + r1 : p - r1;
    }
    return p;
}

// backward_search (suffix_array_algorithm.hpp:250-278, 305-326), one lane per sub-pattern; symbols are the raw uint32_t of the query
template <class BV>
__global__ void __launch_bounds__(256) int_backward_search_kernel(IntView v, const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, uint64_t n_pat,
                                                                  uint64_t* __restrict__ out_l, uint64_t* __restrict__ out_r,
                                                                  unsigned long long* __restrict__ stat_levels)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    uint32_t levels = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pat; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t* pat = reinterpret_cast<const uint32_t*>(blob + off[p]);
        uint64_t m = (off[p + 1] - off[p]) / 4;
        uint64_t l = 0, r = v.n - 1;
        while (m > 0 && r + 1 - l > 0) {
            const uint32_t c = pat[--m];
            const uint32_t cc = int_char2comp(v, c);
            if (cc == 0 && c > 0) { l = 1; r = 0; }                  // :263-265
            else if (l == 0 && r + 1 == v.n) { l = v.C[cc]; r = v.C[cc + 1] - 1; }   // :268-270
            else {
                const uint64_t d = v.D[cc];
                const uint64_t nl = d + int_walk(v, sZ, l, cc, levels);
                r = d + int_walk(v, sZ, r + 1, cc, levels) - 1;
                l = nl;
            }
        }
        out_l[p] = l;
        out_r[p] = r;
    }
    if (stat_levels) {
        unsigned long long t = levels;
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(stat_levels, t);
    }
}

// The locate kernels are the byte index's (sweep_kernels.hpp), walking the matrix through IntWalk (lf_walk.hpp): an LF step reads one
// super-block per matrix level and the symbol's D entry; the symbol read (its compact number, < sigma <= 65534) is the sweep's partition
// key.  The sampling policies are device_rank.hpp's on the IntView, with 4-byte samples.
using IntSaSampling = SaOrderSampling<uint32_t>;
using IntTextSampling = TextOrderSampling<uint32_t>;
template <bool kTextOrder> using IntSampling = typename std::conditional<kTextOrder, IntTextSampling, IntSaSampling>::type;

// wt_int::rank(i, c) on raw symbols (for the primitives test): out = #c in BWT[0, i)
template <class BV>
__global__ void __launch_bounds__(256) int_rank_kernel(IntView v, const uint64_t* __restrict__ pos, const uint32_t* __restrict__ sym, uint64_t* __restrict__ out,
                                                       uint64_t count)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = sym[j];
        const uint32_t cc = int_char2comp(v, c);
        uint32_t lv = 0;
        out[j] = (cc == 0 && c > 0) ? 0 : v.D[cc] + int_walk(v, sZ, pos[j], cc, lv) - v.C[cc];
    }
}

// ---- construction -------------------------------------------------------------------------------------------------------------------
__global__ void int_heads_kernel(const uint32_t* __restrict__ sorted, uint64_t n, uint32_t* __restrict__ head)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) head[j] = (j == 0 || sorted[j] != sorted[j - 1]) ? 1u : 0u;
}
// gid = inclusive scan of the heads: symbol number gid - 1 starts at j (comp 0 is the sentinel, so text symbols get gid)
__global__ void int_alphabet_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ gid, uint64_t n, uint32_t* __restrict__ comp2char,
                                    uint64_t* __restrict__ C)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (j == 0 || sorted[j] != sorted[j - 1]) { comp2char[gid[j]] = sorted[j]; C[gid[j]] = j + 1; }      // one sentinel stands before every symbol
}
// BWT in compact symbols: comp(text[SA[i] - 1]), the sentinel (comp 0) where SA[i] = 0
__global__ void int_bwt_kernel(const uint32_t* __restrict__ text, const uint32_t* __restrict__ sa, uint64_t n, const uint32_t* __restrict__ comp2char,
                               uint64_t sigma, uint32_t* __restrict__ bwt)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = sa[i];
        uint32_t c = 0;
        if (s) {
            const uint32_t sym = text[s - 1];
            uint64_t lo = 1, hi = sigma;
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (comp2char[mid] < sym) lo = mid + 1; else hi = mid; }
            c = (uint32_t)lo;
        }
        bwt[i] = c;
    }
}
__global__ void int_bit_keys_kernel(const uint32_t* __restrict__ vals, uint64_t n, uint32_t bit, uint32_t* __restrict__ keys)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) keys[i] = (vals[i] >> bit) & 1u;
}
// D[c] = C[c] - first position of c in the last arrangement (the walk of position 0 along c's bits)
__global__ void int_D_kernel(IntView v, uint64_t* __restrict__ D)
{
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < v.sigma; c += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t p = 0;                                                // (the index under construction is a plain one)
        for (uint32_t l = 0; l < v.n_levels; ++l) {
            const uint64_t r1 = node_rank1(v.blocks, (uint32_t)(l * v.nb), p);
            p = ((c >> (v.n_levels - 1 - l)) & 1) ? v.Z[l] + r1 : p - r1;
        }
        D[c] = v.C[c] - p;
    }
}
__global__ void int_samples_kernel(const uint32_t* __restrict__ sa, uint64_t n_samples, uint32_t dens, uint32_t* __restrict__ samples)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_samples; j += (uint64_t)gridDim.x * blockDim.x) samples[j] = sa[j * dens];
}
__global__ void int_zero_check_kernel(const uint32_t* __restrict__ text, uint64_t n, uint32_t* __restrict__ flag)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) if (text[j] == 0) *flag = 1;
}

// ---- the reference's level-wise tree <-> the compact BWT (vlg_index_save_sdsl_int / vlg_index_from_int_parts) ----------------------------
// wt_int<> (wt_int.hpp:182-262) keeps L = max_level levels over the ORIGINAL symbols: level l is bit L-1-l of every symbol in the
// arrangement sorted stably by the symbols' top l bits, and a node is the run of one such prefix.  comp2char is ascending, so a node
// starts at C[f], f = the first comp whose symbol has that prefix, and its one-child at C[sp], sp = its first comp whose bit l is 1.
// One LEVEL STEP moves the element at p of level l (R = ones of the level before a position, s = C[f]) to
//     bit ? C[sp] + (R(p) - R(s)) : p - (R(p) - R(s))
// of level l + 1 and makes its node's first comp  bit ? sp : f.  Each lane carries (payload, f): the origin of the element when decoding
// (after the last step f is its compact symbol: bwt[origin] = f), its compact symbol when encoding (the bit is read off comp2char).
// Ranks come from the tree words and an exclusive scan of their popcounts, counted from the level's first word g0 (only differences of
// two ranks inside the level are used, so the bits of neighbouring levels that share a word cancel).  Tree bit offsets are 64-bit.

// per level, for every comp f that starts a node: split[f] = sp and end[f] = the first comp after the node (sigma for the last); shift = L - l
__global__ void int_tree_split_kernel(const uint32_t* __restrict__ c2c, uint64_t sigma, uint32_t shift, uint32_t* __restrict__ split,
                                      uint32_t* __restrict__ end)
{
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= sigma; c += (uint64_t)gridDim.x * blockDim.x) {
        if (c == sigma) { split[c] = end[c] = (uint32_t)sigma; continue; }
        const uint64_t pre = (uint64_t)c2c[c] >> shift;
        if (c > 0 && ((uint64_t)c2c[c - 1] >> shift) == pre) continue;          // not the first comp of its node
        uint64_t lo = c, hi = sigma;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (((uint64_t)c2c[mid] >> (shift - 1)) < 2 * pre + 1) lo = mid + 1; else hi = mid; }
        split[c] = (uint32_t)lo;
        hi = sigma;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (((uint64_t)c2c[mid] >> shift) < pre + 1) lo = mid + 1; else hi = mid; }
        end[c] = (uint32_t)lo;
    }
}
// ones of tree bits [64 g0, q): pre = exclusive scan of the popcounts of words g0, g0 + 1, ...
__device__ __forceinline__ uint64_t int_tree_rank(const uint64_t* __restrict__ tree, const uint32_t* __restrict__ pre, uint64_t g0, uint64_t q)
{
    const uint64_t g = q >> 6;
    const uint32_t o = (uint32_t)(q & 63);
    return pre[g - g0] + (o ? (uint64_t)__popcll(tree[g] & ((1ull << o) - 1)) : 0ull);
}
// decode: popcounts of the words g0 .. g0 + nw - 1 as the file holds them
__global__ void int_tree_pops_kernel(const uint64_t* __restrict__ tree, uint64_t g0, uint64_t nw, uint32_t* __restrict__ pops)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nw; k += (uint64_t)gridDim.x * blockDim.x) pops[k] = (uint32_t)__popcll(tree[g0 + k]);
}
// encode: level l's bits as whole words, one wave per word (64 consecutive tree bits, __ballot), and the popcounts of the words as they
// now stand.  A word the level shares with its neighbours is OR-ed in (the previous level's part is already there, the next one's is not).
__global__ void __launch_bounds__(256) int_tree_emit_kernel(const uint32_t* __restrict__ cur, const uint32_t* __restrict__ c2c, uint64_t base, uint64_t n,
                                                            uint32_t bit, uint64_t g0, uint64_t nw, uint64_t* __restrict__ tree, uint32_t* __restrict__ pops)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < nw; k += waves) {
        const uint64_t g = g0 + k, q = (g << 6) + lane;
        const bool in = q >= base && q < base + n;
        const uint32_t b = in ? (c2c[cur[q - base]] >> bit) & 1u : 0u;
        const uint64_t m = __ballot(b);
        if (lane == 0) {
            uint64_t word = m;
            if ((g << 6) >= base && (g << 6) + 64 <= base + n) tree[g] = m;
            else word |= atomicOr(reinterpret_cast<unsigned long long*>(tree + g), (unsigned long long)m);
            pops[k] = (uint32_t)__popcll(word);
        }
    }
}
// one level step (see above).  Every destination is checked against its child node, so a tree that disagrees with C flags *bad instead
// of writing: with the checks each step is a bijection of [0, n).  kLast (decode): bwt[payload] = the leaf's comp instead of moving on.
template <bool kLast>
__global__ void int_tree_step_kernel(const uint64_t* __restrict__ tree, const uint32_t* __restrict__ pre, uint64_t base, uint64_t g0, uint64_t n,
                                     const uint64_t* __restrict__ C, const uint32_t* __restrict__ split, const uint32_t* __restrict__ end,
                                     const uint32_t* __restrict__ pay, const uint32_t* __restrict__ first, uint32_t* __restrict__ pay_out,
                                     uint32_t* __restrict__ first_out, uint32_t* __restrict__ bad)
{
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = first[p];
        const uint64_t s = C[f], q = base + p;
        if (s > p) { *bad = 1; continue; }
        const uint32_t b = (uint32_t)(tree[q >> 6] >> (q & 63)) & 1u;
        const uint64_t r = int_tree_rank(tree, pre, g0, q) - int_tree_rank(tree, pre, g0, base + s);
        const uint32_t sp = split[f];
        const uint32_t nf = b ? sp : f;
        const uint64_t dst = b ? C[sp] + r : p - r;
        if (dst >= C[b ? end[f] : sp]) { *bad = 1; continue; }
        if (kLast) pay_out[pay[p]] = nf;
        else { pay_out[dst] = pay[p]; first_out[dst] = nf; }
    }
}
// the compact BWT out of the wavelet matrix: one lane per position walks the levels (plain or rrr, the BV policies of device_rank.hpp)
template <class BV>
__global__ void __launch_bounds__(256) int_bwt_extract_kernel(IntView v, uint32_t* __restrict__ bwt)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    const IntWalk<BV> walk{v, sZ};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < v.n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t c;
        (void)walk.lf(i, c);                                           // (the symbol is what is wanted; a degenerate index has only the sentinel, 0)
        bwt[i] = c;
    }
}
__global__ void int_iota_kernel(uint32_t* __restrict__ a, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) a[i] = (uint32_t)i;
}

inline void layout_int(IntHeader& h)
{
    uint64_t off = align_up(sizeof(IntHeader), 256);
    h.off_levels = off;
    if (h.bv_kind == kBvRrr63) {
        h.off_rrr_hdr = off;    off = align_up(off + std::max<uint64_t>((uint64_t)h.levels * h.n_sb, 1) * 32, 256);
        h.off_rrr_stream = off; off = align_up(off + (h.rrr_words + 2) * 8, 256);
        h.off_binom = off;      off = align_up(off + 64 * 64 * 8, 256);
    } else {
        off = align_up(off + (uint64_t)h.levels * h.nb * sizeof(Block), 256);
    }
    h.off_Z = off;       off = align_up(off + (uint64_t)kMaxIntLevels * 8, 256);
    h.off_D = off;       off = align_up(off + h.sigma * 8, 256);
    h.off_C = off;       off = align_up(off + (h.sigma + 1) * 8, 256);
    h.off_c2c = off;     off = align_up(off + h.sigma * 4, 256);
    h.off_samples = off; off = align_up(off + h.n_samples * 4, 256);
    h.off_marked = 0;
    if (h.sampling == kSamplingTextOrder) { h.off_marked = off; off = align_up(off + (h.n / kBlockBits + 1) * sizeof(Block), 256); }
    h.total_bytes = off;
}

// ---- resampling and ISA samples (vlg_index_resample in index.hip, vlg_index_isa_samples in kernels.hip) --------------------------------
// every SA value from the SA-order samples: a lane starts at one sample (j * d, SA[j * d]) and walks LF on the matrix -- (LF(i), SA[i] - 1)
// -- up to the next sampled index, so that every SA index is visited exactly once with its value (index.hip: sa_expand_kernel on the tree).
// (a walk is at most n steps long: a damaged image ends the loop instead of spinning)
template <class BV, class Visit>
__device__ __forceinline__ void int_walk_from_samples(const IntView& v, const IntLds<BV>& sZ, const Visit& visit)
{
    const IntWalk<BV> walk{v, sZ};
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < v.n_samples; j += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t i = j * v.dens, x = v.samples[j];
        for (uint64_t k = 0; k < v.n && i < v.n; ++k) {
            visit(i, x);
            uint32_t c;
            i = walk.lf(i, c);
            x = x ? x - 1 : v.n - 1;
            if (i % v.dens == 0) break;
        }
    }
}
// sa[i] = SA[i] for every i (the resampler's input)
template <class BV>
__global__ void __launch_bounds__(256) int_sa_expand_kernel(IntView v, uint32_t* __restrict__ sa)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    int_walk_from_samples(v, sZ, [&](uint64_t i, uint64_t x) { sa[i] = (uint32_t)x; });
}
// isa_sample[SA[i] / inv_dens] = i for every i with SA[i] % inv_dens == 0 (csa_sampling_strategy.hpp:626-642); n < 2^32: 4-byte samples
template <class BV>
__global__ void __launch_bounds__(256) int_isa_samples_kernel(IntView v, uint32_t inv_dens, uint32_t* __restrict__ out)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    int_walk_from_samples(v, sZ, [&](uint64_t i, uint64_t x) { if (x % inv_dens == 0) out[x / inv_dens] = (uint32_t)i; });
}

// ---- text access (extract.hpp): sdsl::extract and csa.isa[i] on the wavelet matrix ---------------------------------------------------
template <class BV>
__global__ void __launch_bounds__(256) int_extract_kernel(IntView v, ExtractJob job, const uint32_t* __restrict__ isa, uint32_t* __restrict__ out)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    extract_segments(job, isa, out, IntWalk<BV>{v, sZ});
}
template <class BV>
__global__ void __launch_bounds__(256) int_isa_kernel(IntView v, uint32_t d, const uint32_t* __restrict__ isa, const uint64_t* __restrict__ p,
                                                      uint64_t* __restrict__ out, uint64_t count, unsigned long long* __restrict__ bad)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    isa_queries(p, out, count, v.n, d, isa, IntWalk<BV>{v, sZ}, bad);
}

// ---- select (select.hpp): wt_int::select, csa.psi, csa.lf and csa.bwt on the wavelet matrix -----------------------------------------------
// sym non-null: wt_int::select(arg[j], sym[j]) on raw symbols (absent symbol, k = 0 or k past its count: n); sym null: csa.psi[arg[j]]
template <class BV>
__global__ void __launch_bounds__(256) int_select_kernel(IntView v, SelView sv, const uint64_t* __restrict__ arg, const uint32_t* __restrict__ sym,
                                                         uint64_t* __restrict__ out, uint64_t count)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = arg[j];
        uint32_t cc;
        uint64_t k;
        if (sym) {
            const uint32_t c = sym[j];
            cc = int_char2comp(v, c);
            k = a;
            if ((cc == 0 && c > 0) || k == 0 || k > v.C[cc + 1] - v.C[cc]) { out[j] = v.n; continue; }
        } else {
            if (a >= v.n) { out[j] = ~0ull; continue; }
            cc = first_column(v.C, v.sigma, a);
            k = a - v.C[cc] + 1;
        }
        out[j] = v.n_levels ? int_select<BV>(v, sZ, sv, cc, k) : k - 1;      // (only the sentinel: no level)
    }
}
template <class BV>
__global__ void __launch_bounds__(256) int_lf_bwt_kernel(IntView v, const uint64_t* __restrict__ in, uint64_t* __restrict__ out_lf, uint32_t* __restrict__ out_bwt,
                                                         uint64_t count)
{
    __shared__ IntLds<BV> sZ;
    stage_int(sZ, v);
    const IntWalk<BV> walk{v, sZ};
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = in[j];
        uint32_t c = 0;
        const uint64_t r = i < v.n ? walk.lf(i, c) : ~0ull;
        if (out_lf) out_lf[j] = r;
        if (out_bwt) out_bwt[j] = i < v.n ? walk.sym(c) : 0u;
    }
}

}  // namespace

namespace vlg {
void layout_int_blob(IntHeader& h) { layout_int(h); }          // for vlg_index_compress (index.hip)

// a blob whose magic says "integer index": called by vlg_index_attach_blob (index.hip)
vlg_status attach_int_blob(const void* d_blob, uint64_t bytes, vlg_index* idx)
{
    VLG_HIP_TRY(hipMemcpy(&idx->ihdr, d_blob, sizeof(IntHeader), hipMemcpyDeviceToHost));
    const IntHeader& h = idx->ihdr;
    if (h.magic != kIntBlobMagic || h.total_bytes > bytes || h.levels > kMaxIntLevels || h.bv_kind > kBvRrr63)
        return fail(VLG_E_INVALID, "not a VLG integer-index blob");
    if (h.sampling > kSamplingTextOrder || !h.dens || h.n_samples != (h.n + h.dens - 1) / h.dens ||
        (h.sampling == kSamplingTextOrder && (h.off_marked < h.off_samples + h.n_samples * 4 || h.off_marked + (h.n / kBlockBits + 1) * sizeof(Block) > h.total_bytes)))
        return fail(VLG_E_INVALID, "integer-index blob: inconsistent sampling fields");
    idx->d_blob = const_cast<void*>(d_blob);
    idx->owns_blob = false;
    bind_int_view(idx);
    return VLG_OK;
}
}  // namespace vlg

namespace {

// a fresh SA-order integer blob for (n, sigma, dens), every byte zero but the header, its view bound: C, comp2char, the matrix and the
// samples are the caller's to fill (zeroing the whole image also makes the padding between its arrays, and so every blob, deterministic)
vlg_status int_alloc_blob(vlg_index* idx, uint64_t n, uint64_t sigma, uint32_t dens)
{
    IntHeader& h = idx->ihdr;
    memset(&h, 0, sizeof h);
    h.magic = kIntBlobMagic; h.n = n; h.sigma = sigma; h.dens = dens; h.n_samples = (n + dens - 1) / dens; h.nb = n / kBlockBits + 1;
    h.levels = sigma > 1 ? bit_width64(sigma - 1) : 0;
    if (h.levels > kMaxIntLevels || (uint64_t)h.levels * h.nb >= 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "integer index too large for 32-bit block numbers");
    layout_int(h);
    DevBuf blob;
    VLG_HIP_TRY(blob.alloc(h.total_bytes));
    idx->d_blob = blob.take();
    idx->owns_blob = true;
    VLG_HIP_TRY(hipMemset(idx->d_blob, 0, h.total_bytes));
    VLG_HIP_TRY(hipMemcpy(idx->d_blob, &h, sizeof h, hipMemcpyHostToDevice));
    bind_int_view(idx);
    return VLG_OK;
}

// The tail every integer index shares (vlg_index_build_int, vlg_index_from_int_parts): the BWT in compact symbols in d_cur (n words) ->
// the wavelet matrix level by level (wtsa.hpp: wtsa_emit_level), Z and D, in the blob of int_alloc_blob whose C and comp2char are filled.
// d_other, d_ka, d_kb: n-word scratch; tmp: rocPRIM scratch, grown here when the scan or the stable partition needs more than it holds.
vlg_status int_matrix_from_bwt(vlg_index* idx, uint32_t* d_cur, uint32_t* d_other, uint32_t* d_ka, uint32_t* d_kb, DevBuf& tmp)
{
    const IntHeader& h = idx->ihdr;
    const uint64_t n = h.n;
    uint8_t* b = reinterpret_cast<uint8_t*>(idx->d_blob);
    Block* lv = reinterpret_cast<Block*>(b + h.off_levels);
    uint64_t* d_Z = reinterpret_cast<uint64_t*>(b + h.off_Z);
    std::vector<uint64_t> Z(kMaxIntLevels, 0);
    uint32_t* cur = d_cur;
    uint32_t* other = d_other;
    DevBuf d_pops;
    VLG_HIP_TRY(d_pops.alloc((h.nb + 1) * 4));
    for (uint32_t l = 0; l < h.levels; ++l) {
        const uint32_t bit = h.levels - 1 - l;
        if (vlg_status s = wtsa_emit_level(cur, n, bit, lv + (uint64_t)l * h.nb, h.nb, d_pops.as<uint32_t>(), tmp)) return s;
        uint32_t ones = 0;
        VLG_HIP_TRY(hipMemcpy(&ones, d_pops.as<uint32_t>() + h.nb, 4, hipMemcpyDeviceToHost));
        Z[l] = n - ones;
        if (l + 1 < h.levels) {                                    // next arrangement: stable by this bit, zeros first
            hipLaunchKernelGGL(int_bit_keys_kernel, launch_grid(n), dim3(256), 0, nullptr, cur, n, bit, d_ka);
            VLG_HIP_TRY(with_scratch(tmp, [&](void* t, size_t& tb) { return rocprim::radix_sort_pairs(t, tb, d_ka, d_kb, cur, other, n, 0, 1, nullptr); }));
            std::swap(cur, other);
        }
        VLG_HIP_TRY(hipGetLastError());
    }
    VLG_HIP_TRY(hipMemcpy(d_Z, Z.data(), kMaxIntLevels * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(int_D_kernel, launch_grid(h.sigma), dim3(256), 0, nullptr, idx->iview, reinterpret_cast<uint64_t*>(b + h.off_D));
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipDeviceSynchronize());
    return VLG_OK;
}

}  // namespace

extern "C" vlg_status vlg_index_build_int(const uint32_t* h_text, uint64_t n_symbols, uint32_t dens, vlg_index** out)
{
    if (!out || (n_symbols && !h_text)) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available (the VLG library has no CPU fallback)");
    if (!dens) dens = 32;
    if (n_symbols * 5 >= 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "integer text too long for the 32-bit suffix array of this index");
    release_cached_device_memory();
    const uint64_t n = n_symbols + 1;
    IndexPtr idx(new vlg_index());
    DevBuf text, flag, sa, arr_a, arr_b, ka, kb, tmp;
    VLG_HIP_TRY(text.alloc(n_symbols * 4));
    uint32_t* d_text = text.as<uint32_t>();
    if (n_symbols) VLG_HIP_TRY(hipMemcpy(d_text, h_text, n_symbols * 4, hipMemcpyHostToDevice));
    VLG_HIP_TRY(flag.alloc((n_symbols * 5 + 2) * 4));               // the zero check's word now, the flags of symbol_suffix_array after it
    VLG_HIP_TRY(hipMemset(flag.p, 0, 4));
    if (n_symbols) hipLaunchKernelGGL(int_zero_check_kernel, launch_grid(n_symbols), dim3(256), 0, nullptr, d_text, n_symbols, flag.as<uint32_t>());
    uint32_t has_zero = 0;
    VLG_HIP_TRY(hipMemcpy(&has_zero, flag.p, 4, hipMemcpyDeviceToHost));
    if (has_zero) return fail(VLG_E_ZERO_BYTE, "the integer text contains the symbol 0 (reserved for the sentinel: construct.hpp:36-45)");
    // ---- suffix array of the symbols (wtsa.hpp, as vlg_wtsa_build) -----------------------------------------------------------------------
    if (vlg_status s = symbol_suffix_array(d_text, n_symbols, flag, sa)) return s;
    flag.release();
    uint32_t* d_sa = sa.as<uint32_t>();
    // ---- int_alphabet: sorted distinct symbols and their cumulative counts (csa_alphabet_strategy.hpp:496-536) ----------------------
    VLG_HIP_TRY(arr_a.alloc(n * 4));
    VLG_HIP_TRY(arr_b.alloc(n * 4));
    VLG_HIP_TRY(ka.alloc(n * 4));
    VLG_HIP_TRY(kb.alloc(n * 4));
    uint32_t *d_a = arr_a.as<uint32_t>(), *d_b = arr_b.as<uint32_t>(), *d_ka = ka.as<uint32_t>(), *d_kb = kb.as<uint32_t>();
    size_t sort_tb = 0, scan_tb = 0, pair_tb = 0;                   // the largest request of the stages below and of the matrix builder: no stage regrows tmp
    VLG_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_tb, d_a, d_b, n, 0, 32, nullptr));
    VLG_HIP_TRY(rocprim::inclusive_scan(nullptr, scan_tb, d_ka, d_kb, n, rocprim::plus<uint32_t>(), nullptr));
    VLG_HIP_TRY(rocprim::radix_sort_pairs(nullptr, pair_tb, d_ka, d_kb, d_a, d_b, n, 0, 1, nullptr));
    VLG_HIP_TRY(tmp.alloc(std::max(std::max(sort_tb, scan_tb), pair_tb)));
    uint64_t sigma = 1;
    if (n_symbols) {
        VLG_HIP_TRY(with_scratch(tmp, [&](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, d_text, d_b, n_symbols, 0, 32, nullptr); }));       // d_b = sorted text
        hipLaunchKernelGGL(int_heads_kernel, launch_grid(n_symbols), dim3(256), 0, nullptr, d_b, n_symbols, d_ka);
        VLG_HIP_TRY(with_scratch(tmp, [&](void* t, size_t& tb) { return rocprim::inclusive_scan(t, tb, d_ka, d_kb, n_symbols, rocprim::plus<uint32_t>(), nullptr); }));   // d_kb = symbol number (1-based)
        uint32_t distinct = 0;
        VLG_HIP_TRY(hipMemcpy(&distinct, d_kb + (n_symbols - 1), 4, hipMemcpyDeviceToHost));
        sigma = (uint64_t)distinct + 1;
    }
    if (vlg_status s = int_alloc_blob(idx.get(), n, sigma, dens)) return s;
    const IntHeader& h = idx->ihdr;
    uint8_t* b = reinterpret_cast<uint8_t*>(idx->d_blob);
    uint32_t* d_c2c = reinterpret_cast<uint32_t*>(b + h.off_c2c);
    uint64_t* d_C = reinterpret_cast<uint64_t*>(b + h.off_C);
    if (n_symbols) hipLaunchKernelGGL(int_alphabet_kernel, launch_grid(n_symbols), dim3(256), 0, nullptr, d_b, d_kb, n_symbols, d_c2c, d_C);   // comp 0 = the sentinel, C[0] = 0
    VLG_HIP_TRY(hipMemcpy(d_C + sigma, &n, 8, hipMemcpyHostToDevice));
    // ---- BWT in compact symbols, then the wavelet matrix level by level ----------------------------------------------------------------
    hipLaunchKernelGGL(int_bwt_kernel, launch_grid(n), dim3(256), 0, nullptr, d_text, d_sa, n, d_c2c, sigma, d_a);
    VLG_HIP_TRY(hipGetLastError());
    if (vlg_status s = int_matrix_from_bwt(idx.get(), d_a, d_b, d_ka, d_kb, tmp)) return s;
    hipLaunchKernelGGL(int_samples_kernel, launch_grid(h.n_samples), dim3(256), 0, nullptr, d_sa, h.n_samples, dens, reinterpret_cast<uint32_t*>(b + h.off_samples));
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipDeviceSynchronize());
    *out = idx.release();
    return VLG_OK;
}

// int_alphabet of the index (two-phase: null buffers give sigma): C[sigma + 1], comp2char[sigma] (comp 0 = the sentinel)
extern "C" vlg_status vlg_index_export_int_alphabet(const vlg_index* idx, uint64_t* sigma, uint64_t* h_C, uint64_t* h_comp2char)
{
    if (!idx || !sigma) return fail(VLG_E_INVALID, "null argument");
    if (!idx->is_int) return fail(VLG_E_INVALID, "not an integer-alphabet index");
    *sigma = idx->ihdr.sigma;
    if (h_C) VLG_HIP_TRY(hipMemcpy(h_C, idx->iview.C, (idx->ihdr.sigma + 1) * 8, hipMemcpyDeviceToHost));
    if (h_comp2char) {
        std::vector<uint32_t> t(idx->ihdr.sigma);
        VLG_HIP_TRY(hipMemcpy(t.data(), idx->iview.comp2char, idx->ihdr.sigma * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < idx->ihdr.sigma; ++i) h_comp2char[i] = t[i];
    }
    return VLG_OK;
}

// wt_int::rank(i, c) on the BWT of an integer index: out[j] = #sym[j] in BWT[0, i[j])
extern "C" vlg_status vlg_int_rank_batch(const vlg_index* idx, const uint64_t* d_i, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!idx || (count && (!d_i || !d_sym || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!idx->is_int) return fail(VLG_E_INVALID, "not an integer-alphabet index");
    if (!count) return VLG_OK;
    return on_bv(idx->iview.bv_kind, [&](auto bv) {
        return launch(int_rank_kernel<tag_t<decltype(bv)>>, launch_grid(count, 8192), (hipStream_t)stream, idx->iview, d_i, d_sym, d_out, count);
    });
}

namespace vlg {

vlg_status launch_int_backward_search(const IntView& v, const uint8_t* d_blob, const uint64_t* d_off, uint64_t n_pat, uint64_t* d_l, uint64_t* d_r,
                                      unsigned long long* d_stat_levels, hipStream_t st)
{
    if (!n_pat) return VLG_OK;
    return on_bv(v.bv_kind, [&](auto bv) {
        return launch(int_backward_search_kernel<tag_t<decltype(bv)>>, launch_grid(n_pat, 4096), st, v, d_blob, d_off, n_pat, d_l, d_r, d_stat_levels);
    });
}

// the integer index in the sorted sweep (sigma <= 65534: the partition key is 16 bits wide)
vlg_status launch_int_locate_sweep(const IntView& v, const SweepJob<uint32_t>& job)
{
    const bool text_order = shape(v).text_order;
    if (v.dens == 1 && !text_order && job.total)                      // the resident suffix array
        return sweep_dense_copy(job, [&] { return launch_int_dense_copy(v, job.d_l, job.d_out_off, job.n_lists, job.total, job.d_out, job.stream); });
    if (!int_sweep_possible(v)) return fail(VLG_E_INTERNAL, "integer index: not for the sorted sweep");
    return on_bv(v.bv_kind, [&](auto bv) { return on_flag(text_order, [&](auto to) {
        return run_locate_sweep<uint32_t, false>(bind_sweep<IntWalk<tag_t<decltype(bv)>>, IntSampling<decltype(to)::value>, uint32_t, false>(v, job, nullptr), job);
    }); });
}

// SA-order density 1: the samples are the suffix array, and locate copies SA intervals (kernels.hip: sa_dense_copy_kernel)
vlg_status launch_int_dense_copy(const IntView& v, const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, uint32_t* d_out, hipStream_t stream)
{
    if (v.dens != 1 || v.sampling != kSamplingSaOrder) return fail(VLG_E_INTERNAL, "integer index: the copy needs SA-order samples of density 1");
    return launch_sa_dense_copy(v.samples, d_l, d_out_off, n_pat, total, d_out, stream);
}

vlg_status launch_int_locate(const IntView& v, uint32_t* d_io, uint64_t total, unsigned long long* d_stats, hipStream_t st)
{
    if (!total) return VLG_OK;
    const LocateSlices sl = locate_slices(total);
    return on_bv(v.bv_kind, [&](auto bv) { return on_flag(shape(v).text_order, [&](auto to) {
        // (in place: no words, no records -- the tail mode's parameters are empty)
        return launch(locate_kernel<IntWalk<tag_t<decltype(bv)>>, IntSampling<decltype(to)::value>, uint32_t>, dim3(sl.blocks), st, v, d_io, total, sl.per_wave, d_stats,
                      nullptr, 0u, nullptr, 0ull, nullptr);
    }); });
}

// every SA value of an SA-order integer index into d_sa (n words): the input of vlg_index_resample
vlg_status launch_int_sa_expand(const IntView& v, uint32_t* d_sa, hipStream_t st)
{
    if (v.sampling != kSamplingSaOrder) return fail(VLG_E_INTERNAL, "integer index: expanding the suffix array needs SA-order samples");
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_sa_expand_kernel<tag_t<decltype(bv)>>, launch_grid(v.n_samples, 8192), st, v, d_sa); });
}

// isa_sample of an SA-order integer index into d_out ((n - 1) / inv_dens + 1 words): vlg_index_isa_samples
vlg_status launch_int_isa_samples(const IntView& v, uint32_t inv_dens, uint32_t* d_out, hipStream_t st)
{
    if (v.sampling != kSamplingSaOrder || !inv_dens) return fail(VLG_E_INTERNAL, "integer index: ISA samples need SA-order samples");
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_isa_samples_kernel<tag_t<decltype(bv)>>, launch_grid(v.n_samples, 8192), st, v, inv_dens, d_out); });
}

vlg_status launch_int_select(const IntView& v, const SelView& sv, const uint64_t* d_arg, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, hipStream_t st)
{
    if (!count) return VLG_OK;
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_select_kernel<tag_t<decltype(bv)>>, launch_grid(count, 8192), st, v, sv, d_arg, d_sym, d_out, count); });
}
vlg_status launch_int_lf_bwt(const IntView& v, const uint64_t* d_i, uint64_t* d_lf, uint32_t* d_bwt, uint64_t count, hipStream_t st)
{
    if (!count) return VLG_OK;
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_lf_bwt_kernel<tag_t<decltype(bv)>>, launch_grid(count, 8192), st, v, d_i, d_lf, d_bwt, count); });
}
vlg_status launch_int_extract(const IntView& v, const ExtractJob& job, const uint32_t* d_isa, uint32_t* d_out, hipStream_t st)
{
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_extract_kernel<tag_t<decltype(bv)>>, launch_grid(job.n_segs, 8192), st, v, job, d_isa, d_out); });
}

vlg_status launch_int_isa(const IntView& v, uint32_t d, const uint32_t* d_isa, const uint64_t* d_i, uint64_t* d_out, uint64_t count,
                          unsigned long long* d_bad, hipStream_t st)
{
    return on_bv(v.bv_kind, [&](auto bv) { return launch(int_isa_kernel<tag_t<decltype(bv)>>, launch_grid(count, 8192), st, v, d, d_isa, d_i, d_out, count, d_bad); });
}

}  // namespace vlg

// ---- the reference's wt_int<> and the device index (vlg_hip.h: vlg_index_from_int_parts, vlg_index_export_int_tree) ---------------------
namespace {

inline uint32_t int_max_level(uint64_t largest) { return (uint32_t)bit_width64(std::max<uint64_t>(largest, 1)); }   // hi(max(x, 1)) + 1

// device scratch of the level steps: the tree, (payload, first comp) twice, the per-node tables and the popcount scan of one level
struct TreeScratch {
    DevBuf tree, pay[2], first[2], split, end, pops, bad, tmp;
    uint64_t words = 0, max_nw = 0;
    vlg_status alloc(uint64_t n, uint64_t sigma, uint32_t L)
    {
        words = (n * L + 63) / 64;
        max_nw = n / 64 + 2;                                            // words one level of n bits touches
        VLG_HIP_TRY(tree.alloc((words + 1) * 8));
        for (int k = 0; k < 2; ++k) {
            VLG_HIP_TRY(pay[k].alloc(n * 4));
            VLG_HIP_TRY(first[k].alloc(n * 4));
        }
        VLG_HIP_TRY(split.alloc((sigma + 1) * 4));
        VLG_HIP_TRY(end.alloc((sigma + 1) * 4));
        VLG_HIP_TRY(pops.alloc((max_nw + 1) * 4));
        VLG_HIP_TRY(bad.alloc(4));
        VLG_HIP_TRY(hipMemset(bad.p, 0, 4));
        size_t tb = 0;                                                  // the scan's scratch for the widest level, so that no level regrows it
        VLG_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, pops.as<uint32_t>(), pops.as<uint32_t>(), 0u, max_nw, rocprim::plus<uint32_t>(), nullptr));
        VLG_HIP_TRY(tmp.alloc(tb));
        return VLG_OK;
    }
    // exclusive scan of the popcounts of one level's nw words, in place
    vlg_status scan_pops(uint64_t nw)
    {
        uint32_t* p = pops.as<uint32_t>();
        VLG_HIP_TRY(with_scratch(tmp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, p, p, 0u, nw, rocprim::plus<uint32_t>(), nullptr); }));
        return VLG_OK;
    }
};

// level l of the tree: first word g0 and the number of words nw it touches
inline void tree_level_words(uint64_t n, uint32_t l, uint64_t& base, uint64_t& g0, uint64_t& nw)
{
    base = (uint64_t)l * n;
    g0 = base >> 6;
    nw = ((base + n - 1) >> 6) - g0 + 1;
}

// encode: compact BWT in s.pay[0] -> the level-wise tree over comp2char (d_c2c) in s.tree, L levels
vlg_status int_tree_encode(TreeScratch& s, uint64_t n, uint64_t sigma, uint32_t L, const uint32_t* d_c2c, const uint64_t* d_C)
{
    uint64_t* tree = s.tree.as<uint64_t>();
    uint32_t *pops = s.pops.as<uint32_t>(), *split = s.split.as<uint32_t>(), *end = s.end.as<uint32_t>(), *bad_flag = s.bad.as<uint32_t>();
    VLG_HIP_TRY(hipMemset(tree, 0, (s.words + 1) * 8));
    VLG_HIP_TRY(hipMemset(s.first[0].p, 0, n * 4));
    int cur = 0;
    for (uint32_t l = 0; l < L; ++l) {
        uint64_t base, g0, nw;
        tree_level_words(n, l, base, g0, nw);
        // one wave per word: nw * 64 threads, that is four words to a block of 256
        hipLaunchKernelGGL(int_tree_emit_kernel, launch_grid(nw * 64), dim3(256), 0, nullptr, s.pay[cur].as<uint32_t>(), d_c2c, base, n, L - 1 - l, g0, nw, tree, pops);
        if (l + 1 == L) break;                                         // the last level's bits are all the file needs
        if (vlg_status st = s.scan_pops(nw)) return st;
        hipLaunchKernelGGL(int_tree_split_kernel, launch_grid(sigma + 1), dim3(256), 0, nullptr, d_c2c, sigma, L - l, split, end);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(int_tree_step_kernel<false>), launch_grid(n), dim3(256), 0, nullptr, tree, pops, base, g0, n, d_C, split, end,
                           s.pay[cur].as<uint32_t>(), s.first[cur].as<uint32_t>(), s.pay[cur ^ 1].as<uint32_t>(), s.first[cur ^ 1].as<uint32_t>(), bad_flag);
        VLG_HIP_TRY(hipGetLastError());
        cur ^= 1;
    }
    VLG_HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    VLG_HIP_TRY(hipMemcpy(&bad, bad_flag, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(VLG_E_INTERNAL, "integer index: the level-wise tree does not agree with the alphabet");
    return VLG_OK;
}

// decode: the level-wise tree in s.tree -> compact BWT in s.pay[*bwt]; C and comp2char on the device
vlg_status int_tree_decode(TreeScratch& s, uint64_t n, uint64_t sigma, uint32_t L, const uint32_t* d_c2c, const uint64_t* d_C, int* bwt)
{
    const uint64_t* tree = s.tree.as<uint64_t>();
    uint32_t *pops = s.pops.as<uint32_t>(), *split = s.split.as<uint32_t>(), *end = s.end.as<uint32_t>(), *bad_flag = s.bad.as<uint32_t>();
    hipLaunchKernelGGL(int_iota_kernel, launch_grid(n), dim3(256), 0, nullptr, s.pay[0].as<uint32_t>(), n);
    VLG_HIP_TRY(hipMemset(s.first[0].p, 0, n * 4));
    int cur = 0;
    for (uint32_t l = 0; l < L; ++l) {
        uint64_t base, g0, nw;
        tree_level_words(n, l, base, g0, nw);
        hipLaunchKernelGGL(int_tree_pops_kernel, launch_grid(nw), dim3(256), 0, nullptr, tree, g0, nw, pops);
        if (vlg_status st = s.scan_pops(nw)) return st;
        hipLaunchKernelGGL(int_tree_split_kernel, launch_grid(sigma + 1), dim3(256), 0, nullptr, d_c2c, sigma, L - l, split, end);
        if (l + 1 < L)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(int_tree_step_kernel<false>), launch_grid(n), dim3(256), 0, nullptr, tree, pops, base, g0, n, d_C, split, end,
                               s.pay[cur].as<uint32_t>(), s.first[cur].as<uint32_t>(), s.pay[cur ^ 1].as<uint32_t>(), s.first[cur ^ 1].as<uint32_t>(), bad_flag);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(int_tree_step_kernel<true>), launch_grid(n), dim3(256), 0, nullptr, tree, pops, base, g0, n, d_C, split, end,
                               s.pay[cur].as<uint32_t>(), s.first[cur].as<uint32_t>(), s.pay[cur ^ 1].as<uint32_t>(), (uint32_t*)nullptr, bad_flag);
        VLG_HIP_TRY(hipGetLastError());
        uint32_t bad = 0;                                              // a step that flagged left holes: the next one must not read them
        VLG_HIP_TRY(hipMemcpy(&bad, bad_flag, 4, hipMemcpyDeviceToHost));
        if (bad) return fail(VLG_E_INVALID, "wt_int tree does not agree with the alphabet's C (level " + std::to_string(l) + ")");
        cur ^= 1;
    }
    *bwt = cur;
    return VLG_OK;
}

}  // namespace

extern "C" vlg_status vlg_index_export_int_tree(const vlg_index* idx, uint32_t* max_level, uint64_t* h_words)
{
    if (!idx || !max_level) return fail(VLG_E_INVALID, "null argument");
    if (!idx->is_int) return fail(VLG_E_INVALID, "not an integer-alphabet index");
    const IntView& v = idx->iview;
    const uint64_t n = v.n, sigma = v.sigma;
    uint32_t largest = 0;
    VLG_HIP_TRY(hipMemcpy(&largest, v.comp2char + (sigma - 1), 4, hipMemcpyDeviceToHost));
    const uint32_t L = int_max_level(largest);
    *max_level = L;
    if (!h_words) return VLG_OK;
    release_cached_device_memory();
    TreeScratch s;
    if (vlg_status st = s.alloc(n, sigma, L)) return st;
    if (vlg_status st = on_bv(v.bv_kind, [&](auto bv) { return launch(int_bwt_extract_kernel<tag_t<decltype(bv)>>, launch_grid(n), nullptr, v, s.pay[0].as<uint32_t>()); }))
        return st;
    if (vlg_status st = int_tree_encode(s, n, sigma, L, v.comp2char, v.C)) return st;
    VLG_HIP_TRY(hipMemcpy(h_words, s.tree.p, s.words * 8, hipMemcpyDeviceToHost));
    return VLG_OK;
}

extern "C" vlg_status vlg_index_from_int_parts(const vlg_int_index_parts* p, vlg_index** out)
{
    if (!p || !out) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    const uint64_t n = p->n, sigma = p->sigma;
    if (!n || !sigma || sigma > n || !p->C || !p->comp2char || !p->sa_sample_dens || (p->tree_bits && !p->tree_words) || (p->n_samples && !p->sa_samples))
        return fail(VLG_E_INVALID, "integer index parts: missing or empty members");
    if (n > 0xFFFFFFFFull) return fail(VLG_E_UNSUPPORTED, "integer index parts: n >= 2^32 (SA samples and positions are 32-bit)");
    if (p->C[0] != 0 || p->C[sigma] != n || p->comp2char[0] != 0) return fail(VLG_E_INVALID, "integer index parts: C[0] = 0, C[sigma] = n and comp2char[0] = 0 are required");
    for (uint64_t c = 0; c < sigma; ++c) {
        if (p->C[c + 1] <= p->C[c]) return fail(VLG_E_INVALID, "integer index parts: C does not increase");
        if (c && p->comp2char[c] <= p->comp2char[c - 1]) return fail(VLG_E_INVALID, "integer index parts: comp2char does not increase");
    }
    if (p->comp2char[sigma - 1] > 0xFFFFFFFFull) return fail(VLG_E_UNSUPPORTED, "integer index parts: a symbol >= 2^32 (the device index holds uint32_t symbols)");
    const uint32_t L = int_max_level(p->comp2char[sigma - 1]);
    if (p->max_level != L || p->tree_bits != n * L) return fail(VLG_E_INVALID, "integer index parts: max_level or the tree size disagree with the largest symbol");
    if (p->n_samples != (n + p->sa_sample_dens - 1) / p->sa_sample_dens) return fail(VLG_E_INVALID, "integer index parts: SA sample count is not ceil(n / dens)");
    std::vector<uint32_t> c2c(sigma), smp(std::max<uint64_t>(p->n_samples, 1));
    for (uint64_t c = 0; c < sigma; ++c) c2c[c] = (uint32_t)p->comp2char[c];
    for (uint64_t j = 0; j < p->n_samples; ++j) {
        if (p->sa_samples[j] >= n) return fail(VLG_E_INVALID, "integer index parts: an SA sample is not below n");
        smp[j] = (uint32_t)p->sa_samples[j];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available (the VLG library has no CPU fallback)");
    release_cached_device_memory();
    IndexPtr idx(new vlg_index());
    TreeScratch s;
    if (vlg_status st = int_alloc_blob(idx.get(), n, sigma, p->sa_sample_dens)) return st;
    const IntHeader& h = idx->ihdr;
    uint8_t* b = reinterpret_cast<uint8_t*>(idx->d_blob);
    uint32_t* d_c2c = reinterpret_cast<uint32_t*>(b + h.off_c2c);
    uint64_t* d_C = reinterpret_cast<uint64_t*>(b + h.off_C);
    VLG_HIP_TRY(hipMemcpy(d_C, p->C, (sigma + 1) * 8, hipMemcpyHostToDevice));
    VLG_HIP_TRY(hipMemcpy(d_c2c, c2c.data(), sigma * 4, hipMemcpyHostToDevice));
    VLG_HIP_TRY(hipMemcpy(b + h.off_samples, smp.data(), p->n_samples * 4, hipMemcpyHostToDevice));
    if (vlg_status st = s.alloc(n, sigma, L)) return st;
    VLG_HIP_TRY(hipMemset(s.tree.as<uint64_t>() + s.words, 0, 8));
    VLG_HIP_TRY(hipMemcpy(s.tree.p, p->tree_words, s.words * 8, hipMemcpyHostToDevice));
    int bwt = 0;
    if (vlg_status st = int_tree_decode(s, n, sigma, L, d_c2c, d_C, &bwt)) return st;
    // the tree, the tables and the scan go; the four n-word arrays are the matrix builder's scratch
    for (DevBuf* q : {&s.tree, &s.split, &s.end, &s.pops, &s.bad, &s.tmp}) q->release();
    if (vlg_status st = int_matrix_from_bwt(idx.get(), s.pay[bwt].as<uint32_t>(), s.pay[bwt ^ 1].as<uint32_t>(), s.first[0].as<uint32_t>(), s.first[1].as<uint32_t>(), s.tmp))
        return st;
    *out = idx.release();
    return VLG_OK;
}
