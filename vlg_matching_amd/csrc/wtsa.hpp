// The paper's index on the device: text + wavelet tree over the suffix array, searched lazily.
// Internal to search.hip's translation unit (results, workspace and timers live there); included exactly once, at its end.
//   vlg_index<alphabet_tag, wt_int<bit_vector_il<>, rank_support_il<>>>   include/sdsl/vlg_index.hpp:109-198 (default tree type :116-119),
//                                       construct :375-392; on disk: wtsa_sdsl.hpp
//   wt_int                              include/sdsl/wt_int.hpp:215-255 (level-wise layout), :339-361 (operator[]), :824-939 (expand / ranges)
//   vlg_iterator                        include/sdsl/vlg_index.hpp:209-373 (relax / next / pull_forward)
//   forward_search                      include/sdsl/suffix_array_algorithm.hpp:48-112
//
// HBM layout: level l of the tree (l = 0: most significant bit of the suffix-array values) is ONE bit-vector of n values, cut into
// the same 256-bit super-blocks as K1 {7 x u32 data, u32 ones before the block inside the level}; the levels follow each other.
// A node is an interval [b, b + size) of its level; its children are the intervals [b, b + zeros) and [b + zeros, b + size) of the
// next level (wt_int.hpp:215-255).  Everything the search needs is two root-to-leaf walks with four rank reads per level:
//   count_less(l, len, x)   how many of SA[l, l + len) are smaller than x
//   quantile(l, len, q)     the q-th smallest of SA[l, l + len)
// so that "the first occurrence of sub-pattern i at or after position p" = quantile(count_less(p)): the sorted occurrence list of a
// sub-pattern is read by rank without ever being located or sorted.  The reference walks the same tree node by node with a cache of
// expanded nodes per sub-pattern (wt_range_walker); on the GPU a lane owns a query, and a batch of 10^5 queries keeps 10^5
// independent walks in flight.
#pragma once
#include "device_rank.hpp"
#include "extract.hpp"

struct vlg_wtsa {
    uint64_t n_text = 0, n_vals = 0;       // symbols; suffix-array entries (n_text + 1)
    uint32_t sym_bytes = 1, levels = 0;
    uint64_t nb = 0;                       // super-blocks per level
    vlg::Block* d_blocks = nullptr;        // [levels][nb]
    void* d_text = nullptr;                // n_text symbols
    uint32_t file_width = 0;               // width of m_text in the file it was loaded from (0: built; wtsa_sdsl.hpp)
    uint64_t* d_level_prefix = nullptr;    // [levels + 1]: ones of the levels before each, all of them last (wtsa_sdsl.hpp)
};

namespace {

struct WtsaView {
    const Block* blocks;
    const void* text;
    uint64_t nb, n_vals, n_text;
    uint32_t levels, sym_bytes;
};

// ---- construction -------------------------------------------------------------------------------------------------------------
// An integer text is sorted as a byte text: every symbol becomes its five base-255 digits + 1, most significant first -- no zero
// byte, codes compare like the numbers, all codes equally long -- so the aligned suffixes of the byte text stand in the order of
// the integer text's suffixes.
__global__ void wtsa_expand_kernel(const uint32_t* __restrict__ syms, uint64_t n, uint8_t* __restrict__ bytes)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v = syms[i];
        uint8_t d[5];
#pragma unroll
        for (int j = 4; j >= 0; --j) { d[j] = (uint8_t)(v % 255u + 1u); v /= 255u; }
#pragma unroll
        for (int j = 0; j < 5; ++j) bytes[5 * i + j] = d[j];
    }
}

// keep the suffixes that start on a symbol: flags, then (after a scan) the compaction
__global__ void wtsa_aligned_flags_kernel(const uint32_t* __restrict__ sa, uint64_t n, uint32_t* __restrict__ flag)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) flag[i] = sa[i] % 5u == 0 ? 1u : 0u;
}
__global__ void wtsa_aligned_compact_kernel(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ pos /* exclusive scan of the flags */,
                                            uint64_t n, uint32_t* __restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (sa[i] % 5u == 0) out[pos[i]] = sa[i] / 5u;
}

// stable-sort keys of a level: the top `bits` bits of every value (the arrangement of level l is the suffix array stably sorted by
// the top l bits: wt_int.hpp:215-255)
__global__ void wtsa_prefix_keys_kernel(const uint32_t* __restrict__ vals, uint64_t n, uint32_t shift, uint32_t* __restrict__ keys)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) keys[i] = vals[i] >> shift;
}

// data words of one level from its arrangement: one thread per 32-bit word; pops[b] += the word's popcount (the counts come from a scan)
__global__ void wtsa_emit_kernel(const uint32_t* __restrict__ vals, uint64_t n, uint32_t bit, Block* __restrict__ blocks, uint64_t nb,
                                 uint32_t* __restrict__ pops)
{
    const uint64_t total = nb * 7;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t blk = g / 7;
        const uint32_t w = (uint32_t)(g % 7);
        const uint64_t first = blk * kBlockBits + 32ull * w;
        uint32_t word = 0;
        if (first < n) {
            const uint32_t m = n - first < 32 ? (uint32_t)(n - first) : 32u;
            for (uint32_t j = 0; j < m; ++j) word |= ((vals[first + j] >> bit) & 1u) << j;
        }
        blocks[blk].w[w] = word;
        if (word) atomicAdd(&pops[blk], (uint32_t)__popc(word));
    }
}
__global__ void wtsa_counts_kernel(Block* __restrict__ blocks, const uint32_t* __restrict__ before, uint64_t nb)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x) blocks[b].cnt = before[b];
}

// An integer text -> the suffix array of its symbols (vlg_wtsa_build, vlg_index_build_int): the text as bytes (above) through the byte
// sorter, then the suffixes that start on a symbol, in order.  d_sa gets the n_symbols + 1 entries, the sentinel's first.  d_flag:
// scratch of 5 n_symbols + 1 words, allocated here (after the sort) unless the caller brings a buffer that large.
vlg_status symbol_suffix_array(const uint32_t* d_text, uint64_t n_symbols, DevBuf& d_flag, DevBuf& d_sa)
{
    if (!n_symbols) {                                               // the sentinel's suffix alone
        VLG_HIP_TRY(d_sa.alloc(4));
        VLG_HIP_TRY(hipMemset(d_sa.p, 0, 4));
        return VLG_OK;
    }
    const uint64_t byte_len = n_symbols * 5, nb5 = byte_len + 1;
    DevBuf d_sa5, d_bytes, d_pos, d_tmp;
    VLG_HIP_TRY(d_sa5.alloc(nb5 * 4));
    VLG_HIP_TRY(d_bytes.alloc(byte_len));
    hipLaunchKernelGGL(wtsa_expand_kernel, launch_grid(n_symbols), dim3(256), 0, nullptr, d_text, n_symbols, d_bytes.as<uint8_t>());
    VLG_HIP_TRY(hipGetLastError());
    if (vlg_status st = vlg_suffix_array_device(d_bytes.as<uint8_t>(), byte_len, d_sa5.as<uint32_t>(), nullptr)) return st;
    d_bytes.release();
    if (d_flag.cap < nb5 * 4) VLG_HIP_TRY(d_flag.alloc(nb5 * 4));
    VLG_HIP_TRY(d_pos.alloc(nb5 * 4));
    VLG_HIP_TRY(d_sa.alloc((n_symbols + 1) * 4));
    hipLaunchKernelGGL(wtsa_aligned_flags_kernel, launch_grid(nb5), dim3(256), 0, nullptr, d_sa5.as<uint32_t>(), nb5, d_flag.as<uint32_t>());
    VLG_HIP_TRY(with_scratch(d_tmp, [&](void* t, size_t& tb) {
        return rocprim::exclusive_scan(t, tb, d_flag.as<uint32_t>(), d_pos.as<uint32_t>(), 0u, nb5, rocprim::plus<uint32_t>(), nullptr);
    }));
    hipLaunchKernelGGL(wtsa_aligned_compact_kernel, launch_grid(nb5), dim3(256), 0, nullptr, d_sa5.as<uint32_t>(), d_pos.as<uint32_t>(), nb5, d_sa.as<uint32_t>());
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipDeviceSynchronize());
    return VLG_OK;
}

// The count words of one level whose blocks hold their data words and whose ones stand in pops[0, nb) (pops[nb] = 0): pops becomes its
// exclusive scan -- pops[nb] the ones of the whole level -- and every block gets the ones before it.  scratch: rocPRIM's, grown on demand.
vlg_status wtsa_level_counts(Block* lb, uint64_t nb, uint32_t* pops, DevBuf& scratch)
{
    VLG_HIP_TRY(with_scratch(scratch, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, pops, pops, 0u, nb + 1, rocprim::plus<uint32_t>(), nullptr); }));
    hipLaunchKernelGGL(wtsa_counts_kernel, launch_grid(nb), dim3(256), 0, nullptr, lb, pops, nb);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}
// One level of a wavelet tree (vlg_wtsa_build) or matrix (int_matrix_from_bwt) from its arrangement: bit `bit` of the n values in cur
// -> the level's blocks, data and count words; pops: nb + 1 words, left as wtsa_level_counts leaves them.
vlg_status wtsa_emit_level(const uint32_t* cur, uint64_t n, uint32_t bit, Block* lb, uint64_t nb, uint32_t* pops, DevBuf& scratch)
{
    VLG_HIP_TRY(hipMemsetAsync(pops, 0, (nb + 1) * 4, nullptr));
    hipLaunchKernelGGL(wtsa_emit_kernel, launch_grid(nb * 7), dim3(256), 0, nullptr, cur, n, bit, lb, nb, pops);
    return wtsa_level_counts(lb, nb, pops, scratch);
}

// ---- the two walks ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t level_rank(const WtsaView& w, uint32_t base, uint64_t i) { return (uint32_t)node_rank1(w.blocks, base, i); }

// kQuantile false: number of values < xq among SA[l, l + len); true: the xq-th smallest of them (0-based, xq < len)
template <bool kQuantile>
__device__ __forceinline__ uint64_t wtsa_walk(const WtsaView& w, uint64_t l, uint64_t len, uint64_t xq)
{
    if (!kQuantile && (w.levels < 64 ? (xq >> w.levels) != 0 : false)) return len;    // beyond every value
    uint64_t b = 0, sz = w.n_vals, i = l, j = l + len, acc = 0;
    for (uint32_t lvl = 0; lvl < w.levels; ++lvl) {
        const uint32_t base = (uint32_t)(lvl * w.nb);
        const uint32_t rb = level_rank(w, base, b), ri = level_rank(w, base, b + i), rj = level_rank(w, base, b + j),
                       rn = level_rank(w, base, b + sz);
        const uint64_t ones_i = ri - rb, ones_j = rj - rb, ones_n = rn - rb;
        const uint64_t zi = i - ones_i, zj = j - ones_j, zeros_n = sz - ones_n;
        bool right;
        if (kQuantile) {
            const uint64_t z = zj - zi;
            right = xq >= z;
            if (right) { xq -= z; acc |= 1ull << (w.levels - 1 - lvl); }
        } else {
            right = (xq >> (w.levels - 1 - lvl)) & 1;
            if (right) acc += zj - zi;
        }
        if (right) { i = ones_i; j = ones_j; b += zeros_n; sz = ones_n; }
        else { i = zi; j = zj; sz = zeros_n; }
    }
    return acc;
}

__device__ __forceinline__ int64_t wtsa_symbol(const WtsaView& w, uint64_t p)
{
    if (p >= w.n_text) return -1;                                   // the sentinel is smaller than every symbol
    return w.sym_bytes == 1 ? (int64_t)reinterpret_cast<const uint8_t*>(w.text)[p] : (int64_t)reinterpret_cast<const uint32_t*>(w.text)[p];
}

__global__ void __launch_bounds__(256) wtsa_sa_kernel(WtsaView w, const uint64_t* __restrict__ idx, uint64_t* __restrict__ out, uint64_t count)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (uint64_t)gridDim.x * blockDim.x)
        out[t] = idx[t] < w.n_vals ? wtsa_walk<true>(w, idx[t], 1, 0) : ~0ull;
}

// forward_search (suffix_array_algorithm.hpp:48-112): binary search on the suffix array, every probe one access + one comparison
// of the pattern with the text.  One lane per sub-pattern.
__global__ void __launch_bounds__(256) wtsa_ranges_kernel(WtsaView w, const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off,
                                                          uint64_t n_pat, uint64_t* __restrict__ sp, uint64_t* __restrict__ len)
{
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pat; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t m = (off[p + 1] - off[p]) / w.sym_bytes;
        const uint8_t* pat = blob + off[p];
        auto cmp = [&](uint64_t s) -> int {                         // suffix s against the pattern: -1 smaller, 0 has it as a prefix, +1 greater
            for (uint64_t t = 0; t < m; ++t) {
                const int64_t c = wtsa_symbol(w, s + t);
                const int64_t x = w.sym_bytes == 1 ? (int64_t)pat[t] : (int64_t)reinterpret_cast<const uint32_t*>(pat)[t];
                if (c != x) return c < x ? -1 : 1;
            }
            return 0;
        };
        uint64_t lo = 0, hi = w.n_vals;
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (cmp(wtsa_walk<true>(w, mid, 1, 0)) < 0) lo = mid + 1; else hi = mid; }
        const uint64_t first = lo;
        hi = w.n_vals;
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (cmp(wtsa_walk<true>(w, mid, 1, 0)) <= 0) lo = mid + 1; else hi = mid; }
        sp[p] = first;
        len[p] = lo - first;
    }
}

// The text window [wbegin, wend) of every query (begin <= end <= n_text, made so on the host) as ranks of its sub-patterns' lists: an
// occurrence v of a sub-pattern of m symbols lies wholly inside when begin <= v and v + m <= end, and the list is the sorted
// SA[sp, sp + len), so those are its elements of rank [count_less(begin), count_less(end - m + 1)).  One lane per sub-pattern of the
// batch, its query found in qsub; a side of the window that cuts nothing (begin 0, end = the text's) takes no walk.
__global__ void __launch_bounds__(256) wtsa_window_kernel(WtsaView w, const uint64_t* __restrict__ off, const uint64_t* __restrict__ qsub, uint64_t nq,
                                                          uint64_t n_pat, const uint64_t* __restrict__ sp, const uint64_t* __restrict__ len,
                                                          const uint64_t* __restrict__ wbegin, const uint64_t* __restrict__ wend,
                                                          uint64_t* __restrict__ rlo, uint64_t* __restrict__ rhi)
{
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pat; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t m = (off[p + 1] - off[p]) / w.sym_bytes, l = sp[p], n = len[p];
        const uint64_t qj = extract_range_of(qsub, nq, p);
        const uint64_t b = wbegin[qj], e = wend[qj];
        uint64_t from = 0, to = n;
        if (e - b < m) to = 0;                                      // the window is shorter than the sub-pattern
        else if (n) {
            if (b) from = wtsa_walk<false>(w, l, n, b);
            if (e < w.n_text) to = wtsa_walk<false>(w, l, n, e - m + 1);
        }
        rlo[p] = from;
        rhi[p] = to;
    }
}

// ---- the lazy search ----------------------------------------------------------------------------------------------------------------
// Semantics: SURVEY.md Appendix C (what vlg_iterator yields, include/sdsl/vlg_index.hpp:227-291) -- the left-most, lazy,
// non-overlapping tuples.  One lane owns a query and keeps the reference's k monotone pointers, as RANKS into the sorted
// occurrence lists that exist only implicitly in the tree: `count_less` moves a pointer to the first element at or after a
// position, `quantile` reads the element under it.  Where the reference steps a pointer one element at a time (relax: next_right,
// vlg_index.hpp:233-249), the lane leaps: when the element of list i under the pointer lies beyond the window of the element of
// list i-1, every element of list i-1 before  v_i - hi_i  fails the same way, so pointer i-1 goes straight to the first element at
// or after that position.  A pointer that runs off its list ends the query ("stop entirely").  The work of a query is a few
// walks per match or failed alignment, whatever the lengths of its lists -- and it stops after max_matches matches.
struct WQuery { uint32_t k, sub0; uint64_t end_len, out_first, out_tuple; };

// kWave: ONE WAVEFRONT owns a query.  All 64 lanes run the same pointer machine (same walks, same addresses), and whenever the
// pointer of the query's SHORTEST list is set, the lanes look at the next 64 elements of that list at once -- one quantile walk each,
// then two count_less walks per neighbouring list -- and the pointer skips to the first element that has a partner inside the gap
// window on either side.  An element without one is in no tuple at all, so dropping it changes no least tuple and no restart
// position (the argument of the window filter); what it removes is the query's sequential walk over every
// fruitless alignment -- 3 k leaps per element of the shortest list, each two 30-level walks -- which is what a heavy query
// without early matches used to cost (seconds on C3).  kWave false: one lane per query, 64 queries per wavefront.
//
// A text window [begin, end) of a query (vlg_wtsa_search_window_batch) cuts every list to the rank interval [rlo, rhi) of its sorted
// values (wtsa_window_kernel below); the walks still run on the true (sp, len).  Every key a pointer is moved to lies at or behind
// `begin` -- it is derived from an element under another pointer -- so count_less never answers below rlo: the window is the rank the
// first pointer starts at, `r >= rhi` for "the list has run out", the pivot chosen and scanned inside [rlo, rhi), and its partner
// counts clamped to the neighbour's interval.  Without a window rlo = 0 and rhi = len: the machine of before.
// next[q]: where a search that stopped at max_matches is continued (vlg_result_next_positions), ~0 when the query ran out.
template <bool kEmit, bool kWave>
__global__ void __launch_bounds__(64) wtsa_search_kernel(WtsaView w, const uint64_t* __restrict__ sp, const uint64_t* __restrict__ len,
                                                         const uint64_t* __restrict__ rlo, const uint64_t* __restrict__ rhi,
                                                         const uint64_t* __restrict__ wend,
                                                         const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi,
                                                         const WQuery* __restrict__ qs, uint32_t nq, uint32_t kmax, uint64_t max_matches,
                                                         unsigned long long* __restrict__ counts, uint64_t* __restrict__ next,
                                                         uint64_t* __restrict__ out_first,
                                                         uint64_t* __restrict__ out_tuples, unsigned long long* __restrict__ checksum)
{
    extern __shared__ uint32_t s_dyn[];                            // [2][kmax][64]: rank and value under every pointer, per lane
    const uint32_t lane = threadIdx.x;
    const uint64_t qi = kWave ? (uint64_t)blockIdx.x : (uint64_t)blockIdx.x * 64 + lane;
    const bool writer = !kWave || lane == 0;                      // kWave: every lane holds the same state, one of them reports it
    uint32_t* s_rank = s_dyn;
    uint32_t* s_val = s_dyn + (size_t)kmax * 64;
    WQuery Q{0, 0, 0, 0, 0};
    if (qi < nq) Q = qs[qi];
    const uint32_t k = Q.k;
    bool fin = qi >= nq || k == 0;
    for (uint32_t i = 0; i < k && !fin; ++i) fin = rhi[Q.sub0 + i] <= rlo[Q.sub0 + i];   // vlg_index.hpp:315-316: an empty range ends it at once
    uint32_t piv = 0;                                              // kWave: the shortest list of the query (inside its window)
    if (kWave && !fin && k >= 2) {
        uint64_t best = ~0ull;
        for (uint32_t i = 0; i < k; ++i) { const uint64_t n_in = rhi[Q.sub0 + i] - rlo[Q.sub0 + i]; if (n_in < best) { best = n_in; piv = i; } }
    }
    uint64_t emitted = 0, nxt = ~0ull;
    unsigned long long sum = 0;
    // pending walk: level `lv`; op 0 = count_less(key) -> rank, then always the quantile of that rank
    uint32_t lv = 0;
    bool need_count = false;                                       // false: the rank at lv is set, read its value
    uint64_t key = 0;
    uint32_t have = 0;                                             // levels (< 32 tracked; beyond: always recomputed) whose pointer holds a value
    if (!fin) s_rank[lane] = (uint32_t)rlo[Q.sub0];
    while (__any(!fin)) {
        if (!fin) {
            const uint32_t s = Q.sub0 + lv;
            const uint64_t li = sp[s], ni = len[s], re = rhi[s];
            uint64_t r = s_rank[lv * 64 + lane];
            if (need_count) r = wtsa_walk<false>(w, li, ni, key);         // (every key lies beyond the element under the pointer: it only moves forward)
            if (kWave && k >= 2 && lv == piv) {
                // (wave-uniform from here to the ballot: every lane holds the same r)  64 elements of the shortest list at a time
                while (r < re) {
                    const uint64_t cand = r + lane;
                    bool ok = false;
                    if (cand < re) {
                        const uint64_t v = wtsa_walk<true>(w, li, ni, cand);
                        ok = true;
                        if (piv > 0) {                                      // an element u of the list before with lo <= v - u <= hi
                            const uint64_t l_ = lo[s], h_ = hi[s];
                            if (v < l_) ok = false;
                            else {
                                const uint64_t a = v > h_ ? v - h_ : 0, b = v - l_;
                                const uint64_t lp = sp[s - 1], np = len[s - 1];
                                const uint64_t from = wtsa_walk<false>(w, lp, np, a), to = wtsa_walk<false>(w, lp, np, b + 1);
                                ok = (to < rhi[s - 1] ? to : rhi[s - 1]) > (from > rlo[s - 1] ? from : rlo[s - 1]);
                            }
                        }
                        if (ok && piv + 1 < k) {                            // an element x of the list behind with lo' <= x - v <= hi'
                            const uint64_t l_ = lo[s + 1], h_ = hi[s + 1];
                            const uint64_t a = v + l_ < v ? ~0ull : v + l_, b = v + h_ < v ? ~0ull : v + h_;
                            const uint64_t ln = sp[s + 1], nn = len[s + 1];
                            if (a == ~0ull) ok = false;
                            else {
                                const uint64_t from = wtsa_walk<false>(w, ln, nn, a), to = b == ~0ull ? nn : wtsa_walk<false>(w, ln, nn, b + 1);
                                ok = (to < rhi[s + 1] ? to : rhi[s + 1]) > (from > rlo[s + 1] ? from : rlo[s + 1]);
                            }
                        }
                    }
                    const unsigned long long m = __ballot(ok);
                    if (m) { r += (uint32_t)__ffsll((long long)m) - 1; break; }
                    r += 64;
                }
            }
            if (r >= re) fin = true;                                        // the list has run out (inside the window): nothing more for this query
            else {
                const uint64_t v = wtsa_walk<true>(w, li, ni, r);
                s_rank[lv * 64 + lane] = (uint32_t)r;
                s_val[lv * 64 + lane] = (uint32_t)v;
                if (lv < 32) have |= 1u << lv;
                // ---- decide the next walk: no memory is touched in here except the lane's own pointers ------------------------------
                for (;;) {
                    const uint64_t cur = s_val[lv * 64 + lane];
                    if (lv > 0) {
                        const uint64_t prev = s_val[(lv - 1) * 64 + lane];
                        const uint64_t h = hi[Q.sub0 + lv];
                        if (cur > (prev + h < prev ? ~0ull : prev + h)) {
                            // beyond the window of the element one list up: that pointer leaps to the first element that can reach cur
                            const uint64_t reach = cur - h;                 // (cur > prev + h >= h)
                            key = reach > prev + 1 ? reach : prev + 1;
                            --lv; need_count = true;
                            break;
                        }
                    }
                    if (lv + 1 == k) {                                      // a match: report it, then pull the first pointer behind it
                        const uint64_t first = s_val[lane];
                        if (writer) sum += first;
                        if (kEmit && writer) {
                            out_first[Q.out_first + emitted] = first;
                            if (out_tuples) {
                                uint64_t* tp = out_tuples + Q.out_tuple + emitted * k;
                                for (uint32_t i = 0; i < k; ++i) tp[i] = s_val[i * 64 + lane];
                            }
                        }
                        ++emitted;
                        if (max_matches && emitted >= max_matches) {       // stopped, not run out: the next search begins behind this match
                            const uint64_t we = wend[qi];                   // (never beyond the window's end: begin <= end holds for the next call)
                            nxt = cur + Q.end_len < we ? cur + Q.end_len : we;
                            fin = true;
                            break;
                        }
                        key = cur + Q.end_len;                              // vlg_index.hpp:254-266 (pull_forward)
                        lv = 0; need_count = true;
                        break;
                    }
                    // one list down: its pointer stays if it already stands at or behind the window's start
                    ++lv;
                    const uint64_t l = lo[Q.sub0 + lv];
                    const uint64_t from = cur + l < cur ? ~0ull : cur + l;
                    if (lv < 32 && ((have >> lv) & 1) && (uint64_t)s_val[lv * 64 + lane] >= from) continue;
                    key = from; need_count = true;
                    break;
                }
            }
        }
    }
    if (qi < nq && writer && counts) counts[qi] = emitted;
    if (qi < nq && writer && next) next[qi] = nxt;
    if (kEmit && checksum) {
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
        if (lane == 0 && sum) atomicAdd(checksum, sum);
    }
}

// capped searches run once, every query writing into its own cap-sized stretch; this moves the matches together (query-major)
__global__ void wtsa_compact_kernel(const WQuery* __restrict__ from, const uint64_t* __restrict__ to_first, const uint64_t* __restrict__ to_tuple,
                                    const unsigned long long* __restrict__ counts, uint32_t nq, uint64_t cap, const uint64_t* __restrict__ t_first,
                                    const uint64_t* __restrict__ t_tuples, uint64_t* __restrict__ out_first, uint64_t* __restrict__ out_tuples)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (uint64_t)nq * cap; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t qi = t / cap, m = t - qi * cap;
        if (m >= counts[qi]) continue;
        const WQuery Q = from[qi];
        out_first[to_first[qi] + m] = t_first[Q.out_first + m];
        if (out_tuples) for (uint32_t i = 0; i < Q.k; ++i) out_tuples[to_tuple[qi] + m * Q.k + i] = t_tuples[Q.out_tuple + m * Q.k + i];
    }
}

WtsaView wtsa_view(const vlg_wtsa* x) { return WtsaView{x->d_blocks, x->d_text, x->nb, x->n_vals, x->n_text, x->levels, x->sym_bytes}; }
vlg_status wtsa_level_prefix(vlg_wtsa* x);                          // wtsa_sdsl.hpp

}  // namespace

extern "C" void vlg_wtsa_destroy(vlg_wtsa* x)
{
    if (!x) return;
    if (x->d_blocks) (void)hipFree(x->d_blocks);
    if (x->d_text) (void)hipFree(x->d_text);
    if (x->d_level_prefix) (void)hipFree(x->d_level_prefix);
    delete x;
}

using WtsaPtr = Building<vlg_wtsa, vlg_wtsa_destroy>;

extern "C" vlg_status vlg_wtsa_build(const void* h_text, uint64_t n_symbols, uint32_t symbol_bytes, vlg_wtsa** out)
{
    if (!out || (n_symbols && !h_text)) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    if (symbol_bytes != 1 && symbol_bytes != 4) return fail(VLG_E_INVALID, "symbol_bytes must be 1 or 4");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available (the VLG library has no CPU fallback)");
    const uint64_t byte_len = n_symbols * (symbol_bytes == 1 ? 1 : 5);
    if (byte_len >= 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "text too long for the 32-bit suffix array of this index");
    release_cached_device_memory();
    WtsaPtr x(new vlg_wtsa());
    x->n_text = n_symbols; x->n_vals = n_symbols + 1; x->sym_bytes = symbol_bytes;
    x->levels = std::max(1u, bit_width64(n_symbols));               // values 0..n_symbols
    x->nb = x->n_vals / kBlockBits + 1;
    DevBuf d_text, d_sa, d_blocks, d_a, d_b, d_ka, d_kb, d_pops, d_tmp;
    VLG_HIP_TRY(d_text.alloc(n_symbols * symbol_bytes));
    if (n_symbols) VLG_HIP_TRY(hipMemcpy(d_text.p, h_text, n_symbols * symbol_bytes, hipMemcpyHostToDevice));
    x->d_text = d_text.take();
    // ---- suffix array of text + sentinel (the sorter of the FM-index builder) -----------------------------------------------------
    if (symbol_bytes == 1) {
        VLG_HIP_TRY(d_sa.alloc((n_symbols + 1) * 4));
        if (vlg_status st = vlg_suffix_array_device((const uint8_t*)x->d_text, n_symbols, d_sa.as<uint32_t>(), nullptr)) return st;
    } else {
        DevBuf d_flag;                                              // (the stage allocates it)
        if (vlg_status st = symbol_suffix_array((const uint32_t*)x->d_text, n_symbols, d_flag, d_sa)) return st;
    }
    // ---- the tree, one level at a time: emit the bits of the current arrangement, then sort stably by one more bit of prefix ---------
    const uint64_t n = x->n_vals;
    VLG_HIP_TRY(d_blocks.alloc((uint64_t)x->levels * x->nb * sizeof(Block)));
    x->d_blocks = static_cast<Block*>(d_blocks.take());
    VLG_HIP_TRY(d_a.alloc(n * 4));
    VLG_HIP_TRY(d_b.alloc(n * 4));
    VLG_HIP_TRY(d_ka.alloc(n * 4));
    VLG_HIP_TRY(d_kb.alloc(n * 4));
    VLG_HIP_TRY(d_pops.alloc((x->nb + 1) * 4));
    size_t sort_tb = 0, scan_tb = 0;                                // the larger request of the level loop: no level regrows d_tmp
    VLG_HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_tb, d_ka.as<uint32_t>(), d_kb.as<uint32_t>(), d_a.as<uint32_t>(), d_b.as<uint32_t>(), n, 0, 32, nullptr));
    VLG_HIP_TRY(rocprim::exclusive_scan(nullptr, scan_tb, d_pops.as<uint32_t>(), d_pops.as<uint32_t>(), 0u, x->nb + 1, rocprim::plus<uint32_t>(), nullptr));
    VLG_HIP_TRY(d_tmp.alloc(std::max(sort_tb, scan_tb)));
    VLG_HIP_TRY(hipMemcpy(d_a.p, d_sa.p, n * 4, hipMemcpyDeviceToDevice));
    uint32_t* cur = d_a.as<uint32_t>();
    uint32_t* other = d_b.as<uint32_t>();
    for (uint32_t lvl = 0; lvl < x->levels; ++lvl) {
        const uint32_t bit = x->levels - 1 - lvl;
        if (vlg_status st = wtsa_emit_level(cur, n, bit, x->d_blocks + (uint64_t)lvl * x->nb, x->nb, d_pops.as<uint32_t>(), d_tmp)) return st;
        if (lvl + 1 < x->levels) {                              // arrangement of the next level: stable by the top lvl + 1 bits
            hipLaunchKernelGGL(wtsa_prefix_keys_kernel, launch_grid(n), dim3(256), 0, nullptr, cur, n, bit, d_ka.as<uint32_t>());
            VLG_HIP_TRY(with_scratch(d_tmp, [&](void* t, size_t& tb) {
                return rocprim::radix_sort_pairs(t, tb, d_ka.as<uint32_t>(), d_kb.as<uint32_t>(), cur, other, n, 0, lvl + 1, nullptr);
            }));
            std::swap(cur, other);
        }
    }
    if (vlg_status st = wtsa_level_prefix(x.get())) return st;
    VLG_HIP_TRY(hipDeviceSynchronize());
    *out = x.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_get_info(const vlg_wtsa* x, vlg_wtsa_info* info)
{
    if (!x || !info) return fail(VLG_E_INVALID, "null argument");
    info->n = x->n_vals; info->symbol_bytes = x->sym_bytes; info->levels = x->levels; info->blocks_per_level = x->nb;
    info->hbm_bytes = x->n_text * x->sym_bytes + (uint64_t)x->levels * x->nb * sizeof(Block);
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_sa_batch(const vlg_wtsa* x, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!x || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipLaunchKernelGGL(wtsa_sa_kernel, launch_grid(count, 8192), dim3(256), 0, (hipStream_t)stream, wtsa_view(x), d_i, d_out, count);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

namespace {
// bits of one level as plain 64-bit words (bit i of the level = word[i >> 6] >> (i & 63)): what wt_int::tree holds for it
__global__ void wtsa_level_words_kernel(WtsaView w, uint32_t lvl, uint64_t* __restrict__ out, uint64_t n_words)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_words; t += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t word = 0;
        for (uint32_t half = 0; half < 2; ++half) {                 // 32 bits at a time: a 32-bit data word of a block, or parts of two
            const uint64_t bit = t * 64 + 32 * half;
            if (bit >= w.n_vals) break;
            const uint64_t blk = bit / kBlockBits;
            const uint32_t off = (uint32_t)(bit - blk * kBlockBits), wi = off >> 5, sh = off & 31;
            const Block* B = w.blocks + (uint64_t)lvl * w.nb + blk;
            uint64_t v = B->w[wi] >> sh;
            if (sh) {                                                // the rest comes from the next data word (maybe of the next block)
                const uint32_t nx = wi + 1 < 7 ? B->w[wi + 1] : (blk + 1 < w.nb ? B[1].w[0] : 0u);
                v |= (uint64_t)nx << (32 - sh);
            }
            word |= (v & 0xFFFFFFFFull) << (32 * half);
        }
        const uint64_t left = w.n_vals - t * 64;
        if (left < 64) word &= (1ull << left) - 1;
        out[t] = word;
    }
}
__global__ void __launch_bounds__(256) wtsa_range_walk_kernel(WtsaView w, const uint64_t* __restrict__ l, const uint64_t* __restrict__ len,
                                                              const uint64_t* __restrict__ x, int quantile, uint64_t* __restrict__ out, uint64_t count)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = l[t], n = len[t];
        const bool ok = a <= w.n_vals && n <= w.n_vals - a && (!quantile || x[t] < n);
        out[t] = !ok ? ~0ull : (quantile ? wtsa_walk<true>(w, a, n, x[t]) : (n ? wtsa_walk<false>(w, a, n, x[t]) : 0));
    }
}
// wt_int::range_search_2d (wt_int.hpp:612-700) on SA[l, l + len) x [vlb, vrb]: the values inside are the ranks
// [count_less(vlb), count_less(vrb + 1)) of the sorted range.  ok: the range lies inside the suffix array.
__device__ __forceinline__ void wtsa_value_ranks(const WtsaView& w, uint64_t a, uint64_t n, uint64_t vlb, uint64_t vrb, bool& ok, uint64_t& from, uint64_t& to)
{
    ok = a <= w.n_vals && n <= w.n_vals - a;
    from = to = 0;
    if (!ok || !n || vlb > vrb) return;
    from = wtsa_walk<false>(w, a, n, vlb);
    to = vrb == ~0ull ? n : wtsa_walk<false>(w, a, n, vrb + 1);     // (a vrb beyond every value: the walk answers n)
}
__global__ void __launch_bounds__(256) wtsa_range_count_kernel(WtsaView w, const uint64_t* __restrict__ l, const uint64_t* __restrict__ len,
                                                               const uint64_t* __restrict__ vlb, const uint64_t* __restrict__ vrb,
                                                               uint64_t* __restrict__ out, uint64_t count)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (uint64_t)gridDim.x * blockDim.x) {
        bool ok;
        uint64_t from, to;
        wtsa_value_ranks(w, l[t], len[t], vlb[t], vrb[t], ok, from, to);
        out[t] = ok ? to - from : ~0ull;
    }
}
// One lane per reported value: element t of the output belongs to the last range j with out_off[j] <= t (extract_range_of) and is
// the (count_less(vlb) + t - out_off[j])-th smallest of SA[l, l + len) -- one quantile walk, independent of every other output, and the
// outputs of a range come out ascending.  Consecutive lanes hold consecutive ranks of one range: their walks share the first levels
// (the same super-blocks, one read for the wave) and part only where their ranks do.  An element whose range lies outside the
// suffix array, or whose rank lies beyond the values inside [vlb, vrb] (offsets that are not the prefix sum of the counts), is not written.
__global__ void __launch_bounds__(256) wtsa_range_report_kernel(WtsaView w, const uint64_t* __restrict__ l, const uint64_t* __restrict__ len,
                                                                const uint64_t* __restrict__ vlb, const uint64_t* __restrict__ vrb,
                                                                const uint64_t* __restrict__ out_off, uint64_t count, uint64_t total,
                                                                uint64_t* __restrict__ out)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = extract_range_of(out_off, count, t);
        if (t < out_off[j]) continue;                               // (offsets that do not start at 0)
        bool ok;
        uint64_t from, to;
        wtsa_value_ranks(w, l[j], len[j], vlb[j], vrb[j], ok, from, to);
        const uint64_t r = from + (t - out_off[j]);
        if (ok && r < to) out[t] = wtsa_walk<true>(w, l[j], len[j], r);
    }
}
}  // namespace

extern "C" vlg_status vlg_wtsa_export_level(const vlg_wtsa* x, uint32_t level, uint64_t* h_words)
{
    if (!x || !h_words) return fail(VLG_E_INVALID, "null argument");
    if (level >= x->levels) return fail(VLG_E_INVALID, "no such level");
    const uint64_t nw = (x->n_vals + 63) / 64;
    DevBuf d;
    VLG_HIP_TRY(d.alloc(nw * 8));
    hipLaunchKernelGGL(wtsa_level_words_kernel, launch_grid(nw, 8192), dim3(256), 0, nullptr, wtsa_view(x), level, d.as<uint64_t>(), nw);
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipMemcpy(h_words, d.p, nw * 8, hipMemcpyDeviceToHost));
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_range_walk_batch(const vlg_wtsa* x, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_x, int quantile,
                                                uint64_t* d_out, uint64_t count, void* stream)
{
    if (!x || (count && (!d_l || !d_len || !d_x || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipLaunchKernelGGL(wtsa_range_walk_kernel, launch_grid(count, 8192), dim3(256), 0, (hipStream_t)stream, wtsa_view(x), d_l, d_len, d_x,
                       quantile, d_out, count);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_range_count_batch(const vlg_wtsa* x, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_vlb,
                                                 const uint64_t* d_vrb, uint64_t* d_count, uint64_t count, void* stream)
{
    if (!x || (count && (!d_l || !d_len || !d_vlb || !d_vrb || !d_count))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipLaunchKernelGGL(wtsa_range_count_kernel, launch_grid(count, 8192), dim3(256), 0, (hipStream_t)stream, wtsa_view(x), d_l, d_len, d_vlb, d_vrb,
                       d_count, count);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_range_report_batch(const vlg_wtsa* x, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_vlb,
                                                  const uint64_t* d_vrb, const uint64_t* d_out_off, uint64_t count, uint64_t total, uint64_t* d_out,
                                                  void* stream)
{
    if (!x || (count && (!d_l || !d_len || !d_vlb || !d_vrb || !d_out_off)) || (total && !d_out)) return fail(VLG_E_INVALID, "null argument");
    if (!count || !total) return VLG_OK;
    hipLaunchKernelGGL(wtsa_range_report_kernel, launch_grid(total, 8192), dim3(256), 0, (hipStream_t)stream, wtsa_view(x), d_l, d_len, d_vlb, d_vrb,
                       d_out_off, count, total, d_out);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

namespace {
vlg_status wtsa_ranges_device(const vlg_wtsa* x, const vlg_queries* q, uint64_t* d_sp, uint64_t* d_len, hipStream_t st)
{
    if (q->sym_bytes != x->sym_bytes) return fail(VLG_E_INVALID, "the query batch and the index have different alphabets");
    if (!q->nsub) return VLG_OK;
    hipLaunchKernelGGL(wtsa_ranges_kernel, launch_grid(q->nsub, 4096), dim3(256), 0, st, wtsa_view(x), q->d_blob, q->d_suboff, q->nsub, d_sp, d_len);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}
}  // namespace

extern "C" vlg_status vlg_wtsa_ranges(const vlg_wtsa* x, const vlg_queries* q, uint64_t* h_sp, uint64_t* h_ep, void* stream)
{
    if (!x || !q || (q->nsub && (!h_sp || !h_ep))) return fail(VLG_E_INVALID, "null argument");
    if (q->has_classes()) return fail(VLG_E_UNSUPPORTED, "a batch with character classes is searched by vlg_search_batch on a byte FM-index only");
    if (q->has_mismatches()) return fail(VLG_E_UNSUPPORTED, "a batch with mismatch budgets is searched by vlg_search_batch on a byte FM-index only");
    if (!q->nsub) return VLG_OK;
    DevBuf d;
    VLG_HIP_TRY(d.alloc(2 * q->nsub * 8));
    std::vector<uint64_t> h(2 * q->nsub);
    if (vlg_status s = wtsa_ranges_device(x, q, d.as<uint64_t>(), d.as<uint64_t>() + q->nsub, (hipStream_t)stream)) return s;
    VLG_HIP_TRY(hipMemcpyAsync(h.data(), d.p, 2 * q->nsub * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    VLG_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (uint64_t i = 0; i < q->nsub; ++i) { h_sp[i] = h[i]; h_ep[i] = h[i] + h[q->nsub + i] - 1; }    // sp = ep + 1 when there is no occurrence
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_search_window_batch(const vlg_wtsa* x, const vlg_queries* q, const uint64_t* h_begin, const uint64_t* h_end,
                                                   uint64_t max_matches, vlg_workspace* ws, vlg_result** out)
{
    if (!x || !q || !ws || !out) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    if (q->has_classes()) return fail(VLG_E_UNSUPPORTED, "a batch with character classes is searched by vlg_search_batch on a byte FM-index only");
    if (q->has_mismatches()) return fail(VLG_E_UNSUPPORTED, "a batch with mismatch budgets is searched by vlg_search_batch on a byte FM-index only");
    if (q->has_windows()) return fail(VLG_E_INVALID, "the batch carries text windows (vlg_queries_set_windows): this search takes its windows as arrays");
    if (q->has_documents()) return fail(VLG_E_UNSUPPORTED, "the batch carries documents (vlg_queries_set_documents): vlg_search_batch honours them, this search does not");
    hipStream_t st = ws->stream;
    const uint64_t nq = q->nq, nsub = q->nsub;
    if (nq > 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "too many queries in one batch");
    if (h_begin && h_end)
        for (uint64_t i = 0; i < nq; ++i) if (h_begin[i] > h_end[i]) return fail(VLG_E_INVALID, "a window begins behind its end");
    vlg_result* res = new_result(nq, q->qsub);
    res->has_next = true;
    res->next.assign(nq, ~0ull);
    DevBuf d_mem;
    ResultPiece piece;
    piece.q0 = 0; piece.q1 = nq;
    auto run = [&]() -> vlg_status {
        if (!nq) { res->pieces.push_back(piece); return VLG_OK; }
        // device scratch: ranges, their cut to the windows, gap bounds, windows, next positions, query table, counts, checksum
        const uint64_t bytes = (6 * (nsub + 1) + 4 * nq + 2) * 8 + (nq + 1) * sizeof(WQuery) + 1024;
        VLG_HIP_TRY(d_mem.alloc(bytes));
        uint64_t* d_sp = d_mem.as<uint64_t>();
        uint64_t* d_len = d_sp + nsub + 1;
        uint64_t* d_rlo = d_len + nsub + 1;
        uint64_t* d_rhi = d_rlo + nsub + 1;
        uint64_t* d_lo = d_rhi + nsub + 1;
        uint64_t* d_hi = d_lo + nsub + 1;
        uint64_t* d_wb = d_hi + nsub + 1;
        uint64_t* d_we = d_wb + nq;
        uint64_t* d_next = d_we + nq;
        unsigned long long* d_counts = (unsigned long long*)(d_next + nq);
        unsigned long long* d_chk = d_counts + nq;
        WQuery* d_q = (WQuery*)(d_chk + 2);
        // the windows: end clamped to the text, begin to the end (a window behind the text is an empty one)
        svec<uint64_t> hwb(nq), hwe(nq), hnext(nq);
        for (uint64_t i = 0; i < nq; ++i) {
            hwe[i] = h_end ? std::min<uint64_t>(h_end[i], x->n_text) : x->n_text;
            hwb[i] = h_begin ? std::min<uint64_t>(h_begin[i], hwe[i]) : 0;
        }
        VLG_HIP_TRY(hipMemcpyAsync(d_wb, hwb.data(), nq * 8, hipMemcpyHostToDevice, st));
        VLG_HIP_TRY(hipMemcpyAsync(d_we, hwe.data(), nq * 8, hipMemcpyHostToDevice, st));
        svec<WQuery> hq(nq);
        for (uint64_t i = 0; i < nq; ++i) hq[i] = WQuery{res->k[i], (uint32_t)q->qsub[i], q->end_len[i], 0, 0};
        svec<uint64_t> hlo(q->lo.begin(), q->lo.end()), hhi(q->hi.begin(), q->hi.end());
        if (nsub) {
            VLG_HIP_TRY(hipMemcpyAsync(d_lo, hlo.data(), nsub * 8, hipMemcpyHostToDevice, st));
            VLG_HIP_TRY(hipMemcpyAsync(d_hi, hhi.data(), nsub * 8, hipMemcpyHostToDevice, st));
        }
        VLG_HIP_TRY(hipMemcpyAsync(d_q, hq.data(), nq * sizeof(WQuery), hipMemcpyHostToDevice, st));
        VLG_HIP_TRY(hipMemsetAsync(d_chk, 0, 16, st));
        {
            Timed t(ws, KS_BSEARCH, 0);
            if (vlg_status s = wtsa_ranges_device(x, q, d_sp, d_len, st)) return s;
            if (nsub) {
                hipLaunchKernelGGL(wtsa_window_kernel, launch_grid(nsub, 4096), dim3(256), 0, st, wtsa_view(x), q->d_suboff, q->d_qsub, nq, nsub, d_sp,
                                   d_len, d_wb, d_we, d_rlo, d_rhi);
                VLG_HIP_TRY(hipGetLastError());
            }
        }
        const uint32_t kmax = std::max<uint32_t>(q->kmax, 1);
        const size_t lds = (size_t)2 * kmax * 64 * 4;
        // one wavefront per query (its shortest list is looked at 64 elements at a time), or the older one lane per query
        const bool wave = [] { const char* e = getenv("VLG_WTSA_LANE_PER_QUERY"); return !(e && e[0] == '1'); }();
        const uint32_t wgs = wave ? (uint32_t)nq : (uint32_t)((nq + 63) / 64);
        const WtsaView w = wtsa_view(x);
        // A capped search whose matches fit a scratch buffer at cap per query runs ONCE (the uncapped one counts first, then emits)
        const uint64_t per_query = max_matches * (1 + (ws->tuples ? (uint64_t)kmax : 0)) * 8;
        if (wave && max_matches && max_matches <= (1u << 20) && nq * per_query <= (2ull << 30)) {
            DevBuf d_capped;
            VLG_HIP_TRY(d_capped.alloc(nq * per_query + 2 * (nq + 1) * 8));
            uint64_t* t_first = d_capped.as<uint64_t>();
            uint64_t* t_tuples = ws->tuples ? t_first + nq * max_matches : nullptr;
            uint64_t* d_to_first = t_first + nq * per_query / 8;
            uint64_t* d_to_tuple = d_to_first + nq + 1;
            for (uint64_t i = 0; i < nq; ++i) { hq[i].out_first = i * max_matches; hq[i].out_tuple = i * max_matches * kmax; }
            VLG_HIP_TRY(hipMemcpyAsync(d_q, hq.data(), nq * sizeof(WQuery), hipMemcpyHostToDevice, st));
            {
                Timed t(ws, KS_JOIN_CHAIN, 0);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(wtsa_search_kernel<true, true>), dim3(wgs), dim3(64), lds, st, w, d_sp, d_len, d_rlo, d_rhi, d_we, d_lo,
                                   d_hi, d_q, (uint32_t)nq, kmax, max_matches, d_counts, d_next, t_first, t_tuples, d_chk);
            }
            VLG_HIP_TRY(hipGetLastError());
            svec<unsigned long long> counts(nq);
            unsigned long long chk = 0;
            VLG_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, nq * 8, hipMemcpyDeviceToHost, st));
            VLG_HIP_TRY(hipMemcpyAsync(hnext.data(), d_next, nq * 8, hipMemcpyDeviceToHost, st));
            VLG_HIP_TRY(hipMemcpyAsync(&chk, d_chk, 8, hipMemcpyDeviceToHost, st));
            VLG_HIP_TRY(hipStreamSynchronize(st));
            std::copy(hnext.begin(), hnext.end(), res->next.begin());
            svec<uint64_t> to_first(nq + 1), to_tuple(nq + 1);
            uint64_t M = 0, TV = 0;
            for (uint64_t i = 0; i < nq; ++i) {
                to_first[i] = M; to_tuple[i] = TV;
                M += counts[i]; TV += ws->tuples ? counts[i] * hq[i].k : 0;
                res->counts[i] = counts[i];
            }
            piece.matches = M; piece.tuple_vals = TV;
            if (M) {
                VLG_HIP_TRY(result_alloc(&piece.d_first, M * 8, &piece.first_bytes));
                if (TV) VLG_HIP_TRY(result_alloc(&piece.d_tuples, TV * 8, &piece.tuple_bytes));
                VLG_HIP_TRY(hipMemcpyAsync(d_to_first, to_first.data(), nq * 8, hipMemcpyHostToDevice, st));
                VLG_HIP_TRY(hipMemcpyAsync(d_to_tuple, to_tuple.data(), nq * 8, hipMemcpyHostToDevice, st));
                Timed t(ws, KS_GATHER, 8ull * (M + TV));
                hipLaunchKernelGGL(wtsa_compact_kernel, launch_grid(nq * max_matches, 8192), dim3(256), 0, st, d_q, d_to_first, d_to_tuple, d_counts,
                                   (uint32_t)nq, max_matches, t_first, TV ? t_tuples : nullptr, static_cast<uint64_t*>(piece.d_first),
                                   static_cast<uint64_t*>(piece.d_tuples));
                VLG_HIP_TRY(hipGetLastError());
            }
            VLG_HIP_TRY(hipStreamSynchronize(st));
            res->pieces.push_back(piece);
            res->sum.n_matches = M;
            res->sum.n_tuple_values = TV;
            res->sum.checksum = chk;
            res->sum.n_chunks = 1;
            return VLG_OK;
        }
        {
            Timed t(ws, KS_JOIN_CHAIN, 0);
            if (wave)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(wtsa_search_kernel<false, true>), dim3(wgs), dim3(64), lds, st, w, d_sp, d_len, d_rlo, d_rhi, d_we, d_lo,
                                   d_hi, d_q, (uint32_t)nq, kmax, max_matches, d_counts, d_next, nullptr, nullptr, nullptr);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(wtsa_search_kernel<false, false>), dim3(wgs), dim3(64), lds, st, w, d_sp, d_len, d_rlo, d_rhi, d_we, d_lo,
                                   d_hi, d_q, (uint32_t)nq, kmax, max_matches, d_counts, d_next, nullptr, nullptr, nullptr);
        }
        VLG_HIP_TRY(hipGetLastError());
        svec<unsigned long long> counts(nq);
        VLG_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, nq * 8, hipMemcpyDeviceToHost, st));
        VLG_HIP_TRY(hipMemcpyAsync(hnext.data(), d_next, nq * 8, hipMemcpyDeviceToHost, st));
        VLG_HIP_TRY(hipStreamSynchronize(st));
        std::copy(hnext.begin(), hnext.end(), res->next.begin());
        uint64_t M = 0, TV = 0;
        for (uint64_t i = 0; i < nq; ++i) {
            hq[i].out_first = M; hq[i].out_tuple = TV;
            M += counts[i]; TV += ws->tuples ? counts[i] * hq[i].k : 0;
            res->counts[i] = counts[i];
        }
        piece.matches = M; piece.tuple_vals = TV;
        if (M) {
            VLG_HIP_TRY(result_alloc(&piece.d_first, M * 8, &piece.first_bytes));
            if (TV) VLG_HIP_TRY(result_alloc(&piece.d_tuples, TV * 8, &piece.tuple_bytes));
            VLG_HIP_TRY(hipMemcpyAsync(d_q, hq.data(), nq * sizeof(WQuery), hipMemcpyHostToDevice, st));
            Timed t(ws, KS_GATHER, 8ull * (M + TV));
            if (wave)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(wtsa_search_kernel<true, true>), dim3(wgs), dim3(64), lds, st, w, d_sp, d_len, d_rlo, d_rhi, d_we, d_lo,
                                   d_hi, d_q, (uint32_t)nq, kmax, max_matches, d_counts, nullptr, static_cast<uint64_t*>(piece.d_first),
                                   static_cast<uint64_t*>(piece.d_tuples), d_chk);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(wtsa_search_kernel<true, false>), dim3(wgs), dim3(64), lds, st, w, d_sp, d_len, d_rlo, d_rhi, d_we, d_lo,
                                   d_hi, d_q, (uint32_t)nq, kmax, max_matches, d_counts, nullptr, static_cast<uint64_t*>(piece.d_first),
                                   static_cast<uint64_t*>(piece.d_tuples), d_chk);
            VLG_HIP_TRY(hipGetLastError());
        }
        unsigned long long chk = 0;
        VLG_HIP_TRY(hipMemcpyAsync(&chk, d_chk, 8, hipMemcpyDeviceToHost, st));
        VLG_HIP_TRY(hipStreamSynchronize(st));
        res->pieces.push_back(piece);
        res->sum.n_matches = M;
        res->sum.n_tuple_values = TV;
        res->sum.checksum = chk;
        res->sum.n_chunks = 1;
        return VLG_OK;
    };
    vlg_status stt;
    {
        HostPoolScope staging(&ws->host);
        try { stt = run(); }
        catch (const std::bad_alloc&) { stt = fail(VLG_E_OOM, "out of host memory (pinned staging)"); }
    }
    if (stt) { if (piece.d_first && res->pieces.empty()) result_cache().give(piece.d_first, piece.first_bytes);
               if (piece.d_tuples && res->pieces.empty()) result_cache().give(piece.d_tuples, piece.tuple_bytes);
               vlg_result_destroy(res); return stt; }
    *out = res;
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_search_batch(const vlg_wtsa* x, const vlg_queries* q, uint64_t max_matches, vlg_workspace* ws, vlg_result** out)
{
    return vlg_wtsa_search_window_batch(x, q, nullptr, nullptr, max_matches, ws, out);
}

extern "C" vlg_status vlg_result_next_positions(const vlg_result* r, uint64_t* h_next)
{
    if (!r || (!h_next && !r->next.empty())) return fail(VLG_E_INVALID, "null argument");
    if (!r->has_next) return fail(VLG_E_INVALID, "next positions exist for the results of vlg_wtsa_* searches only");
    std::copy(r->next.begin(), r->next.end(), h_next);
    return VLG_OK;
}
