// Document listing: which documents each query of a result matches, and how often -- vlg_result_list_documents, vlg_doc_listing_*
// (include/vlg_hip.h).  Part of search.hip's translation unit; doc_list_math.hpp holds the arithmetic that is not wave code.
//
// The first positions of a result lie in HBM, ascending per query, beside the document starts and their fences.  Three passes reduce
// them to one (document, first match) pair per maximal run of matches of one query in one document:
//   heads   : element-parallel like the join passes -- the matches of a piece are dealt to waves in runs of kDocListRun, a wave takes 64
//             per step: load the positions, find every lane's document, find the query borders of the step, flag the heads, ballot.
//             One word of head bits per step, one head count per run.
//   scan    : exclusive scan of the head counts of all runs of all pieces (rocPRIM); the last entry is the number of pairs.
//   scatter : (VLG_DOCLIST_PAIRS) every head writes its document (4 bytes: n_docs < 2^32 - 16) and its match index at its rank.
// The pairs of a query begin at the head rank of its first match (doc_borders_kernel): df is the difference of neighbours.
// Scratch beyond the outputs: one bit per match, one word per run, the match offsets of the queries -- from result_alloc, returned.
// The scatter pass finds the document of a head again from its position (one lane on its own, through the fences) by default;
// VLG_DOCLIST_STORE_IDS=1 in the environment makes the head pass store 4 bytes per match for it to read instead (DESIGN.md 8 has
// both measured).  Under VLG_DOCLIST_DF nothing is stored either way.
#include "doc_list_math.hpp"

namespace {

#ifndef VLG_DOCLIST_RUN
#define VLG_DOCLIST_RUN 2048
#endif
// a multiple of 64: runs start on a word of the head bits, and a step writes that word whole
static_assert(VLG_DOCLIST_RUN >= 64 && VLG_DOCLIST_RUN % 64 == 0 && VLG_DOCLIST_RUN <= (1u << 24), "VLG_DOCLIST_RUN: a multiple of 64 matches, at least 64");
constexpr uint32_t kDocListRun = VLG_DOCLIST_RUN;      // matches a wave of the head and scatter passes takes

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// The documents of a wave's step (the DocWave of the join passes, answering with the document instead of its end).  Positions ascend
// only inside a query, so the step is bracketed by its smallest and largest key, not by its first and last lane.  The wave keeps the
// document [c_lo, c_hi) of the largest key of the step before and asks nothing while the bracket falls into it; otherwise it ranks
// both ends among the starts (64-ary through the fences, wave-uniform addresses) and every lane bisects between the two ranks.
// Keys are < n_text = B[nB - 1] (the caller clamps), so a rank -- the index of the first entry > key -- lies in [1, nB - 1].
struct DocListWave {
    uint64_t c_lo = 1, c_hi = 0;        // wave-uniform; empty at first
    uint32_t r0 = 0, r1 = 0;
    bool shared = false;
    // (all 64 lanes call it; xmin, xmax wave-uniform)
    __device__ __forceinline__ void locate(const DocRef& d, uint64_t xmin, uint64_t xmax)
    {
        shared = xmin >= c_lo && xmax < c_hi;
        if (shared) return;
        r0 = uniform(wave_kary_lower_bound<uint64_t>(d.B, d.BF, 0, d.nB, xmin + 1));
        r1 = uniform(wave_kary_lower_bound<uint64_t>(d.B, d.BF, r0, d.nB, xmax + 1));
        c_hi = d.B[r1];
        c_lo = d.B[r1 - 1];
        shared = r0 == r1;
    }
    __device__ __forceinline__ uint32_t doc(const DocRef& d, uint64_t x) const
    {
        if (shared) return r1 - 1;
        return (uint32_t)vlg::doc_upper_bound(d.B, r0, r1, x) - 1;          // the rank of x lies in [r0, r1]
    }
};

// the document of one position < n_text, one lane on its own (doc_locate_kernel's lookup)
__device__ __forceinline__ uint32_t doc_of_position(const DocRef& d, uint64_t x)
{
    const uint64_t g = vlg::doc_upper_bound(d.BF, 0, d.nB >> 6, x);
    const uint64_t w0 = g << 6, w1 = w0 + 64 < d.nB ? w0 + 64 : d.nB;
    return (uint32_t)vlg::doc_upper_bound(d.B, w0, w1, x) - 1;
}

// The query of the match a wave stands at, carried from step to step (the head pass, and the span pass of match_text.hpp).
// off[0, nq] are the match offsets of the result's queries; q is a query WITH matches, however many empty ones stand around it.
struct QueryCarry {
    uint64_t q = 0, q_end = 0;          // wave-uniform: off[q] <= the match < q_end = off[q + 1]
    // to the query of match g < off[nq]
    __device__ __forceinline__ void seek(const uint64_t* __restrict__ off, uint32_t nq, uint64_t g)
    {
        q = (uint64_t)uniform(wave_kary_lower_bound<uint64_t>(off, 0, nq + 1, g + 1)) - 1;
        q_end = off[q + 1];
    }
    // to the query of match step_end - 1, 64 offsets at a time; border(v, in) sees every offset the wave passes: lane-wise the
    // offset v (~0 behind the last) and whether it lies in front of step_end, i.e. whether a query begins at match v of the step
    template <class F>
    __device__ __forceinline__ void advance(const uint64_t* __restrict__ off, uint32_t nq, uint32_t lane, uint64_t step_end, F&& border)
    {
        while (q_end < step_end) {                                              // wave-uniform; q_end >= the step's first match
            const uint64_t idx = q + 1 + lane;
            const uint64_t v = idx <= nq ? off[idx] : ~0ull;
            const bool in = v < step_end;
            border(v, in);
            q += (uint32_t)__popcll(__ballot(in));                              // at least one; off[q] < step_end <= off[nq]
            q_end = off[q + 1];
        }
    }
};

// One piece of a result as the passes see it: P[0, m) its first positions, `first` the matches of the pieces before it, `pad` its
// place in the padded numbering (doc_list_math.hpp), n_text the sentinel of the documents.
template <typename pos_t>
struct DocListPiece { const pos_t* P; uint64_t m, first, pad, n_text; };

// Head pass.  off[0, nq] are the match offsets of the result's queries (off[nq] = all matches).  bits / run_heads are indexed in the
// padded numbering; ids (null unless the scatter pass reads them) gets the document of every match of the piece; *bad is raised when a
// position is no position of the documents' text (such a key is clamped, so nothing is read out of bounds).
template <typename pos_t>
__global__ void __launch_bounds__(256) doc_heads_kernel(DocListPiece<pos_t> pc, DocRef dr, const uint64_t* __restrict__ off, uint32_t nq,
                                                        uint64_t* __restrict__ bits, uint64_t* __restrict__ run_heads, uint32_t* __restrict__ ids,
                                                        uint32_t* __restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t run = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t run_begin = run * kDocListRun;
    if (run_begin >= pc.m) return;                                              // (whole waves leave)
    const uint64_t run_end = run_begin + kDocListRun < pc.m ? run_begin + kDocListRun : pc.m;
    const uint64_t top = pc.n_text - 1;
    bool any_bad = false;

    // the query of the run's first match: off[q] <= g < off[q + 1] -- a query with matches, however many empty ones stand around it
    const uint64_t g0 = pc.first + run_begin;
    QueryCarry qc;
    qc.seek(off, nq, g0);
    const bool first0 = off[qc.q] == g0;

    DocListWave dw;
    uint32_t carry = ~0u;                                                       // document of the match in front of the step's lane 0
    if (run_begin) {                                                            // (a piece begins with a query: its match 0 is a head anyway)
        uint64_t xp = (uint64_t)pc.P[run_begin - 1];
        if (xp > top) { any_bad = true; xp = top; }
        dw.locate(dr, xp, xp);
        carry = dw.doc(dr, xp);
    }

    uint32_t heads = 0;
    for (uint64_t s = run_begin; s < run_end; s += 64) {
        const uint64_t e = s + lane;
        const bool valid = e < run_end;
        uint64_t x = valid ? (uint64_t)pc.P[e] : 0;
        if (x > top) { any_bad = true; x = top; }
        const uint64_t xmin = wave_min<uint64_t>(valid ? x : ~0ull), xmax = wave_max_u64(x);
        dw.locate(dr, xmin, xmax);
        const uint32_t d = dw.doc(dr, x);
        if (ids && valid) ids[e] = d;

        // query borders inside the step: every offset in [gs, step_end) marks its match as the first of a query
        const uint64_t gs = pc.first + s, step_end = gs + (run_end - s < 64 ? run_end - s : 64);
        uint64_t firsts = s == run_begin && first0 ? 1ull : 0ull;
        qc.advance(off, nq, lane, step_end, [&](uint64_t v, bool in) { firsts |= wave_or_u64(in ? 1ull << (v - gs) : 0ull); });

        uint32_t prev = __shfl_up(d, 1);
        if (lane == 0) prev = carry;
        const bool head = valid && vlg::doclist_head((firsts >> lane) & 1, d, prev);
        const uint64_t word = __ballot(head);
        if (lane == 0) bits[(pc.pad + s) >> 6] = word;
        heads += (uint32_t)__popcll(word);
        carry = __shfl(d, 63);
    }
    if (lane == 0) run_heads[(pc.pad + run_begin) / kDocListRun] = heads;
    if (__any(any_bad) && lane == 0) atomicOr(bad, 1u);
}

// pair_off[q] = head rank of the first match of query q, q in [0, nq]: where its pairs begin
__global__ void __launch_bounds__(256) doc_borders_kernel(const uint64_t* __restrict__ off, uint64_t nq, const uint64_t* __restrict__ piece_first,
                                                          const uint64_t* __restrict__ piece_pad, uint64_t n_pieces, const uint64_t* __restrict__ run_rank,
                                                          const uint64_t* __restrict__ bits, uint64_t* __restrict__ pair_off)
{
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= nq; q += (uint64_t)gridDim.x * blockDim.x)
        pair_off[q] = vlg::doclist_rank_of_match(piece_first, piece_pad, n_pieces, run_rank, bits, kDocListRun, off[q]);
}

// Scatter pass: the heads of a run write (document, match index) at their ranks.  A step without a head reads nothing but its word.
template <typename pos_t>
__global__ void __launch_bounds__(256) doc_scatter_kernel(DocListPiece<pos_t> pc, DocRef dr, const uint64_t* __restrict__ bits,
                                                          const uint64_t* __restrict__ run_rank, const uint32_t* __restrict__ ids,
                                                          uint32_t* __restrict__ docs, uint64_t* __restrict__ first_match)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t run = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t run_begin = run * kDocListRun;
    if (run_begin >= pc.m) return;
    const uint64_t run_end = run_begin + kDocListRun < pc.m ? run_begin + kDocListRun : pc.m;
    const uint64_t top = pc.n_text - 1;
    uint64_t base = run_rank[(pc.pad + run_begin) / kDocListRun];
    for (uint64_t s = run_begin; s < run_end; s += 64) {
        const uint64_t word = bits[(pc.pad + s) >> 6];                          // (bits of valid matches only: the head pass wrote it so)
        if (!word) continue;
        if ((word >> lane) & 1) {
            const uint64_t e = s + lane;
            uint32_t d;
            if (ids) d = ids[e];
            else { const uint64_t x = (uint64_t)pc.P[e]; d = doc_of_position(dr, x < top ? x : top); }
            const uint64_t slot = base + (uint64_t)__popcll(word & ((1ull << lane) - 1));
            docs[slot] = d;
            first_match[slot] = pc.first + e;
        }
        base += (uint64_t)__popcll(word);
    }
}

// device memory of a listing and of its making, back to the cache of the result buffers when it goes
struct CachedBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
    CachedBuf() = default;
    CachedBuf(const CachedBuf&) = delete;
    CachedBuf& operator=(const CachedBuf&) = delete;
    ~CachedBuf() { if (p) result_cache().give(p, bytes); }
    hipError_t alloc(uint64_t need) { return result_alloc(&p, need ? need : 256, &bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

struct vlg_doc_listing {
    uint64_t nq = 0, n_pairs = 0;
    bool has_pairs = false;
    std::vector<uint64_t> match_off;     // host, [nq + 1]: closes the count of a query's last pair
    CachedBuf pair_off;                  // [nq + 1] uint64_t (none when the result had no match)
    CachedBuf docs;                      // [n_pairs] uint32_t
    CachedBuf first_match;               // [n_pairs] uint64_t
};

namespace {

template <typename pos_t>
void doc_list_launch_heads(const ResultPiece& p, uint64_t first, uint64_t pad, const vlg_documents* d, const uint64_t* d_off, uint32_t nq, uint64_t* bits,
                           uint64_t* run_heads, uint32_t* ids, uint32_t* bad)
{
    const uint64_t runs = vlg::doclist_runs(p.matches, kDocListRun);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(doc_heads_kernel<pos_t>), dim3((uint32_t)((runs + 3) / 4)), dim3(256), 0, (hipStream_t) nullptr,
                       DocListPiece<pos_t>{static_cast<const pos_t*>(p.d_first), p.matches, first, pad, d->n_text},
                       DocRef{d->d_starts, d->d_fences, (uint32_t)(d->n_docs + 1), nullptr}, d_off, nq, bits, run_heads, ids, bad);
}
template <typename pos_t>
void doc_list_launch_scatter(const ResultPiece& p, uint64_t first, uint64_t pad, const vlg_documents* d, const uint64_t* bits, const uint64_t* run_rank,
                             const uint32_t* ids, uint32_t* docs, uint64_t* first_match)
{
    const uint64_t runs = vlg::doclist_runs(p.matches, kDocListRun);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(doc_scatter_kernel<pos_t>), dim3((uint32_t)((runs + 3) / 4)), dim3(256), 0, (hipStream_t) nullptr,
                       DocListPiece<pos_t>{static_cast<const pos_t*>(p.d_first), p.matches, first, pad, d->n_text},
                       DocRef{d->d_starts, d->d_fences, (uint32_t)(d->n_docs + 1), nullptr}, bits, run_rank, ids, docs, first_match);
}

}  // namespace

extern "C" vlg_status vlg_result_list_documents(const vlg_result* r, const vlg_documents* d, int what, vlg_doc_listing** out)
{
    if (!r || !d || !out) return fail(VLG_E_INVALID, "null argument");
    if (what != VLG_DOCLIST_DF && what != VLG_DOCLIST_PAIRS) return fail(VLG_E_INVALID, "vlg_result_list_documents: what is VLG_DOCLIST_DF or VLG_DOCLIST_PAIRS");
    if (!r->owned.empty()) return fail(VLG_E_UNSUPPORTED, "vlg_result_list_documents: the result of a collective search holds only part of the queries");
    const uint64_t nq = r->counts.size();
    if (nq >= 0xFFFFFFFFull) return fail(VLG_E_UNSUPPORTED, "vlg_result_list_documents: more than 2^32 - 2 queries");
    std::unique_ptr<vlg_doc_listing> l(new (std::nothrow) vlg_doc_listing);
    if (!l) return fail(VLG_E_OOM, "host allocation");
    l->nq = nq;
    l->has_pairs = what == VLG_DOCLIST_PAIRS;
    l->match_off.resize(nq + 1);
    l->match_off[0] = 0;
    for (uint64_t q = 0; q < nq; ++q) l->match_off[q + 1] = l->match_off[q] + r->counts[q];
    const uint64_t M = l->match_off[nq];

    // the pieces that hold matches, laid end to end (doc_list_math.hpp); a piece begins with a query
    std::vector<const ResultPiece*> pieces;
    std::vector<uint64_t> piece_m;
    for (const auto& p : r->pieces)
        if (p.matches) { pieces.push_back(&p); piece_m.push_back(p.matches); }
    const uint64_t np = pieces.size();
    std::vector<uint64_t> lay(2 * (np + 1));
    uint64_t* first = lay.data();
    uint64_t* pad = first + np + 1;
    vlg::doclist_layout(piece_m.data(), np, kDocListRun, first, pad);
    if (first[np] != M) return fail(VLG_E_INTERNAL, "vlg_result_list_documents: the pieces of the result do not add up to its counts");
    for (uint64_t k = 0; k < np; ++k) {
        if (pieces[k]->width != 4 && pieces[k]->width != 8) return fail(VLG_E_INTERNAL, "vlg_result_list_documents: positions of an unknown width");
        if (!std::binary_search(l->match_off.begin(), l->match_off.end(), first[k]))
            return fail(VLG_E_INTERNAL, "vlg_result_list_documents: a piece of the result begins inside a query");
    }
    if (!M) { *out = l.release(); return VLG_OK; }                             // nothing to launch: zero pairs

    const uint64_t n_runs = pad[np] / kDocListRun, n_words = pad[np] / 64;
    static const bool store_ids = [] { const char* e = getenv("VLG_DOCLIST_STORE_IDS"); return e && atoi(e) != 0; }();
    const bool use_ids = store_ids && l->has_pairs;

    // scratch, one block: [run_rank: n_runs + 1][flag][bits: n_words][match offsets: nq + 1][piece first, pad: 2 (np + 1)], all 8 bytes wide
    const uint64_t o_flag = n_runs + 1, o_bits = o_flag + 1, o_off = o_bits + n_words, o_lay = o_off + nq + 1, n_scratch = o_lay + 2 * (np + 1);
    CachedBuf scratch, ids, scan_tmp;
    VLG_HIP_TRY(scratch.alloc(n_scratch * 8));
    uint64_t* const d_scr = scratch.as<uint64_t>();
    uint64_t* const d_rank = d_scr;
    uint32_t* const d_bad = reinterpret_cast<uint32_t*>(d_scr + o_flag);
    if (use_ids) VLG_HIP_TRY(ids.alloc(M * 4));
    VLG_HIP_TRY(hipMemsetAsync(d_scr + n_runs, 0, 16, nullptr));               // the entry behind the last run (the scan makes it the total) and the flag
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + o_off, l->match_off.data(), (nq + 1) * 8, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + o_lay, lay.data(), lay.size() * 8, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));                                // (the host vectors were pageable)

    for (uint64_t k = 0; k < np; ++k) {
        uint32_t* const pids = use_ids ? ids.as<uint32_t>() + first[k] : nullptr;
        if (pieces[k]->width == 4) doc_list_launch_heads<uint32_t>(*pieces[k], first[k], pad[k], d, d_scr + o_off, (uint32_t)nq, d_scr + o_bits, d_rank, pids, d_bad);
        else doc_list_launch_heads<uint64_t>(*pieces[k], first[k], pad[k], d, d_scr + o_off, (uint32_t)nq, d_scr + o_bits, d_rank, pids, d_bad);
        VLG_HIP_TRY(hipGetLastError());
    }
    {
        size_t tmp_bytes = 0;
        VLG_HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, d_rank, d_rank, 0ull, n_runs + 1, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        VLG_HIP_TRY(scan_tmp.alloc(tmp_bytes));
        VLG_HIP_TRY(rocprim::exclusive_scan(scan_tmp.p, tmp_bytes, d_rank, d_rank, 0ull, n_runs + 1, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    }
    uint64_t back[2] = {0, 0};                                                  // the number of pairs and the flag, read back together
    VLG_HIP_TRY(hipMemcpy(back, d_scr + n_runs, 16, hipMemcpyDeviceToHost));
    if ((uint32_t)back[1])
        return fail(VLG_E_INVALID, "vlg_result_list_documents: a match begins at or behind the documents' text length " + std::to_string(d->n_text) +
                                       " (documents of another text)");
    l->n_pairs = back[0];

    VLG_HIP_TRY(l->pair_off.alloc((nq + 1) * 8));
    hipLaunchKernelGGL(doc_borders_kernel, launch_grid(nq + 1, 4096), dim3(256), 0, (hipStream_t) nullptr, d_scr + o_off, nq, d_scr + o_lay, d_scr + o_lay + np + 1, np,
                       d_rank, d_scr + o_bits, l->pair_off.as<uint64_t>());
    VLG_HIP_TRY(hipGetLastError());
    if (l->has_pairs) {
        VLG_HIP_TRY(l->docs.alloc(l->n_pairs * 4));
        VLG_HIP_TRY(l->first_match.alloc(l->n_pairs * 8));
        for (uint64_t k = 0; k < np; ++k) {
            const uint32_t* const pids = use_ids ? ids.as<uint32_t>() + first[k] : nullptr;
            if (pieces[k]->width == 4)
                doc_list_launch_scatter<uint32_t>(*pieces[k], first[k], pad[k], d, d_scr + o_bits, d_rank, pids, l->docs.as<uint32_t>(), l->first_match.as<uint64_t>());
            else
                doc_list_launch_scatter<uint64_t>(*pieces[k], first[k], pad[k], d, d_scr + o_bits, d_rank, pids, l->docs.as<uint32_t>(), l->first_match.as<uint64_t>());
            VLG_HIP_TRY(hipGetLastError());
        }
    }
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));                                // the listing is there; the scratch goes back
    *out = l.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_doc_listing_info(const vlg_doc_listing* l, uint64_t* n_queries, uint64_t* n_pairs)
{
    if (!l) return fail(VLG_E_INVALID, "null argument");
    if (n_queries) *n_queries = l->nq;
    if (n_pairs) *n_pairs = l->n_pairs;
    return VLG_OK;
}

extern "C" vlg_status vlg_doc_listing_fetch(const vlg_doc_listing* l, uint64_t* h_df, uint64_t* h_offsets, uint64_t* h_docs, uint64_t* h_counts,
                                            uint64_t* h_first_match)
{
    if (!l) return fail(VLG_E_INVALID, "null argument");
    if ((h_docs || h_counts || h_first_match) && !l->has_pairs)
        return fail(VLG_E_INVALID, "vlg_doc_listing_fetch: the listing was made with VLG_DOCLIST_DF and holds no pairs");
    const uint64_t nq = l->nq, np = l->n_pairs;
    std::vector<uint64_t> po;
    if (h_df || h_counts || (h_offsets && !l->pair_off.p)) po.assign(nq + 1, 0);
    uint64_t* const off = po.empty() ? h_offsets : po.data();
    if (off && l->pair_off.p) VLG_HIP_TRY(hipMemcpy(off, l->pair_off.p, (nq + 1) * 8, hipMemcpyDeviceToHost));
    if (h_offsets && h_offsets != off) memcpy(h_offsets, off, (nq + 1) * 8);
    if (h_df) for (uint64_t q = 0; q < nq; ++q) h_df[q] = off[q + 1] - off[q];
    if (!np) return VLG_OK;
    if (h_docs) {                                                              // 4 bytes per pair cross the bus
        std::vector<uint32_t> narrow(np);
        VLG_HIP_TRY(hipMemcpy(narrow.data(), l->docs.p, np * 4, hipMemcpyDeviceToHost));
        std::copy(narrow.begin(), narrow.end(), h_docs);
    }
    if (h_first_match || h_counts) {
        std::vector<uint64_t> fm;
        if (!h_first_match) fm.resize(np);
        uint64_t* const f = h_first_match ? h_first_match : fm.data();
        VLG_HIP_TRY(hipMemcpy(f, l->first_match.p, np * 8, hipMemcpyDeviceToHost));
        if (h_counts) vlg::doclist_counts(l->match_off.data(), off, nq, f, h_counts);
    }
    return VLG_OK;
}

extern "C" void vlg_doc_listing_destroy(vlg_doc_listing* l) { delete l; }
