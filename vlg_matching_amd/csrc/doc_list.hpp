// Document listing: which documents each query of a result matches, and how often -- vlg_result_list_documents, vlg_doc_listing_*
// (include/vlg_hip.h).  Part of search.hip's translation unit: the head rule at work, the three listing kernels, the handle and its fetch.
// result_passes.hpp holds what the passes share with the other consumers of a result, doc_list_math.hpp the arithmetic that is not wave code.
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
#include "result_passes.hpp"

namespace {

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
    const WaveRun w(0, pc.m);
    if (w.empty()) return;
    const uint32_t lane = w.lane;
    const uint64_t top = pc.n_text - 1;
    bool any_bad = false;

    // the query of the run's first match: off[q] <= g < off[q + 1] -- a query with matches, however many empty ones stand around it
    const uint64_t g0 = pc.first + w.begin;
    QueryCarry qc;
    qc.seek(off, nq, g0);
    const bool first0 = off[qc.q] == g0;

    DocWave dw;
    uint32_t carry = ~0u;                                                       // document of the match in front of the step's lane 0
    if (w.begin) {                                                            // (a piece begins with a query: its match 0 is a head anyway)
        uint64_t xp = (uint64_t)pc.P[w.begin - 1];
        if (xp > top) { any_bad = true; xp = top; }
        dw.locate(dr, xp, xp);
        carry = dw.doc(dr, xp);
    }

    uint32_t heads = 0;
    for (uint64_t s = w.begin; s < w.end; s += 64) {
        const uint64_t e = s + lane;
        const bool valid = e < w.end;
        uint64_t x = valid ? (uint64_t)pc.P[e] : 0;
        if (x > top) { any_bad = true; x = top; }
        const uint64_t xmin = wave_min<uint64_t>(valid ? x : ~0ull), xmax = wave_max<uint64_t>(x);
        dw.locate(dr, xmin, xmax);
        const uint32_t d = dw.doc(dr, x);
        if (ids && valid) ids[e] = d;

        // query borders inside the step: every offset in [gs, step_end) marks its match as the first of a query
        const uint64_t gs = pc.first + s, step_end = gs + (w.end - s < 64 ? w.end - s : 64);
        uint64_t firsts = s == w.begin && first0 ? 1ull : 0ull;
        qc.advance(off, nq, lane, step_end, [&](uint64_t v, bool in) { firsts |= wave_or<uint64_t>(in ? 1ull << (v - gs) : 0ull); });

        uint32_t prev = __shfl_up(d, 1);
        if (lane == 0) prev = carry;
        const bool head = valid && vlg::doclist_head((firsts >> lane) & 1, d, prev);
        const uint64_t word = __ballot(head);
        if (lane == 0) bits[(pc.pad + s) >> 6] = word;
        heads += (uint32_t)__popcll(word);
        carry = __shfl(d, 63);
    }
    if (lane == 0) run_heads[(pc.pad + w.begin) / kDocListRun] = heads;
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
    const WaveRun w(0, pc.m);
    if (w.empty()) return;
    const uint32_t lane = w.lane;
    const uint64_t top = pc.n_text - 1;
    uint64_t base = run_rank[(pc.pad + w.begin) / kDocListRun];
    for (uint64_t s = w.begin; s < w.end; s += 64) {
        const uint64_t word = bits[(pc.pad + s) >> 6];                          // (bits of valid matches only: the head pass wrote it so)
        if (!word) continue;
        if ((word >> lane) & 1) {
            const uint64_t e = s + lane;
            uint32_t d;
            if (ids) d = ids[e];
            else { const uint64_t x = (uint64_t)pc.P[e]; d = (uint32_t)doc_rank_dev(dr, x < top ? x : top) - 1; }
            const uint64_t slot = base + (uint64_t)__popcll(word & ((1ull << lane) - 1));
            docs[slot] = d;
            first_match[slot] = pc.first + e;
        }
        base += (uint64_t)__popcll(word);
    }
}

}  // namespace

struct vlg_doc_listing {
    uint64_t nq = 0, n_pairs = 0;
    bool has_pairs = false;
    std::vector<uint64_t> match_off;     // host, [nq + 1]: closes the count of a query's last pair
    CachedBuf pair_off;                  // [nq + 1] uint64_t (none when the result had no match)
    CachedBuf docs;                      // [n_pairs] uint32_t
    CachedBuf first_match;               // [n_pairs] uint64_t
};

extern "C" vlg_status vlg_result_list_documents(const vlg_result* r, const vlg_documents* d, int what, vlg_doc_listing** out)
{
    if (!r || !d || !out) return fail(VLG_E_INVALID, "null argument");
    if (what != VLG_DOCLIST_DF && what != VLG_DOCLIST_PAIRS) return fail(VLG_E_INVALID, "vlg_result_list_documents: what is VLG_DOCLIST_DF or VLG_DOCLIST_PAIRS");
    ResultView v;
    if (vlg_status s = v.build(r, "vlg_result_list_documents")) return s;
    std::unique_ptr<vlg_doc_listing> l(new (std::nothrow) vlg_doc_listing);
    if (!l) return fail(VLG_E_OOM, "host allocation");
    const uint64_t nq = l->nq = v.nq, np = v.np, M = v.matches();
    l->has_pairs = what == VLG_DOCLIST_PAIRS;
    const auto done = [&] { l->match_off = std::move(v.off); *out = l.release(); return VLG_OK; };
    if (!M) return done();                                                     // nothing to launch: zero pairs

    const uint64_t n_runs = v.pad(np) / kDocListRun, n_words = v.pad(np) / 64;
    static const bool store_ids = [] { const char* e = getenv("VLG_DOCLIST_STORE_IDS"); return e && atoi(e) != 0; }();
    const bool use_ids = store_ids && l->has_pairs;

    // scratch, one block: [run_rank: n_runs + 1][flag][bits: n_words][match offsets: nq + 1][piece first, pad: 2 (np + 1)], all 8 bytes wide
    const uint64_t o_flag = n_runs + 1, o_bits = o_flag + 1, o_off = o_bits + n_words, o_lay = o_off + nq + 1, n_scratch = o_lay + 2 * (np + 1);
    CachedBuf scratch, ids;
    VLG_HIP_TRY(scratch.alloc(n_scratch * 8));
    uint64_t* const d_scr = scratch.as<uint64_t>();
    uint64_t* const d_rank = d_scr;
    uint32_t* const d_bad = reinterpret_cast<uint32_t*>(d_scr + o_flag);
    if (use_ids) VLG_HIP_TRY(ids.alloc(M * 4));
    VLG_HIP_TRY(hipMemsetAsync(d_scr + n_runs, 0, 16, nullptr));               // the entry behind the last run (the scan makes it the total) and the flag
    VLG_HIP_TRY(v.upload_off(d_scr + o_off));
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + o_lay, v.lay.data(), v.lay.size() * 8, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));                                // (the host vectors were pageable)

    // pass(piece, its place in ids) for every piece, in the type of its positions
    const DocRef dr = doc_ref(d);
    const auto per_piece = [&](auto&& pass) -> vlg_status {
        for (uint64_t k = 0; k < np; ++k) {
            const ResultPiece& p = *v.pieces[k];
            with_piece_type(p, [&](auto t) {
                pass(DocListPiece<decltype(t)>{static_cast<const decltype(t)*>(p.d_first), p.matches, v.first(k), v.pad(k), d->n_text},
                     use_ids ? ids.as<uint32_t>() + v.first(k) : nullptr);
            });
            VLG_HIP_TRY(hipGetLastError());
        }
        return VLG_OK;
    };
    if (vlg_status s = per_piece([&](auto pc, uint32_t* pids) {
            hipLaunchKernelGGL(doc_heads_kernel, run_grid(pc.m), dim3(256), 0, (hipStream_t) nullptr, pc, dr, d_scr + o_off, (uint32_t)nq, d_scr + o_bits, d_rank, pids, d_bad);
        })) return s;
    uint64_t back[2] = {0, 0};                                                  // the number of pairs and the flag
    if (vlg_status s = scan_with_total(d_rank, n_runs, back)) return s;
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
        if (vlg_status s = per_piece([&](auto pc, const uint32_t* pids) {
                hipLaunchKernelGGL(doc_scatter_kernel, run_grid(pc.m), dim3(256), 0, (hipStream_t) nullptr, pc, dr, d_scr + o_bits, d_rank, pids, l->docs.as<uint32_t>(),
                                   l->first_match.as<uint64_t>());
            })) return s;
    }
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));                                // the listing is there; the scratch goes back
    return done();
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
