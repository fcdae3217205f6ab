// Match texts: what every match of a result matched, extracted on the device -- vlg_result_extract_matches, vlg_match_texts_*
// (include/vlg_hip.h).  Part of search.hip's translation unit: the span kernel, the tuple and last-symbol preparation, the handle and its
// fetch.  result_passes.hpp holds what the span pass shares with the other consumers of a result, match_span.hpp the rule.
//
// The first positions and the tuples of a result lie in HBM beside the document starts, and a text access gives any text range back.
// Three steps turn the matches [match_begin, match_end) of the fetch numbering into their texts:
//   spans   : element-parallel -- the matches of the slice that a piece holds are dealt to waves in runs of kDocListRun, 64 per step
//             (WaveRun).  A lane finds its query (QueryCarry: the wave carries the query of the step's first
//             match and passes the offsets up to the step's last; a step that leaves its query lets the lanes bisect between the two),
//             reads p0 and, where k > 1, the match's last tuple value, finds the document of p0 (DocWave, as the listing's head pass does)
//             and writes b, the inclusive end e - 1 and the length e - b.  A core that is none of the text is counted, not extracted.
//   scan    : one exclusive scan of the lengths (rocPRIM) gives the out-offsets; its last entry is the number of symbols, read back
//             once together with the counter.
//   extract : vlg_extract_batch over the three device arrays.
// Scratch of this entry beyond the outputs: the inclusive ends and four per-query arrays (match offsets, k, symbols of the last
// sub-pattern, tuple base inside the piece) -- from result_alloc, returned.  vlg_extract_batch brings its own: segment counts from
// hipMalloc / hipFree on every call, a scan, a read-back and two synchronisations of its own (part of the fixed cost).
#include "match_span.hpp"
#include "result_passes.hpp"

namespace {

// What the span pass sees of one piece: P its first positions, T its tuples (null: none were materialised, and no query with k > 1
// has a match in the slice), `first` the matches of the pieces before it, [a, b) the matches of the piece that belong to the slice,
// out0 the place of match a in the slice.
template <typename pos_t>
struct SpanPiece { const pos_t* P; const pos_t* T; uint64_t first, a, b, out0; };
// per query: match offsets off[0, nq], sub-patterns k, symbols of the last one, where its tuples begin inside its piece
struct SpanQueries { const uint64_t* off; const uint64_t* m_last; const uint64_t* tbase; const uint32_t* k; uint32_t nq; };
struct SpanRule { uint64_t n_text, fl, fr; };

// begin / last / len are indexed by the match's place in the slice; *bad counts the cores that are none of the text (such a match
// gets the range [0, 1), so that nothing downstream reads out of bounds before the host has seen the counter).  dr.B null: no documents.
template <typename pos_t>
__global__ void __launch_bounds__(256) match_span_kernel(SpanPiece<pos_t> pc, SpanQueries sq, DocRef dr, SpanRule rule, uint64_t* __restrict__ begin,
                                                         uint64_t* __restrict__ last, uint64_t* __restrict__ len, unsigned long long* __restrict__ bad)
{
    const WaveRun w(pc.a, pc.b);
    if (w.empty()) return;
    const uint32_t lane = w.lane;
    const uint64_t top = rule.n_text - 1;                                       // (documents: n_text >= 1)

    QueryCarry qc;
    qc.seek(sq.off, sq.nq, pc.first + w.begin);
    DocWave dw;
    uint32_t n_bad = 0;
    for (uint64_t s = w.begin; s < w.end; s += 64) {
        const uint64_t n_step = w.end - s < 64 ? w.end - s : 64;
        const bool valid = lane < n_step;
        const uint64_t e = s + (valid ? lane : n_step - 1);                     // (a lane behind the run repeats its last match)
        const uint64_t g = pc.first + e, step_end = pc.first + s + n_step;

        // the lane's query: the carried one while the step stays inside it, else between it and the query of the step's last match
        const uint64_t q_lo = qc.q;
        qc.advance(sq.off, sq.nq, lane, step_end, [](uint64_t, bool) {});
        const uint64_t q = q_lo == qc.q ? q_lo : vlg::doc_upper_bound(sq.off, q_lo + 1, qc.q + 1, g) - 1;

        const uint64_t p0 = (uint64_t)pc.P[e];
        const uint32_t k = sq.k[q];
        uint64_t pl = p0;
        if (k > 1 && pc.T) pl = (uint64_t)pc.T[sq.tbase[q] + (g - sq.off[q]) * k + (k - 1)];
        const uint64_t ce = vlg::match_core_end(pl, sq.m_last[q]);
        const bool ok = vlg::match_core_ok(p0, ce, rule.n_text);

        uint64_t B0 = 0, B1 = rule.n_text;
        if (dr.B) {                                                             // wave-uniform
            const uint64_t x = p0 < top ? p0 : top;                             // (a position behind the text is not ok anyway)
            dw.locate(dr, wave_min<uint64_t>(x), wave_max<uint64_t>(x));
            if (dw.shared) { B0 = dw.c_lo; B1 = dw.c_hi; }
            else { const uint32_t d = dw.doc(dr, x); B0 = dr.B[d]; B1 = dr.B[d + 1]; }
        }
        vlg::MatchSpan sp = vlg::match_span(p0, ce, B0, B1, rule.fl, rule.fr);
        if (!ok) { sp.b = 0; sp.e = 1; }
        if (valid) {
            const uint64_t o = pc.out0 + (e - pc.a);
            begin[o] = sp.b;
            last[o] = sp.e - 1;
            len[o] = sp.e - sp.b;
        }
        n_bad += (uint32_t)__popcll(__ballot(valid && !ok));
    }
    if (n_bad && lane == 0) atomicAdd(bad, (unsigned long long)n_bad);
}

}  // namespace

struct vlg_match_texts {
    uint64_t n_matches = 0, n_symbols = 0;
    uint32_t sym_bytes = 1;
    CachedBuf meta;                      // [begin: n_matches][offsets: n_matches + 1][counter] uint64_t (none for an empty slice)
    CachedBuf symbols;                   // [n_symbols] of sym_bytes
};

extern "C" vlg_status vlg_result_extract_matches(const vlg_result* r, const vlg_queries* q, const vlg_text_access* t, const vlg_documents* docs,
                                                 uint64_t flank_left, uint64_t flank_right, uint64_t match_begin, uint64_t match_end,
                                                 uint64_t max_symbols, vlg_match_texts** out)
{
    static const char* const fn = "vlg_result_extract_matches: ";
    if (!r || !q || !t || !out) return fail(VLG_E_INVALID, "null argument");
    ResultView v;
    if (vlg_status s = v.build(r, "vlg_result_extract_matches")) return s;
    const uint64_t nq = v.nq, np = v.np, M = v.matches();
    const uint64_t* const off = v.off.data();
    const uint64_t* const first = v.lay.data();                                 // [np + 1]
    if (q->nq != nq || q->qsub.size() != nq + 1 || r->k.size() != nq)
        return fail(VLG_E_INVALID, std::string(fn) + "the batch has " + std::to_string(q->nq) + " queries, the result " + std::to_string(nq));
    for (uint64_t i = 0; i < nq; ++i)
        if (q->qsub[i + 1] - q->qsub[i] != r->k[i])
            return fail(VLG_E_INVALID, std::string(fn) + "query " + std::to_string(i) + " of the batch has " + std::to_string(q->qsub[i + 1] - q->qsub[i]) +
                                           " sub-patterns, that of the result " + std::to_string(r->k[i]));
    const vlg_index* idx = t->idx;
    const uint32_t sym_bytes = idx->is_int ? 4u : 1u;
    if (q->sym_bytes != sym_bytes)
        return fail(VLG_E_INVALID, std::string(fn) + (idx->is_int ? "a byte batch on the text of an integer index" : "an integer batch on the text of a byte index"));
    if (q->nsub && q->suboff.size() != q->nsub + 1) return fail(VLG_E_INVALID, std::string(fn) + "the batch carries no sub-pattern lengths");
    const uint64_t n_text = idx->hdr.n - 1;                                     // the sentinel is not text
    if (docs && docs->n_text != n_text)
        return fail(VLG_E_INVALID, std::string(fn) + "documents of a text of " + std::to_string(docs->n_text) + " symbols, the text access has " +
                                       std::to_string(n_text));

    if (match_end == ~0ull) match_end = M;
    if (match_begin > match_end) return fail(VLG_E_INVALID, std::string(fn) + "match_begin > match_end");
    if (match_end > M) return fail(VLG_E_INVALID, std::string(fn) + "match_end " + std::to_string(match_end) + " beyond the " + std::to_string(M) + " matches");
    const uint64_t ns = match_end - match_begin;

    // a piece stores all the tuples of its queries or none
    std::vector<uint64_t> m_last(nq), tbase(nq);
    for (uint64_t i = 0; i < nq; ++i) m_last[i] = vlg::match_last_symbols(q->suboff.data(), q->qsub[i], q->qsub[i + 1], sym_bytes);
    vlg::match_tuple_bases(off, r->k.data(), nq, first, np, tbase.data());
    for (uint64_t i = 0, j = 0; i < nq; ++i) {                                  // (j: the piece of query i, where it has matches)
        if (off[i + 1] == off[i]) continue;
        while (j + 1 < np && off[i] >= first[j + 1]) ++j;
        const uint64_t tv = v.pieces[j]->tuple_vals;
        if (tv) {
            if (tbase[i] + r->counts[i] * r->k[i] > tv) return fail(VLG_E_INTERNAL, std::string(fn) + "the tuples of a piece are fewer than its counts say");
        } else if (r->k[i] > 1 && off[i] < match_end && off[i + 1] > match_begin)      // (the span pass depends on this refusal: without
                                                                                     //  tuples it takes pl = p0 for every lane)
            return fail(VLG_E_INVALID, std::string(fn) + "tuples were not materialised (workspace option \"tuples\" is 0) and query " + std::to_string(i) +
                                           ", which has matches in the slice, has " + std::to_string(r->k[i]) + " sub-patterns");
    }

    std::unique_ptr<vlg_match_texts> m(new (std::nothrow) vlg_match_texts);
    if (!m) return fail(VLG_E_OOM, "host allocation");
    m->n_matches = ns;
    m->sym_bytes = sym_bytes;
    if (!ns) { *out = m.release(); return VLG_OK; }                            // nothing to launch: zero texts

    // handle: [begin: ns][offsets: ns + 1][counter]; scratch: [last: ns][off: nq + 1][m_last: nq][tbase: nq][k: nq, 4 bytes each]
    const uint64_t o_off = ns, o_bad = o_off + ns + 1;
    const uint64_t s_off = ns, s_ml = s_off + nq + 1, s_tb = s_ml + nq, s_k = s_tb + nq;
    CachedBuf scratch;
    VLG_HIP_TRY(m->meta.alloc((o_bad + 1) * 8));
    VLG_HIP_TRY(scratch.alloc(s_k * 8 + nq * 4));
    uint64_t* const d_meta = m->meta.as<uint64_t>();
    uint64_t* const d_scr = scratch.as<uint64_t>();
    VLG_HIP_TRY(hipMemsetAsync(d_meta + o_off + ns, 0, 16, nullptr));          // the entry behind the last length (the scan makes it the total) and the counter
    VLG_HIP_TRY(v.upload_off(d_scr + s_off));
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + s_ml, m_last.data(), nq * 8, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + s_tb, tbase.data(), nq * 8, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipMemcpyAsync(d_scr + s_k, r->k.data(), nq * 4, hipMemcpyHostToDevice, nullptr));
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));                                // (the host vectors were pageable)

    const SpanQueries sq{d_scr + s_off, d_scr + s_ml, d_scr + s_tb, reinterpret_cast<const uint32_t*>(d_scr + s_k), (uint32_t)nq};
    const SpanRule rule{n_text, flank_left, flank_right};
    unsigned long long* const d_bad = reinterpret_cast<unsigned long long*>(d_meta + o_bad);
    const DocRef dr = doc_ref(docs);
    for (uint64_t j = 0; j < np; ++j) {
        const uint64_t a = std::max(match_begin, first[j]), b = std::min(match_end, first[j + 1]);
        if (a >= b) continue;
        const ResultPiece& p = *v.pieces[j];
        with_piece_type(p, [&](auto t) {
            using pos_t = decltype(t);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(match_span_kernel<pos_t>), run_grid(b - a), dim3(256), 0, (hipStream_t) nullptr,
                               SpanPiece<pos_t>{static_cast<const pos_t*>(p.d_first), static_cast<const pos_t*>(p.d_tuples), first[j], a - first[j], b - first[j],
                                                a - match_begin},
                               sq, dr, rule, d_meta, d_scr, d_meta + o_off, d_bad);
        });
        VLG_HIP_TRY(hipGetLastError());
    }
    uint64_t back[2] = {0, 0};                                                  // the number of symbols and the counter
    if (vlg_status s = scan_with_total(d_meta + o_off, ns, back)) return s;
    if (back[1])
        return fail(VLG_E_INVALID, std::string(fn) + std::to_string(back[1]) + " match(es) of the slice do not end inside the text of " + std::to_string(n_text) +
                                       " symbols (queries or a text access that do not belong to this result)");
    if (max_symbols && back[0] > max_symbols)
        return fail(VLG_E_WORKSPACE, std::string(fn) + "the texts of the slice have " + std::to_string(back[0]) + " symbols, max_symbols is " +
                                         std::to_string(max_symbols));
    m->n_symbols = back[0];
    VLG_HIP_TRY(m->symbols.alloc(m->n_symbols * sym_bytes));
    if (vlg_status s = vlg_extract_batch(t, d_meta, d_scr, d_meta + o_off, ns, m->n_symbols, m->symbols.p, nullptr)) return s;   // (synchronises)
    *out = m.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_match_texts_info(const vlg_match_texts* m, uint64_t* n_matches, uint64_t* n_symbols, uint32_t* symbol_bytes)
{
    if (!m) return fail(VLG_E_INVALID, "null argument");
    if (n_matches) *n_matches = m->n_matches;
    if (n_symbols) *n_symbols = m->n_symbols;
    if (symbol_bytes) *symbol_bytes = m->sym_bytes;
    return VLG_OK;
}

extern "C" vlg_status vlg_match_texts_fetch(const vlg_match_texts* m, uint64_t* h_offsets, uint64_t* h_begin, void* h_symbols)
{
    if (!m) return fail(VLG_E_INVALID, "null argument");
    const uint64_t ns = m->n_matches;
    if (!ns) { if (h_offsets) h_offsets[0] = 0; return VLG_OK; }
    if (h_begin) VLG_HIP_TRY(hipMemcpy(h_begin, m->meta.as<uint64_t>(), ns * 8, hipMemcpyDeviceToHost));
    if (h_offsets) VLG_HIP_TRY(hipMemcpy(h_offsets, m->meta.as<uint64_t>() + ns, (ns + 1) * 8, hipMemcpyDeviceToHost));
    if (h_symbols && m->n_symbols) VLG_HIP_TRY(hipMemcpy(h_symbols, m->symbols.p, m->n_symbols * m->sym_bytes, hipMemcpyDeviceToHost));
    return VLG_OK;
}

extern "C" void vlg_match_texts_destroy(vlg_match_texts* m) { delete m; }
