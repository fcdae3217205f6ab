// Match texts (vlg_result_extract_matches): which text range a match stands for.  Plain C++ (no HIP header): the span pass of
// match_text.hpp calls it on the device, the entry point on the host, and a CPU test compiles it alone (tests/match_span_check.cpp).
//
// The matches of a result are numbered as vlg_result_fetch returns them.  For match i of query q
//   p0     its first position;  pl the position of its last sub-pattern (its last tuple value; p0 when k(q) = 1)
//   m_last the number of SYMBOLS of q's last sub-pattern                                                      (match_last_symbols)
//   core   [p0, ce) with ce = pl + m_last                                                                     (match_core_end)
//   bounds [B0, B1): [0, n_text) without documents, otherwise the document of p0 (a match belongs to the document of its FIRST
//          position, as in the listing)
// and with the flanks fl, fr the extracted range is [b, e)                                                    (match_span):
//   b = p0 - min(fl, p0 - min(p0, B0))         e = ce + min(fr, max(B1, ce) - ce)
// The core is never cut; the flanks stop at the bounds; a core that reaches over B1 (a result of a search without documents, looked
// at through documents) keeps itself and gets no right flank.  A flank of UINT64_MAX means "to the bound".  A core is one of the text
// iff p0 < ce <= n_text (match_core_ok): anything else says that the queries or the text do not belong to the result.
// All arithmetic in uint64_t, nothing wraps: sums saturate, differences are taken on the side known to be the larger one.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VLG_MS_HD __host__ __device__ __forceinline__
#else
#define VLG_MS_HD inline
#endif

namespace vlg {

VLG_MS_HD uint64_t span_sat_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s < a ? ~0ull : s; }
VLG_MS_HD uint64_t span_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
VLG_MS_HD uint64_t span_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// symbols of the last sub-pattern of a query that owns the sub-patterns [s0, s1) of a batch: suboff counts bytes of the blob (the
// positions of a class batch are one byte each), sym_bytes of them make a symbol.  A query without sub-patterns has none.
VLG_MS_HD uint64_t match_last_symbols(const uint64_t* suboff, uint64_t s0, uint64_t s1, uint64_t sym_bytes)
{
    return s1 > s0 ? (suboff[s1] - suboff[s1 - 1]) / sym_bytes : 0;
}

VLG_MS_HD uint64_t match_core_end(uint64_t pl, uint64_t m_last) { return span_sat_add(pl, m_last); }
VLG_MS_HD bool match_core_ok(uint64_t p0, uint64_t ce, uint64_t n_text) { return p0 < ce && ce <= n_text; }

struct MatchSpan { uint64_t b, e; };     // [b, e), never empty for a core that is one

VLG_MS_HD MatchSpan match_span(uint64_t p0, uint64_t ce, uint64_t B0, uint64_t B1, uint64_t fl, uint64_t fr)
{
    MatchSpan s;
    s.b = p0 - span_min(fl, p0 - span_min(p0, B0));
    s.e = ce + span_min(fr, span_max(B1, ce) - ce);
    return s;
}

// Where the tuples of a query begin inside its piece: a result is held in pieces (one per chunk of queries, a query never spans two,
// piece j begins with match piece_first[j] of the result), and a piece stores count * k tuple values per query, query after query.
// off[0, nq] are the match offsets of the queries; base[q] = the exclusive sum of count * k over the queries of q's piece before q.
inline void match_tuple_bases(const uint64_t* off, const uint32_t* k, uint64_t nq, const uint64_t* piece_first, uint64_t n_pieces, uint64_t* base)
{
    uint64_t j = 0, acc = 0;
    for (uint64_t q = 0; q < nq; ++q) {
        while (j + 1 < n_pieces && off[q] >= piece_first[j + 1]) { ++j; acc = 0; }
        base[q] = acc;
        acc += (off[q + 1] - off[q]) * k[q];
    }
}

}  // namespace vlg
