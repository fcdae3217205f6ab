// Document listing (vlg_result_list_documents): the arithmetic that is not wave code.  Plain C++ (no HIP header): the kernels of
// doc_list.hpp call it on the device, vlg_doc_listing_fetch on the host, and a CPU test compiles it alone (tests/doc_list_check.cpp).
//
// The matches of a result are numbered 0 .. M - 1 in the order vlg_result_fetch returns their first positions; query q owns
// [off[q], off[q + 1]).  The listing of q is the sequence of maximal runs of equal doc(first position) inside that range.
//   * match i is a HEAD (begins a run)  iff  it is the first match of its query or doc(i) != doc(i - 1)           (doclist_head)
//   * rank(g) = heads among the matches < g;  df[q] = rank(off[q + 1]) - rank(off[q]), pair p of the listing is the head of rank p
//   * count of pair p = first_match[p + 1] - first_match[p], closed by off[q + 1] for the last pair of q          (doclist_counts)
// A result is held in pieces (one per chunk of queries, a query never spans two); a piece's matches are dealt to waves in runs of R
// (a multiple of 64), so every piece begins on a run of its own in the PADDED numbering the head bits and the per-run head counts are
// indexed by: piece k begins at pad[k] = R * (runs of the pieces before it), match first[k] + e of it is bit pad[k] + e  (doclist_layout).
// All arithmetic in uint64_t.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VLG_DL_HD __host__ __device__ __forceinline__
#else
#define VLG_DL_HD inline
#endif

namespace vlg {

// the head rule; prev_doc is not looked at for the first match of a query (a run never continues across a query border)
VLG_DL_HD bool doclist_head(bool first_of_query, uint64_t doc, uint64_t prev_doc) { return first_of_query || doc != prev_doc; }

VLG_DL_HD uint64_t doclist_runs(uint64_t matches, uint64_t run) { return matches / run + (matches % run != 0); }

VLG_DL_HD uint64_t doclist_popcount(uint64_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__popcll(w);
#else
    return (uint64_t)__builtin_popcountll(w);
#endif
}

// Concatenation of pieces: first[k] = matches of the pieces before piece k, pad[k] = where its bits begin (a multiple of `run`).
// Both arrays get n_pieces + 1 entries; the last ones are the total number of matches and of padded bits.
inline void doclist_layout(const uint64_t* piece_matches, uint64_t n_pieces, uint64_t run, uint64_t* first, uint64_t* pad)
{
    uint64_t f = 0, p = 0;
    for (uint64_t k = 0; k < n_pieces; ++k) {
        first[k] = f; pad[k] = p;
        f += piece_matches[k];
        p += doclist_runs(piece_matches[k], run) * run;
    }
    first[n_pieces] = f; pad[n_pieces] = p;
}

// the piece that holds match g < first[n_pieces]: the last k with first[k] <= g (pieces without matches are never the answer)
VLG_DL_HD uint64_t doclist_piece_of(const uint64_t* first, uint64_t n_pieces, uint64_t g)
{
    uint64_t a = 0, b = n_pieces;                       // first[a] <= g < first[b]
    while (b - a > 1) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (first[mid] <= g) a = mid; else b = mid;
    }
    return a;
}

// heads in front of the padded bit `at`: the exclusive prefix of its run's head count plus the set bits of the run in front of it
VLG_DL_HD uint64_t doclist_rank(const uint64_t* run_rank, const uint64_t* bits, uint64_t run, uint64_t at)
{
    const uint64_t r = at / run;
    uint64_t rank = run_rank[r];
    for (uint64_t w = r * run / 64; w < at / 64; ++w) rank += doclist_popcount(bits[w]);
    if (at % 64) rank += doclist_popcount(bits[at / 64] & ((1ull << (at % 64)) - 1));
    return rank;
}

// rank of match g of the result (g == total: all heads, kept behind the last run's prefix)
VLG_DL_HD uint64_t doclist_rank_of_match(const uint64_t* first, const uint64_t* pad, uint64_t n_pieces, const uint64_t* run_rank,
                                         const uint64_t* bits, uint64_t run, uint64_t g)
{
    if (g >= first[n_pieces]) return run_rank[pad[n_pieces] / run];
    const uint64_t k = doclist_piece_of(first, n_pieces, g);
    return doclist_rank(run_rank, bits, run, pad[k] + (g - first[k]));
}

// counts from consecutive heads: pair_off[nq + 1] = the pairs of each query, first_match[pair_off[nq]], off[nq + 1] = the matches
inline void doclist_counts(const uint64_t* off, const uint64_t* pair_off, uint64_t nq, const uint64_t* first_match, uint64_t* counts)
{
    for (uint64_t q = 0; q < nq; ++q)
        for (uint64_t p = pair_off[q]; p < pair_off[q + 1]; ++p)
            counts[p] = (p + 1 < pair_off[q + 1] ? first_match[p + 1] : off[q + 1]) - first_match[p];
}

}  // namespace vlg
