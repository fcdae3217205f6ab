// Types shared by the translation units of the search path.
#pragma once
#include <cstdint>
#include <vector>

// The documents of a text (vlg_documents_create): the starts and the sentinel n_text in HBM, and one fence per 64 of them, laid out
// as the fences of the occurrence lists are (join_device.hpp: F[g] = B[64 g + 63]).  The host copy serves the argument checks.
struct vlg_documents {
    uint64_t n_docs = 0, n_text = 0;
    std::vector<uint64_t> starts;    // [n_docs + 1], starts[n_docs] = n_text
    uint64_t* d_starts = nullptr;    // [n_docs + 1]
    uint64_t* d_fences = nullptr;    // [(n_docs + 1) / 64]
};

struct vlg_queries {
    uint64_t nq = 0, nsub = 0;
    std::vector<uint64_t> qsub;      // [nq+1]
    std::vector<uint64_t> suboff;    // [nsub+1]
    std::vector<uint8_t> blob;
    std::vector<uint64_t> lo, hi;    // [nsub]
    std::vector<uint64_t> end_len;   // [nq]
    uint32_t kmax = 0, kmin = 0;     // over queries with at least one sub-pattern
    uint32_t sym_bytes = 1;          // 1: byte sub-patterns; 4: integer alphabet (vlg_queries_parse_int), symbols little-endian in blob
    uint8_t* d_blob = nullptr;
    uint64_t* d_suboff = nullptr;
    uint64_t* d_qsub = nullptr;      // [nq+1] on the device (the interval plan groups sub-patterns by query)
    // text windows (vlg_queries_set_windows): empty = the batch carries none; otherwise [nq] each, host only.  win_end holds the
    // caller's values (UINT64_MAX = "to the end of the text"): the batch does not know n, the search clamps.
    std::vector<uint64_t> win_begin, win_end;
    bool has_windows() const { return !win_end.empty(); }
    // character classes (vlg_queries_parse_classes / _create_classes): empty = the batch has none and is a byte batch like any other.
    // Otherwise one 256-bit row per position of the batch (bit c = byte c), position p of the batch = byte p of blob, so that suboff
    // still counts positions; blob then holds placeholders (the byte itself where a position accepts one byte, the least member
    // otherwise) that only vlg_search_batch's class path may read, and only for the sub-patterns sub_literal[] marks.
    std::vector<uint8_t> masks;      // [positions * 32]
    std::vector<uint8_t> sub_literal;    // [nsub]: every position of the sub-pattern accepts exactly one byte
    uint8_t* d_masks = nullptr;
    bool has_classes() const { return !masks.empty(); }
    // mismatch budgets (vlg_queries_set_mismatches): empty = none.  Otherwise sub-pattern s may differ from the text in up to sub_k[s]
    // of its positions (substitutions only), and at least one budget is > 0.  Host state only, like the windows.
    std::vector<uint8_t> sub_k;          // [nsub]
    bool has_mismatches() const { return !sub_k.empty(); }
    // documents (vlg_queries_set_documents): null = none.  Borrowed: the handle outlives every search of the batch.
    const vlg_documents* docs = nullptr;
    bool has_documents() const { return docs != nullptr; }
};
