// Text windows on the FM-index path (vlg_queries_set_windows + vlg_search_batch): the key arithmetic of a window, and the cut of a
// sorted occurrence list to it.  Plain C++ (no HIP header): search.hip computes the keys with it on the host, and a CPU test compiles
// it alone (tests/window_cut_check.cpp).
//
// A sub-pattern of m symbols occurs at v inside the window [begin, end) of a text of n_text positions iff begin <= v and v + m <= E,
// E = min(end, n_text).  On the sorted list of its occurrences that is the rank interval [lower_bound(klo), lower_bound(khi)) with
// klo = begin and khi = E - m + 1: a window is a cut of the list, and nothing of the list moves.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vlg {

struct WindowKeys {
    uint64_t klo, khi;      // the occurrences v with klo <= v < khi lie inside the window (valid when !empty)
    bool empty;             // the window holds no occurrence of m symbols at all
};

// All arithmetic in uint64_t; nothing wraps for end = 2^64 - 1 (khi <= n_text, or n_text + 1 when m = 0).  khi can be 2^32 while the
// positions are 32-bit (n_text = 2^32 + 1): keys are compared as 64-bit values.
inline WindowKeys window_keys(uint64_t begin, uint64_t end, uint64_t m, uint64_t n_text)
{
    const uint64_t E = end < n_text ? end : n_text;
    if (begin >= E || E - begin < m) return {0, 0, true};
    return {begin, E - m + 1, false};
}

// Host reference of the cut: list[*rlo .. *rhi) are the elements inside the window (an empty window gives rlo = rhi = 0).
template <typename pos_t>
inline void window_cut_host(const pos_t* list, size_t len, const WindowKeys& k, size_t* rlo, size_t* rhi)
{
    *rlo = *rhi = 0;
    if (k.empty) return;
    auto lower = [&](uint64_t key) {
        size_t a = 0, b = len;
        while (a < b) { const size_t mid = a + ((b - a) >> 1); if ((uint64_t)list[mid] < key) a = mid + 1; else b = mid; }
        return a;
    };
    *rlo = lower(k.klo);
    *rhi = lower(k.khi);
}

}  // namespace vlg
