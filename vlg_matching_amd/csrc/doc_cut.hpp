// Document boundaries (vlg_documents + vlg_queries_set_documents): the arithmetic that keeps a match inside one document.  Plain C++
// (no HIP header): the join kernels (join_device.hpp) call it on the device, vlg_documents_create on the host, and a CPU test
// compiles it alone (tests/doc_cut_check.cpp).
//
// The documents of a text of n_text positions are given by their starts B[0] = 0 < B[1] < ... < B[d-1] < n_text, closed by the
// sentinel B[d] = n_text: document j is [B[j], B[j+1]).  nb(x), the next boundary of a position x < n_text, is the first entry > x.
//   * an occurrence of m symbols at x lies inside a document  iff  x + m <= nb(x)                              (doc_straddles)
//   * the next sub-pattern, of m' symbols, has to start in [x + lo, min(x + hi, nb(x) - m')]                    (doc_cap_window):
//     one cap keeps it in x's document and drops the candidates that cross the boundary themselves
//   * the chain of a query restarts at min(end + end_len, nb(x)): a match never delays the first match of the
//     next document (end lies in x's document, so nb(x) = nb(end))                                             (doc_cap_restart)
// All arithmetic in uint64_t, nothing wraps: differences are taken on the side that is known to be the larger one.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VLG_DOC_HD __host__ __device__ __forceinline__
#else
#define VLG_DOC_HD inline
#endif

namespace vlg {

// index of the first entry > x of the ascending array B[a, b) (b if there is none)
VLG_DOC_HD uint64_t doc_upper_bound(const uint64_t* B, uint64_t a, uint64_t b, uint64_t x)
{
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (B[mid] <= x) a = mid + 1; else b = mid;
    }
    return a;
}

// nb(x) for x < n_text over the n_docs + 1 entries of B (starts and sentinel); x >= n_text has no document: the sentinel itself
VLG_DOC_HD uint64_t doc_next_boundary(const uint64_t* B, uint64_t n_docs, uint64_t x)
{
    const uint64_t r = doc_upper_bound(B, 0, n_docs + 1, x);
    return B[r <= n_docs ? r : n_docs];
}

// an occurrence of m symbols at x < nb crosses the boundary nb = nb(x)
VLG_DOC_HD bool doc_straddles(uint64_t x, uint64_t m, uint64_t nb) { return m > nb - x; }

// The window's upper end `thi` (x + hi, saturated by the caller) capped so that a next sub-pattern of m_next symbols stays inside
// x's document; false: no start at or after x fits in front of the boundary.
VLG_DOC_HD bool doc_cap_window(uint64_t x, uint64_t m_next, uint64_t nb, uint64_t& thi)
{
    if (m_next > nb - x) return false;
    const uint64_t cap = nb - m_next;                     // >= x
    if (cap < thi) thi = cap;
    return true;
}

// restart key of a chain whose match begins at x and ends at `end`
VLG_DOC_HD uint64_t doc_cap_restart(uint64_t end, uint64_t end_len, uint64_t nb)
{
    const uint64_t k = end + end_len;
    const uint64_t key = k < end ? ~0ull : k;             // saturated
    return key < nb ? key : nb;
}

// what vlg_documents_create accepts: 0 = fine, otherwise the index of the first offending start plus one
inline uint64_t doc_starts_invalid(const uint64_t* starts, uint64_t n_docs, uint64_t n_text)
{
    if (!starts || !n_docs || starts[0] != 0) return 1;
    for (uint64_t j = 0; j < n_docs; ++j) {
        if (starts[j] >= n_text) return j + 1;
        if (j && starts[j] <= starts[j - 1]) return j + 1;
    }
    return 0;
}

}  // namespace vlg
