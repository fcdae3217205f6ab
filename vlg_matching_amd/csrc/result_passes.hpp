// What the device passes over a finished result share (doc_list.hpp: document listing; match_text.hpp: match texts; the next consumer).
// Part of search.hip's translation unit, behind the result cache and join_device.hpp:
//   ResultView       a result as its pieces: the refusals, the match offsets of the queries, the pieces with matches laid end to end
//   with_piece_type  the position type of a piece (4 or 8 bytes) as a type
//   doc_ref          the only place that builds a DocRef
//   CachedBuf, scan_with_total   device memory from the cache of the result buffers; rocPRIM's scan with its total read back
//   WaveRun, run_grid, QueryCarry   how the matches of a piece are dealt to waves, and the query a wave stands in
#pragma once
#include "doc_list_math.hpp"

namespace {

#ifndef VLG_DOCLIST_RUN
#define VLG_DOCLIST_RUN 2048
#endif
// a multiple of 64: runs start on a word of the head bits, and a step writes that word whole
static_assert(VLG_DOCLIST_RUN >= 64 && VLG_DOCLIST_RUN % 64 == 0 && VLG_DOCLIST_RUN <= (1u << 24), "VLG_DOCLIST_RUN: a multiple of 64 matches, at least 64");
constexpr uint32_t kDocListRun = VLG_DOCLIST_RUN;      // matches a wave of a result pass takes

// the documents as the kernels see them (join_device.hpp); no documents: the empty DocRef (B null)
inline DocRef doc_ref(const vlg_documents* d, const uint64_t* seg_len = nullptr)
{
    if (!d) return DocRef();
    return DocRef{d->d_starts, d->d_fences, (uint32_t)(d->n_docs + 1), seg_len};
}

// device memory of a handle and of its making, back to the cache of the result buffers when it goes
struct CachedBuf {
    void* p = nullptr;
    uint64_t cap = 0;
    CachedBuf() = default;
    CachedBuf(const CachedBuf&) = delete;
    CachedBuf& operator=(const CachedBuf&) = delete;
    ~CachedBuf() { release(); }
    void release() { if (p) result_cache().give(p, cap); p = nullptr; cap = 0; }
    hipError_t alloc(uint64_t need) { release(); return result_alloc(&p, need ? need : 256, &cap); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Exclusive scan of d[0, n] in place -- n values and the zero behind them, which becomes their total -- and that total read back
// together with the word behind it (a flag or a counter of the pass before).  Synchronises: the temp goes back on return.
inline vlg_status scan_with_total(uint64_t* d, uint64_t n, uint64_t back[2])
{
    CachedBuf tmp;
    VLG_HIP_TRY(with_scratch(tmp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, d, d, 0ull, n + 1, rocprim::plus<uint64_t>(), (hipStream_t) nullptr); }));
    VLG_HIP_TRY(hipMemcpy(back, d + n, 16, hipMemcpyDeviceToHost));
    return VLG_OK;
}

// A result as the passes see it.  The matches are numbered in the order vlg_result_fetch returns them; query q owns [off[q], off[q + 1]).
// The pieces that hold matches lie end to end: piece k holds [first[k], first[k + 1]) and begins with a query; pad[k] is its place in the
// padded numbering of doc_list_math.hpp.
struct ResultView {
    uint64_t nq = 0, np = 0;
    std::vector<uint64_t> off;                  // [nq + 1]
    std::vector<const ResultPiece*> pieces;     // [np]
    std::vector<uint64_t> lay;                  // first[np + 1], pad[np + 1]: one block, as the listing uploads it
    uint64_t first(uint64_t k) const { return lay[k]; }
    uint64_t pad(uint64_t k) const { return lay[np + 1 + k]; }
    uint64_t matches() const { return off[nq]; }

    // fn: the entry point, for the messages
    vlg_status build(const vlg_result* r, const char* fn)
    {
        const std::string who = std::string(fn) + ": ";
        if (!r->owned.empty()) return fail(VLG_E_UNSUPPORTED, who + "the result of a collective search holds only part of the queries");
        nq = r->counts.size();
        if (nq >= 0xFFFFFFFFull) return fail(VLG_E_UNSUPPORTED, who + "more than 2^32 - 2 queries");
        off.resize(nq + 1);
        off[0] = 0;
        for (uint64_t q = 0; q < nq; ++q) off[q + 1] = off[q] + r->counts[q];
        std::vector<uint64_t> piece_m;
        for (const auto& p : r->pieces)
            if (p.matches) { pieces.push_back(&p); piece_m.push_back(p.matches); }
        np = pieces.size();
        lay.resize(2 * (np + 1));
        vlg::doclist_layout(piece_m.data(), np, kDocListRun, lay.data(), lay.data() + np + 1);
        if (first(np) != matches()) return fail(VLG_E_INTERNAL, who + "the pieces of the result do not add up to its counts");
        for (uint64_t k = 0; k < np; ++k) {
            if (pieces[k]->width != 4 && pieces[k]->width != 8) return fail(VLG_E_INTERNAL, who + "positions of an unknown width");
            if (!std::binary_search(off.begin(), off.end(), first(k))) return fail(VLG_E_INTERNAL, who + "a piece of the result begins inside a query");
        }
        return VLG_OK;
    }
    // (asynchronous, from pageable memory: synchronise before the view goes)
    hipError_t upload_off(uint64_t* d_off) const { return hipMemcpyAsync(d_off, off.data(), (nq + 1) * 8, hipMemcpyHostToDevice, nullptr); }
};

// f(uint32_t{}) or f(uint64_t{}): the positions of the piece are of the argument's type (ResultView has refused every other width)
template <class F>
void with_piece_type(const ResultPiece& p, F&& f)
{
    if (p.width == 4) f(uint32_t{}); else f(uint64_t{});
}

// The matches [a, b) of a piece are dealt to waves in runs of kDocListRun, four waves to a workgroup; a wave takes 64 per step.
inline dim3 run_grid(uint64_t matches) { return dim3((uint32_t)((vlg::doclist_runs(matches, kDocListRun) + 3) / 4)); }
struct WaveRun {
    uint32_t lane;
    uint64_t begin, end;                // wave-uniform: the wave's matches
    __device__ __forceinline__ WaveRun(uint64_t a, uint64_t b) : lane(threadIdx.x & 63)
    {
        begin = a + ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kDocListRun;
        end = begin + kDocListRun < b ? begin + kDocListRun : b;
    }
    __device__ __forceinline__ bool empty() const { return begin >= end; }     // (whole waves leave)
};

// The query of the match a wave stands at, carried from step to step.
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

}  // namespace
