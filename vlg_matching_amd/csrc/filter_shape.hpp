// Window filter: what the filter of one query looks like and what it is charged, written so that a CPU program compiles it too
// (tests/filter_shape_check.cpp), like select_code.hpp and rrr_code.hpp: no HIP header, no workspace, no allocation.
//   FilterOptions        the workspace values the decision reads (search.hip: filter_options fills it)
//   filter_shape         a query's list lengths -> how it is filtered, from which pivot, what it marks and in how many runs.  The
//                        planner (plan_joins, plan_super_chunk) and the driver (filter.hpp: FilterPass) both read this and nothing else
//   filter_bytes         what plan_joins charges a query for the arrays FilterPass::carve takes, term by term
//   filter_group_charge  ... and a group of queries on top of its queries
// The charges decide where groups and chunks are cut: they are generous in places (noted below) and stay as they are.
#pragma once
#include <cstdint>

namespace vlg {

// Slots are dealt to waves in contiguous runs so a wave can carry the segment it is in and the last answer
// of its searches from one 64-slot step to the next (join_device.hpp); a run is also the unit of the filter's activity bits.
constexpr uint32_t kRun = 2048;

struct FilterOptions {
    bool filter, filter_pivot;
    uint64_t filter_min, filter_stream_min, filter_pivot_ratio, pivot_range_ratio;
};

enum class FilterKind : uint8_t {
    kNone,          // joined as it is
    kStream,        // streaming sweeps over block bitmaps; activity bits for every list but the last
    kPivotBits,     // from its shortest list outwards; activity bits for the lists it marks
    kPivotRanges    // ... the index ranges themselves, 8 bytes per pivot element and marked level
};
enum SegKind : uint8_t { kBits = 0, kRanges = 1 };      // what a compacted segment keeps; a run = kRun slots / 64 pivot elements

struct FilterShape {
    FilterKind kind = FilterKind::kNone;
    uint32_t k = 0, pivot = 0;          // lists; level of the shortest one (the first of them)
    const uint64_t* occ = nullptr;      // the k list lengths
    bool by_pivot() const { return kind == FilterKind::kPivotBits || kind == FilterKind::kPivotRanges; }
    SegKind seg_kind() const { return kind == FilterKind::kPivotRanges ? kRanges : kBits; }
    // level i gets bits or ranges: the last list is never filtered and a pivot list keeps every element
    bool marked(uint32_t i) const { return i + 1 < k && !(by_pivot() && i == pivot); }
    // marked levels; for a pivot query also the levels searched per pivot element
    uint32_t levels() const { return kind == FilterKind::kNone ? 0 : k - 1 - (by_pivot() && pivot + 1 < k ? 1 : 0); }
    // (with two lists and the first one as the pivot there is nothing to mark: the query stays out of the filter's tables)
    bool marks() const { return levels() != 0; }
    uint64_t runs(uint32_t i) const { return kind == FilterKind::kPivotRanges ? (occ[pivot] + 63) / 64 : (occ[i] + kRun - 1) / kRun; }
};

// What a pivot-filtered query keeps for the lists it marks: activity bits (a bit per slot) or the index ranges themselves (8 bytes
// per pivot element and marked level), the latter when the marked slots are at least pivot_range_ratio times the (pivot element,
// level) pairs -- 64 is where the two cost the same bytes; 0 = always bits.
// Below that the ranges are the larger state, by design: with the summaries a pair is charged kRangeGroupBytes / 64 = 8.5 bytes, the
// slots it stands for pivot_range_ratio / 8 at the least, so a query's filter state grows by up to 68 / pivot_range_ratio (4.25 times
// at the default of 16, 68 times at 1).  plan_joins charges exactly that: under a workspace cap so tight that the ranges of one query
// pass the group's share (a third of the join budget), that query is joined unfiltered where its bits might have fitted.  Ratios
// below 8 are for tests.
inline bool filter_keeps_ranges(const uint64_t* occ, uint32_t k, uint32_t pivot, uint64_t pivot_range_ratio)
{
    if (!pivot_range_ratio) return false;
    uint64_t slots = 0, levels = 0;
    for (uint32_t i = 0; i + 1 < k; ++i) if (i != pivot) { slots += occ[i]; ++levels; }
    return levels && slots / pivot_range_ratio >= occ[pivot] * levels;
}

inline FilterShape filter_shape(const uint64_t* occ /* the query's k list lengths */, uint32_t k, const FilterOptions& o)
{
    FilterShape s;
    s.k = k; s.occ = occ;
    if (!o.filter || k < 2 || !occ[0]) return s;
    uint64_t slots = 0, all = 0, best = ~0ull;
    for (uint32_t i = 0; i < k; ++i) {
        if (i + 1 < k) slots += occ[i];
        all += occ[i];
        if (occ[i] < best) { best = occ[i]; s.pivot = i; }
    }
    if (slots < o.filter_min || !slots) return s;
    // two binary searches per pivot element and level against a pass (or two) over every element of every list
    if (o.filter_pivot && best * o.filter_pivot_ratio <= all)
        s.kind = filter_keeps_ranges(occ, k, s.pivot, o.pivot_range_ratio) ? FilterKind::kPivotRanges : FilterKind::kPivotBits;
    else if (slots >= o.filter_stream_min) s.kind = FilterKind::kStream;   // the block bitmaps of a streamed query are a fixed cost (2 x n / 2^g bits)
    return s;
}

// ---- the charge, next to what FilterPass::carve takes (filter.hpp; T x n = n items of T) --------------------------------------
constexpr uint64_t kSegBytes = 64;                     // d_segs: RSeg x segments
constexpr uint64_t kSegTableBytes = 64;                // per segment, 44 at the most: d_task_seg 4, d_task_run0 8; if compacted d_cseg 4, d_crun0 8,
                                                       // d_segcnt 8, and in a group of both kinds d_kseg 4, d_krun0 8
constexpr uint64_t kQueryTableBytes = 64;              // per query, 24 at the most: d_ptasks 16, d_prun0 8
constexpr uint64_t kBitRunBytes = kRun / 8 + 4;        // per run of kRun slots: d_abits, d_runcnt
// per group of 64 pivot elements and marked level: ranges 64 x uint2, d_top 8, key 8, first 8, inner 4, d_runcnt 4, and a byte
// towards the scan of the groups' maxima
constexpr uint64_t kRangeGroupBytes = 64 * 8 + 8 + 8 + 8 + 4 + 4 + 1;

// Bytes of filter state a query needs (0 = the query is not filtered); nbw = words of one block bitmap; runs: what its lists add
// to the runs of a compaction.  A query with nothing to mark is charged all the same, and one that keeps bits also for the runs of
// its pivot list, which has none.
inline uint64_t filter_bytes(const FilterShape& s, uint64_t nbw, uint64_t* runs = nullptr)
{
    if (s.kind == FilterKind::kNone) return 0;
    uint64_t bytes = s.kind == FilterKind::kStream ? 2 * nbw * 8 /* d_bm */ : 0, nruns = 0;
    if (s.kind == FilterKind::kPivotRanges) {
        nruns = s.levels() * s.runs(s.pivot);
        bytes += nruns * kRangeGroupBytes;
    } else {
        for (uint32_t i = 0; i + 1 < s.k; ++i) nruns += (s.occ[i] + kRun - 1) / kRun;
        bytes += nruns * kBitRunBytes;
    }
    if (runs) *runs = nruns + s.k;
    return bytes + s.k * (kSegBytes + kSegTableBytes) + kQueryTableBytes;
}

// What the filter needs of the join budget: the state of one group (total = the batch's filter_bytes, at most cap a group), the
// d_cnt and d_off of a chunk that compacts its own lists (JoinChunk::compact_survivors: 4 + 4 bytes a run; runs = the batch's),
// and once the temporary storage of the scans with the rounding of every take
inline uint64_t filter_group_charge(uint64_t total, uint64_t cap, uint64_t runs)
{
    return (total < cap ? total : cap) + runs * 8 + (total ? 16384 : 0);
}

}  // namespace vlg
