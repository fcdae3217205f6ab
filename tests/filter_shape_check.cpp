// CPU check of the window filter's shape and charge (vlg_matching_amd/csrc/filter_shape.hpp), built and run by tests/test_filter_shape.py:
// the header the planner and the filter's driver compile, against
//   1. a literal restatement of filter_mode, filter_by_ranges and filter_bytes as they stood before the header existed (commit ab541d6;
//      sizeof(RSeg) written as 64): kind, pivot, runs of every marked level and the bytes charged must be the same;
//   2. the bytes FilterPass::carve takes for the query (filter.hpp), restated below array by array: the charge must cover them.  Not
//      counted: rocPRIM's temporary storage and the rounding of every take, which filter_group_charge's constant pays for.
// over every k in 1..5, every list length in {0, 1, 63, 64, 65, 2047, 2048, 2049, 70000} at every level, and every combination of
// filter {0,1}, filter_min {0,4096}, filter_stream_min {0,2^40}, filter_pivot {0,1}, filter_pivot_ratio {1,2,8}, pivot_range_ratio {0,1,16,64}.
#include "filter_shape.hpp"
#include <cstdio>
#include <initializer_list>
#include <vector>
using namespace vlg;

// ---- the parent commit's functions ------------------------------------------------------------------
struct OldQueries { std::vector<uint64_t> qsub; };
struct OldPlan { std::vector<uint64_t> occ; };
struct OldWorkspace { bool filter, filter_pivot; uint64_t filter_min, filter_stream_min, filter_pivot_ratio, pivot_range_ratio; };
constexpr uint64_t kOldSizeofRSeg = 64, kOldSizeofUint2 = 8;

static int old_filter_mode(const OldQueries* q, const OldPlan& pl, const OldWorkspace* ws, uint64_t qi, uint32_t* pivot = nullptr)
{
    const uint64_t s0 = q->qsub[qi], k = q->qsub[qi + 1] - s0;
    if (!ws->filter || k < 2 || !pl.occ[s0]) return 0;
    uint64_t slots = 0, all = 0, best = ~0ull;
    uint32_t p = 0;
    for (uint64_t i = 0; i < k; ++i) {
        if (i + 1 < k) slots += pl.occ[s0 + i];
        all += pl.occ[s0 + i];
        if (pl.occ[s0 + i] < best) { best = pl.occ[s0 + i]; p = (uint32_t)i; }
    }
    if (slots < ws->filter_min || !slots) return 0;
    if (pivot) *pivot = p;
    if (ws->filter_pivot && best * ws->filter_pivot_ratio <= all) return 2;
    return slots >= ws->filter_stream_min ? 1 : 0;
}

static bool old_filter_by_ranges(const OldQueries* q, const OldPlan& pl, const OldWorkspace* ws, uint64_t qi, uint32_t pivot)
{
    if (!ws->pivot_range_ratio) return false;
    const uint64_t s0 = q->qsub[qi], k = q->qsub[qi + 1] - s0;
    uint64_t slots = 0, levels = 0;
    for (uint64_t i = 0; i + 1 < k; ++i) if (i != pivot) { slots += pl.occ[s0 + i]; ++levels; }
    return levels && slots / ws->pivot_range_ratio >= pl.occ[s0 + pivot] * levels;
}
constexpr uint64_t kOldRangeGroupBytes = 64 * kOldSizeofUint2 + 8 /* top */ + 8 + 8 + 4 /* key, first, inner */ + 4 /* count */ + 1 /* scan */;

static uint64_t old_filter_bytes(const OldQueries* q, const OldPlan& pl, const OldWorkspace* ws, uint64_t qi, uint64_t nbw, uint64_t* runs = nullptr)
{
    uint32_t pivot = 0;
    const int mode = old_filter_mode(q, pl, ws, qi, &pivot);
    if (!mode) return 0;
    const uint64_t s0 = q->qsub[qi], k = q->qsub[qi + 1] - s0;
    uint64_t bytes = mode == 1 ? 2 * nbw * 8 : 0, nruns = 0;
    if (mode == 2 && old_filter_by_ranges(q, pl, ws, qi, pivot)) {
        const uint64_t groups = (pl.occ[s0 + pivot] + 63) / 64 * (k - 1 - (pivot + 1 < k ? 1 : 0));
        bytes += groups * kOldRangeGroupBytes;
        nruns = groups;
    } else {
        for (uint64_t i = 0; i + 1 < k; ++i) { const uint64_t r = (pl.occ[s0 + i] + kRun - 1) / kRun; bytes += r * (kRun / 8 + 4); nruns += r; }
    }
    if (runs) *runs = nruns + k;
    return bytes + k * (kOldSizeofRSeg + 64) + 64;
}

// ---- what FilterPass::carve takes for one query (T x n = n items of T), in the order of its takes ---------------
static uint64_t carved_bytes(const FilterShape& s, uint64_t nbw)
{
    if (!s.marks()) return 0;                           // the query stays out of the tables
    uint64_t runs = 0;
    for (uint32_t i = 0; i < s.k; ++i) if (s.marked(i)) runs += s.runs(i);
    const uint64_t m = s.levels();
    uint64_t b = 0;
    b += 64 * s.k;                                      // d_segs: RSeg x segments
    b += (4 + 8) * m;                                   // d_cseg, d_crun0: per compacted segment
    if (s.seg_kind() == kBits) b += runs * kRun / 8;    // d_abits
    b += 4 * runs;                                      // d_runcnt
    if (s.seg_kind() == kRanges) b += runs * (64 * 8 + 8 /* ranges, d_top */ + 8 + 8 + 4 /* key, first, inner */);
    b += (4 + 8) * m;                                   // d_kseg, d_krun0 (a group of both kinds carves them for both)
    b += 8 * m;                                         // d_segcnt
    if (s.kind == FilterKind::kStream) b += 2 * nbw * 8;    // d_bm
    b += (4 + 8) * s.k;                                 // d_task_seg, d_task_run0
    if (s.by_pivot()) b += 16 + 8;                      // d_ptasks, d_prun0
    return b;
}

int main()
{
    const uint64_t lens[9] = {0, 1, 63, 64, 65, 2047, 2048, 2049, 70000};
    const uint64_t nbws[2] = {1, 4097};
    std::vector<OldWorkspace> opts;
    for (int f = 0; f < 2; ++f) for (uint64_t fm : {0ull, 4096ull}) for (uint64_t fs : {0ull, 1ull << 40}) for (int fp = 0; fp < 2; ++fp)
        for (uint64_t pr : {1ull, 2ull, 8ull}) for (uint64_t rr : {0ull, 1ull, 16ull, 64ull}) opts.push_back(OldWorkspace{f != 0, fp != 0, fm, fs, pr, rr});
    unsigned long long shapes = 0, kinds[4] = {0, 0, 0, 0}, unmarked = 0;
    OldQueries q;
    OldPlan pl;
    for (uint32_t k = 1; k <= 5; ++k) {
        // one query in front, so that the old code's s0 is not 0
        q.qsub = {0, 2, 2 + k};
        pl.occ.assign(2 + k, 7);
        uint32_t digit[5] = {0, 0, 0, 0, 0};
        for (;;) {
            for (uint32_t i = 0; i < k; ++i) pl.occ[2 + i] = lens[digit[i]];
            const uint64_t* occ = pl.occ.data() + 2;
            for (const OldWorkspace& w : opts) {
                const FilterOptions fo{w.filter, w.filter_pivot, w.filter_min, w.filter_stream_min, w.filter_pivot_ratio, w.pivot_range_ratio};
                const FilterShape s = filter_shape(occ, k, fo);
                uint32_t pivot = 0;
                const int mode = old_filter_mode(&q, pl, &w, 1, &pivot);
                const bool ranges = mode == 2 && old_filter_by_ranges(&q, pl, &w, 1, pivot);
                const FilterKind want = mode == 0 ? FilterKind::kNone : mode == 1 ? FilterKind::kStream : ranges ? FilterKind::kPivotRanges : FilterKind::kPivotBits;
                bool ok = s.kind == want && s.k == k && (mode == 0 || s.pivot == pivot) && s.by_pivot() == (mode == 2) && s.seg_kind() == (ranges ? kRanges : kBits);
                // the driver's rules before the header: which levels are marked, and their runs
                uint32_t marked = 0;
                for (uint32_t i = 0; ok && mode && i < k; ++i) {
                    const bool m = i + 1 < k && !(mode == 2 && i == pivot);
                    ok = s.marked(i) == m;
                    if (m) { ++marked; ok = ok && s.runs(i) == (ranges ? (occ[pivot] + 63) / 64 : (occ[i] + kRun - 1) / kRun); }
                }
                ok = ok && (!mode || (s.levels() == marked && s.marks() == !(mode == 2 && k <= 2 && pivot == 0)));
                ok = ok && (mode || !s.marks());
                if (mode == 2) ok = ok && s.levels() == (k >= 2 ? k - 2 + (pivot + 1 == k ? 1 : 0) : 0);     // the probe count's expression
                for (uint64_t nbw : nbws) {
                    uint64_t runs_old = ~0ull, runs_new = ~0ull;
                    const uint64_t b_old = old_filter_bytes(&q, pl, &w, 1, nbw, &runs_old), b_new = filter_bytes(s, nbw, &runs_new);
                    ok = ok && b_old == b_new && runs_old == runs_new;
                    // the planner's invariant: the charge covers what is carved for the query
                    if (b_new < carved_bytes(s, nbw)) {
                        printf("charge %llu below the carve %llu\n", (unsigned long long)b_new, (unsigned long long)carved_bytes(s, nbw));
                        ok = false;
                    }
                }
                if (!ok) {
                    printf("mismatch: k %u, lengths", k);
                    for (uint32_t i = 0; i < k; ++i) printf(" %llu", (unsigned long long)occ[i]);
                    printf("; filter %d min %llu stream_min %llu pivot %d ratio %llu range_ratio %llu; old mode %d pivot %u ranges %d, new kind %d pivot %u\n",
                           (int)w.filter, (unsigned long long)w.filter_min, (unsigned long long)w.filter_stream_min, (int)w.filter_pivot,
                           (unsigned long long)w.filter_pivot_ratio, (unsigned long long)w.pivot_range_ratio, mode, pivot, (int)ranges, (int)s.kind, s.pivot);
                    return 1;
                }
                ++shapes; ++kinds[(int)s.kind];
                if (s.kind != FilterKind::kNone && !s.marks()) ++unmarked;
            }
            uint32_t i = 0;
            while (i < k && ++digit[i] == 9) digit[i++] = 0;
            if (i == k) break;
        }
    }
    // the group's charge, as plan_joins wrote it
    for (uint64_t total : {0ull, 1ull, 4096ull, 1ull << 33}) for (uint64_t cap : {0ull, 4096ull, 1ull << 32}) for (uint64_t runs : {0ull, 5ull, 1ull << 24})
        if (filter_group_charge(total, cap, runs) != (total < cap ? total : cap) + runs * 8 + (total ? 16384 : 0)) { printf("group charge mismatch\n"); return 1; }
    if (kRangeGroupBytes != kOldRangeGroupBytes) { printf("kRangeGroupBytes changed\n"); return 1; }
    printf("kinds: none %llu, streamed %llu, pivot bits %llu, pivot ranges %llu; charged with nothing to mark %llu\n", kinds[0], kinds[1], kinds[2], kinds[3], unmarked);
    if (!kinds[0] || !kinds[1] || !kinds[2] || !kinds[3] || !unmarked) { printf("a kind was never met\n"); return 1; }
    printf("ok %llu shapes\n", shapes);
    return 0;
}
