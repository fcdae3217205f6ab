// Device side of the join (K5): search helpers, feasibility bitset, link / jump / chain / gather kernels.
// Internal to search.hip's translation unit (everything has internal linkage); included exactly once from there.
#pragma once
#include "doc_cut.hpp"
// =============================================================================================
// Join kernels
// =============================================================================================
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kChecksumSlots = 64;     // partial checksums of the gather kernel (added up by the host)

// Occurrence lists are PHYSICAL: one sorted list per distinct SA interval of the batch, shared by every
// query that uses the sub-pattern.  Join state (link / end / feasibility ...) is LOGICAL: one slot per
// element of every (query, level) whose level is not the query's last one (the last list is only searched).
// Logical slots are laid out class-major: all segments with the same `dist` (sub-patterns after them in their
// query) are contiguous, so every pass of the join streams exactly the slots it works on.
struct SegMeta {            // one per sub-pattern of the chunk (device array, class-major order)
    uint32_t begin, end;    // logical slots (begin == end for the last level of a k>=2 query)
    uint32_t pbegin, pend;  // physical list inside P
    uint32_t dist;          // sub-patterns after it in its query (0 = last)
    uint32_t level;         // index inside the query (0 = first)
    uint32_t next;          // segment of the query's next sub-pattern (valid when dist > 0)
    uint32_t query;         // query of the chunk
    uint64_t lo, hi;        // gap bounds between the previous sub-pattern and this one
};

struct QueryMeta {          // one per query of the chunk
    uint32_t seg0;          // first segment (level 0); kNone if the query is dead
    uint32_t k;
    uint64_t end_len;
    uint64_t out_first;     // offsets into the chunk's result arrays (filled before gather)
    uint64_t out_tuple;
};

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) { uint64_t c = a + b; return c < a ? ~0ull : c; }
__device__ __forceinline__ uint32_t phys_of(const SegMeta& m, uint32_t e) { return m.pbegin + (e - m.begin); }

template <typename pos_t>
__device__ __forceinline__ uint32_t lower_bound_dev(const pos_t* __restrict__ P, uint32_t a, uint32_t b, uint64_t key)
{
    while (a < b) {
        uint32_t mid = a + ((b - a) >> 1);
        if ((uint64_t)P[mid] < key) a = mid + 1; else b = mid;
    }
    return a;
}

// Lower bound by galloping from a known lower fence: all indices below `lo` hold values < key.
// Consecutive slots of a list have ascending keys, so the previous answer is a tight fence and the search costs
// O(log distance) probes into lines the neighbouring lanes touch too, instead of log2 |list| cold probes.
template <typename pos_t>
__device__ __forceinline__ uint32_t gallop_lower_bound(const pos_t* __restrict__ P, uint32_t lo, uint32_t b, uint64_t key)
{
    uint32_t step = 1, hi = b;
    bool found = false;
    while (lo < b) {
        uint32_t p = lo + step - 1;
        if (p >= b) p = b - 1;
        if ((uint64_t)P[p] < key) { lo = p + 1; step <<= 1; }
        else { hi = p; found = true; break; }
    }
    if (!found) return b;
    return lower_bound_dev(P, lo, hi, key);
}

// ---- fences ------------------------------------------------------------------------------------------------------------------
// F[g] = P[64 g + 63] for every whole block of 64 elements of the arrays the joins search (fence_build_kernel: the sorted
// physical lists; filter_compact_kernel: the survivors' private lists, as it writes them).  A search that cannot start from a previous answer
// first ranks its key among the fences of the list -- dense entries, ONE 256-byte load for 64 blocks, where probing the list
// itself touches 64 lines -- and then looks at one block of the list.  The fences with index in [a >> 6, b >> 6) are elements of
// the list P[a,b) whatever its borders, so no list needs fences of its own.  F == nullptr: the lists are probed directly.
template <typename pos_t>
__global__ void fence_build_kernel(const pos_t* __restrict__ P, uint64_t g0, uint64_t g1, pos_t* __restrict__ F)
{
    for (uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += (uint64_t)gridDim.x * blockDim.x) F[g] = P[64 * g + 63];
}

// ---- rungs: a search ladder over the sorted lists -----------------------------------------------------------------------------
// R_j[i] = P[f^j (i + 1) - 1], j = 1 .. levels, f = kRungFan: the last element of every whole block of f^j elements.  A lower bound
// descends from the level whose one group of f entries covers the list: ONE aligned load of f entries per level picks one of f
// blocks, so a search touches log_f(length) lines instead of the log2(length) of a bisection -- the pivot filter, whose loads go to
// a different line in almost every lane, is bound by exactly those line requests (L1 misses on their way to L2), not by bytes.
// Entry i of level j lies inside the list P[a,b) iff a >> (s j) <= i < b >> (s j), s = log2 f, whatever the list's borders, so the
// lists share one ladder; entries before the list count as smaller than any key, entries behind it as larger.
#ifndef VLG_RUNG_SHIFT
#define VLG_RUNG_SHIFT 2
#endif
constexpr uint32_t kRungShift = VLG_RUNG_SHIFT, kRungFan = 1u << kRungShift;
constexpr uint32_t kMaxRungs = 32 / kRungShift;         // f^kMaxRungs elements: more than any index here (32-bit)
// >= 2: a level's group of f entries is read as f / 4 aligned quads (pivot_ranges_rungs); <= 8: every lane holds 2 x kPivotGroups
// groups of f entries in registers
static_assert(kRungShift >= 2 && kRungShift <= 8, "VLG_RUNG_SHIFT: 2 .. 8");
struct RungLayout { uint64_t off[kMaxRungs + 1]; uint32_t levels; uint64_t entries; };
inline RungLayout rung_layout(uint64_t total)
{
    RungLayout L{};
    L.levels = 0;
    while (L.levels < kMaxRungs && (total >> (kRungShift * (L.levels + 1))) != 0) ++L.levels;   // the block of level `levels + 1` covers every index
    uint64_t at = 0;
    for (uint32_t j = 1; j <= L.levels; ++j) {                                                  // whole groups, and one to spare
        L.off[j] = at;
        at += (((total >> (kRungShift * j)) + kRungFan - 1) & ~(uint64_t)(kRungFan - 1)) + kRungFan;
    }
    L.entries = at;
    return L;
}

// (F: the fences of the same array, written on the way when the ladder has a level of blocks of 64 -- it is that level -- or null)
template <typename pos_t>
__global__ void rung_build_kernel(const pos_t* __restrict__ P, uint64_t total, pos_t* __restrict__ R, const uint64_t* __restrict__ off, uint32_t levels,
                                  pos_t* __restrict__ F)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (total >> kRungShift); i += (uint64_t)gridDim.x * blockDim.x) {
        const pos_t v = P[kRungFan * i + kRungFan - 1];
        R[off[1] + i] = v;
        uint64_t k = i;
        for (uint32_t j = 2; j <= levels && (k & (kRungFan - 1)) == kRungFan - 1; ++j) {
            k >>= kRungShift;
            R[off[j] + k] = v;
            if (F && kRungShift * j == 6) F[k] = v;
        }
    }
}
constexpr bool kRungsHoldFences = 6 % kRungShift == 0 && kRungShift < 6;       // some level has blocks of 64

template <typename pos_t> struct alignas(4 * sizeof(pos_t)) RungQuad { pos_t v[4]; };

// Keys the windows did not reach (the list is much denser than the keys): two-level search.  Lane t reads the LAST element of
// block t behind the fence `wb` -- one round trip covers 64 blocks -- every lane ranks its key among these 64 fences through
// cross-lane reads and then bisects the one block that holds its answer (6 probes inside 256 bytes).  A galloping search
// would pay ~2 log2(distance) dependent, scattered round trips instead.
constexpr uint32_t kFarRounds = 4;

// -DVLG_LINK_STATS: path counters of the pair search (wave_lower_bound2 and its far searches), one atomic per wave and event;
// search.hip prints and clears them behind every link launch.  A diagnostic build: the atomics cost fifty times what the searches do.
// (the count is formed by every lane -- it may hold a wave-wide vote -- and added by lane 0)
#ifdef VLG_LINK_STATS
enum { LS_PAIRS = 0, LS_WINDOWS, LS_PLACED, LS_FAR0, LS_FAR1, LS_FAR_ROUNDS0, LS_FAR_ROUNDS1, LS_COUNT };
__device__ unsigned long long g_link_stats[LS_COUNT];
#define VLG_LINK_STAT(i, n) do { const unsigned long long n_ = (unsigned long long)(n); if ((threadIdx.x & 63) == 0 && n_) atomicAdd(&g_link_stats[i], n_); } while (0)
#else
#define VLG_LINK_STAT(i, n) do { } while (0)
#endif
template <typename pos_t>
__device__ __forceinline__ void wave_far_lower_bound(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t wb, uint32_t b, pos_t key,
                                                     bool need, uint32_t& j, pos_t& val, uint32_t stat_reg = 2 /* VLG_LINK_STATS: 0 / 1 = a register of a pair */)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr pos_t kInf = (pos_t)~(pos_t)0;
    for (uint32_t round = 0; round < kFarRounds && wb < b; ++round) {
        if (!__any(need)) return;
        if (stat_reg < 2) VLG_LINK_STAT(LS_FAR_ROUNDS0 + stat_reg, 1);
        // without fences the blocks start at wb; with them they are the aligned blocks of the array, the first one cut at wb
        const uint32_t g0 = F ? wb >> 6 : 0;
        pos_t f;
        if (F) f = g0 + lane < (b >> 6) ? F[g0 + lane] : kInf;       // blocks that reach behind the list end with +inf
        else { const uint64_t fi = (uint64_t)wb + 64 * lane + 63; f = fi < b ? P[fi] : kInf; }
        const pos_t flast = __shfl(f, 63);
        const bool can = need && key <= flast;
        uint32_t lo = 0;                                             // first block whose last element is >= key
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1) {
            const pos_t v = __shfl(f, (int)(lo + step - 1));
            lo += v < key ? step : 0u;
        }
        if (can) {
            uint64_t w0 = F ? ((uint64_t)(g0 + lo) << 6) : (uint64_t)wb + 64 * lo;   // the answer is in [w0, w0+63] (or b, in a clipped block)
            const uint64_t w1 = w0 + 64 < b ? w0 + 64 : b;
            if (w0 < wb) w0 = wb;
            uint32_t pos = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint64_t at = w0 + pos + step - 1;
                if (at < w1 && P[at] < key) pos += step;
            }
            const uint64_t at = w0 + pos;
            if (at < b) { j = (uint32_t)at; val = P[at]; } else j = b;
            need = false;
        }
        const uint64_t nwb = F ? ((uint64_t)(g0 + 64) << 6) : (uint64_t)wb + 4096;
        wb = nwb < b ? (uint32_t)nwb : b;
    }
    if (need) {
        j = gallop_lower_bound(P, wb < b ? wb : b, b, (uint64_t)key);
        if (j < b) val = P[j]; else j = b;
    }
}

// Lower bounds of 64 ascending keys in one sorted list, as a wave: the answers of a step lie just behind the last
// answer of the previous step, so the wave loads consecutive 64-element windows of the list with ONE coalesced load
// each and every lane ranks its key inside the window through cross-lane reads (6 steps) -- a merge of two sorted
// runs, without the ~15 scattered probes per lane of an independent search.  `wb` (wave-uniform) must be a fence:
// every element before it is smaller than every key.  Lanes still unresolved after kCoopWindows windows fall back
// to galloping from the last window's end.
constexpr uint32_t kCoopWindows = 4;
// Keys and list elements are compared as pos_t (one cross-lane read per step for 32-bit positions); `val` receives the list
// element at the answer, so the caller needs no load of its own for it.
template <typename pos_t>
__device__ __forceinline__ uint32_t wave_lower_bound(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t wb, uint32_t b, pos_t key, bool need, pos_t& val)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr pos_t kInf = (pos_t)~(pos_t)0;
    uint32_t res = b;
    for (uint32_t it = 0; it < kCoopWindows; ++it) {
        if (!__any(need)) break;
        const uint32_t idx = wb + lane;
        const pos_t w = idx < b ? P[idx] : kInf;                     // +inf behind the list
        const pos_t wlast = __shfl(w, 63);
        const bool can = need && key <= wlast;
        uint32_t lo = 0;                                             // for `can` lanes w[63] >= key, so the answer is in [0,63]
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1) {                 // lo = elements of w[0,63) below the key
            const pos_t v = __shfl(w, (int)(lo + step - 1));
            lo += v < key ? step : 0u;
        }
        const pos_t at = __shfl(w, (int)lo);
        if (can) { res = wb + lo; val = at; need = false; }
        wb += 64;
    }
    if (__any(need)) wave_far_lower_bound(P, F, wb < b ? wb : b, b, key, need, res, val);
    return res < b ? res : b;
}

// Two steps at once: 128 ascending keys (lane i holds keys i and 64+i) share every window load, its fence test and the
// loop around them, which is most of what a step costs.
#ifndef VLG_COOP_WINDOWS2
#define VLG_COOP_WINDOWS2 4
#endif
static_assert(VLG_COOP_WINDOWS2 >= 1, "VLG_COOP_WINDOWS2: at least one window before the far search");
constexpr uint32_t kCoopWindows2 = VLG_COOP_WINDOWS2;      // round 3, link class on C3: 3 -> 22.2, 4 -> 21.9, 6 -> 22.5, 9 -> 22.8 ms (flat: the
                                                             // far search is about as cheap per key as a window); round 2:            // measured on C3: 2 -> 35.2, 3 -> 33.8, 4 -> 33.2, 6 -> 31.9, 8..16 -> 33..34 ms
// kEarly: the next window's address is wb + 64 whatever the ranking of this one finds, so its load is issued before the ranking -- six
// dependent cross-lane reads -- and has come when the loop wants it; a pair that ends in this window has loaded one window for
// nothing (one coalesced load).  The addresses are those the loop loaded before, each one iteration earlier.  Measured in DESIGN 9
// (profiles/link_skip.jsonl).  VLG_LINK_EARLY = 0 compiles the loop that loads a window when it turns to it, for an A/B between two builds.
#ifndef VLG_LINK_EARLY
#define VLG_LINK_EARLY 1
#endif
static_assert(VLG_LINK_EARLY == 0 || VLG_LINK_EARLY == 1, "VLG_LINK_EARLY: 0 or 1");
template <typename pos_t, bool kEarly>
__device__ __forceinline__ void wave_lower_bound2(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t wb, uint32_t b, pos_t key0, bool need0, pos_t key1,
                                                  bool need1, uint32_t& j0, pos_t& v0, uint32_t& j1, pos_t& v1)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr pos_t kInf = (pos_t)~(pos_t)0;
    j0 = b; j1 = b;
    VLG_LINK_STAT(LS_PAIRS, 1);
    pos_t w_next = kInf;
    if (kEarly) w_next = wb + lane < b ? P[wb + lane] : kInf;
    for (uint32_t it = 0; it < kCoopWindows2; ++it) {
        if (!__any(need0 || need1)) break;
        pos_t w;
        if (kEarly) {
            w = w_next;
            if (it + 1 < kCoopWindows2) w_next = wb + 64 + lane < b ? P[wb + 64 + lane] : kInf;
        } else {
            const uint32_t idx = wb + lane;
            w = idx < b ? P[idx] : kInf;
        }
        const pos_t wlast = __shfl(w, 63);
        const bool can0 = need0 && key0 <= wlast, can1 = need1 && key1 <= wlast;
        VLG_LINK_STAT(LS_WINDOWS, 1);
        VLG_LINK_STAT(LS_PLACED, (__any(can0) ? 1 : 0) + (__any(can1) ? 1 : 0));
        uint32_t lo0 = 0, lo1 = 0;
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1) {                 // lo = elements of w[0,63) below the key (w[63] >= key for `can` lanes)
            const pos_t a0 = __shfl(w, (int)(lo0 + step - 1)), a1 = __shfl(w, (int)(lo1 + step - 1));
            lo0 += a0 < key0 ? step : 0u;
            lo1 += a1 < key1 ? step : 0u;
        }
        const pos_t at0 = __shfl(w, (int)lo0), at1 = __shfl(w, (int)lo1);
        if (can0) { j0 = wb + lo0; v0 = at0; need0 = false; }
        if (can1) { j1 = wb + lo1; v1 = at1; need1 = false; }
        wb += 64;
    }
    if (__any(need0 || need1)) {
        wb = wb < b ? wb : b;
        VLG_LINK_STAT(LS_FAR0, __any(need0) ? 1 : 0);
        VLG_LINK_STAT(LS_FAR1, __any(need1) ? 1 : 0);
        wave_far_lower_bound(P, F, wb, b, key0, need0, j0, v0, 0);
        wave_far_lower_bound(P, F, wb, b, key1, need1, j1, v1, 1);
    }
}

// ---- wave-private list tiles -----------------------------------------------------------------------------------
// A wave that needs the lower bounds of many keys in one sorted list stages the list in LDS, kTB elements at a time
// (coalesced loads that do not depend on any answer), and every lane searches its kKeys keys there: log2(kTB) LDS probes
// per key, several independent searches per lane in flight, no dependent global round trip per key.
constexpr uint32_t kKeys = 8;                 // keys per lane and block
constexpr uint32_t kBlk = 64 * kKeys;         // slots per block
constexpr uint32_t kTB = 1024;                // list elements per tile
constexpr uint32_t kKeyGroup = 4;             // searches interleaved per lane
constexpr uint32_t kMinPiece = 128;           // shorter pieces of a segment take the per-lane path

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_or(T v)
{
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform(uint64_t v)
{
    return (uint64_t)uniform((uint32_t)v) | ((uint64_t)uniform((uint32_t)(v >> 32)) << 32);
}

// Lower bound of one wave-uniform key in P[a,b): 64 probes per round narrow the range 64-fold.
template <typename pos_t>
__device__ __forceinline__ uint32_t wave_kary_lower_bound(const pos_t* __restrict__ P, uint32_t a, uint32_t b, uint64_t key)
{
    const uint32_t lane = threadIdx.x & 63;
    while (b - a > 64) {
        const uint32_t step = (b - a + 63) / 64;
        const uint64_t idx = (uint64_t)a + (uint64_t)(lane + 1) * step - 1;
        const bool in = idx < b;
        const uint64_t v = in ? (uint64_t)P[idx] : 0;
        const uint32_t c = (uint32_t)__popcll(__ballot(in && v < key));          // probes 0..c-1 are smaller than the key
        const uint64_t na = (uint64_t)a + (uint64_t)c * step;                    // <= b
        const uint64_t nb = (uint64_t)a + (uint64_t)(c + 1) * step - 1;          // probe c (if it exists) is not smaller
        a = (uint32_t)na;
        b = nb < b ? (uint32_t)nb : b;
    }
    const uint32_t idx = a + lane;
    const bool in = idx < b;
    const uint64_t v = in ? (uint64_t)P[idx] : 0;
    return a + (uint32_t)__popcll(__ballot(in && v < key));
}
// The same through the fences: the key is ranked among the list's fences (the same 64-ary search, over F), then inside one block.
template <typename pos_t>
__device__ __forceinline__ uint32_t wave_kary_lower_bound(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t a, uint32_t b, uint64_t key)
{
    if (!F) return wave_kary_lower_bound(P, a, b, key);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = wave_kary_lower_bound(F, a >> 6, b >> 6, key);            // first block of the list whose last element is >= key
    uint64_t w0 = (uint64_t)g << 6;
    const uint64_t w1 = w0 + 64 < b ? w0 + 64 : b;                               // (behind the last whole block: the rest of the list)
    if (w0 < a) w0 = a;
    const uint64_t idx = w0 + lane;
    const bool in = idx < w1;
    const uint64_t v = in ? (uint64_t)P[idx] : 0;
    return (uint32_t)w0 + (uint32_t)__popcll(__ballot(in && v < key));
}

// Lower bounds in P[.,pend) of the keys flagged in `need` (bit i = key[i]).  `wb` is a wave-uniform fence: every element
// before it is smaller than every flagged key of the wave.  j[i] = the lower bound (pend if there is none), v[i] = P[j[i]].
// The keys of the wave need not be ordered; tiles that cannot hold an answer are skipped with one probe.
template <typename pos_t>
__device__ __forceinline__ void tile_lower_bounds(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t wb, const uint32_t pend, pos_t* __restrict__ tile,
                                                  const pos_t (&key)[kKeys], uint32_t need, uint32_t (&j)[kKeys], pos_t (&v)[kKeys])
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr pos_t kInf = (pos_t)~(pos_t)0;
#pragma unroll
    for (uint32_t i = 0; i < kKeys; ++i) { j[i] = pend; v[i] = 0; }
    while (__any(need != 0) && wb < pend) {
#pragma unroll
        for (uint32_t r = 0; r < kTB / 64; ++r) {
            const uint64_t idx = (uint64_t)wb + lane + 64 * r;
            tile[lane + 64 * r] = idx < pend ? P[idx] : kInf;                    // +inf behind the list
        }
        wave_sync();
        const pos_t tile_last = tile[kTB - 1];
#pragma unroll
        for (uint32_t g = 0; g < kKeys; g += kKeyGroup) {
            bool take[kKeyGroup];
            bool any = false;
#pragma unroll
            for (uint32_t i = 0; i < kKeyGroup; ++i) { take[i] = ((need >> (g + i)) & 1) && key[g + i] <= tile_last; any |= take[i]; }
            if (!__any(any)) continue;
            uint32_t pos[kKeyGroup];
#pragma unroll
            for (uint32_t i = 0; i < kKeyGroup; ++i) pos[i] = 0;
#pragma unroll
            for (uint32_t step = kTB / 2; step; step >>= 1) {
#pragma unroll
                for (uint32_t i = 0; i < kKeyGroup; ++i)
                    if (tile[pos[i] + step - 1] < key[g + i]) pos[i] += step;
            }
#pragma unroll
            for (uint32_t i = 0; i < kKeyGroup; ++i) {
                const pos_t val = tile[pos[i]];
                if (take[i]) {                                                   // tile[kTB-1] >= key, so pos is the lower bound
                    const uint64_t at = (uint64_t)wb + pos[i];
                    j[g + i] = at < pend ? (uint32_t)at : pend;
                    v[g + i] = val;
                    need &= ~(1u << (g + i));
                }
            }
        }
        wave_sync();                                                            // the tile is overwritten next
        if (!__any(need != 0)) break;
        // next tile; when even its last element is below the smallest open key, jump to that key's lower bound
        uint64_t kmin = ~0ull;
#pragma unroll
        for (uint32_t i = 0; i < kKeys; ++i)
            if ((need >> i) & 1) kmin = (uint64_t)key[i] < kmin ? (uint64_t)key[i] : kmin;
        kmin = wave_min(kmin);
        const uint64_t nwb = (uint64_t)wb + kTB;
        if (nwb >= pend) { wb = pend; break; }
        wb = (uint32_t)nwb;
        const uint64_t probe_at = nwb + kTB - 1 < pend ? nwb + kTB - 1 : (uint64_t)pend - 1;
        if ((uint64_t)P[probe_at] < kmin) wb = wave_kary_lower_bound(P, F, (uint32_t)probe_at + 1, pend, kmin);
    }
}

// start-to-start window of one element (position x) in the key domain of the lists; false if no position can be in it
template <typename pos_t>
__device__ __forceinline__ bool gap_window(uint64_t x, uint64_t lo, uint64_t hi, pos_t& tlo, pos_t& thi);
template <>
__device__ __forceinline__ bool gap_window<uint64_t>(uint64_t x, uint64_t lo, uint64_t hi, uint64_t& tlo, uint64_t& thi)
{
    tlo = sat_add(x, lo); thi = sat_add(x, hi);
    return true;
}
template <>
__device__ __forceinline__ bool gap_window<uint32_t>(uint64_t x, uint64_t lo, uint64_t hi, uint32_t& tlo, uint32_t& thi)
{
    const uint64_t a = sat_add(x, lo), b = sat_add(x, hi);
    tlo = (uint32_t)a;
    thi = b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
    return a <= 0xFFFFFFFFull;                                                   // positions fit 32 bits
}

// Slots are dealt to waves in contiguous runs of kRun (filter_shape.hpp, which the host planner shares) so a wave can carry the
// segment it is in and the last answer of its searches from one 64-slot step to the next.
#ifndef VLG_LINK_RUN
#define VLG_LINK_RUN 2048
#endif
// a multiple of 64: runs start on a word of the feasibility bitmap, and a step writes that word whole
static_assert(VLG_LINK_RUN >= 64 && VLG_LINK_RUN % 64 == 0 && VLG_LINK_RUN <= (1u << 24), "VLG_LINK_RUN: a multiple of 64 slots");
constexpr uint32_t kLinkRun = VLG_LINK_RUN;      // slots a wave of the link pass takes (round 4, C3: 2048 -> 21.3 ms, 4096 -> 21.9 ms: what stands in front of
                                                 // a run -- segment, metadata, the first fence -- is not what the pass waits for; it is issue-bound)

__device__ __forceinline__ uint32_t seg_find(const uint32_t* __restrict__ seg_begin, uint32_t nseg, uint64_t slot)
{
    uint32_t lo = 0, hi = nseg;                        // last p with seg_begin[p] <= slot
    while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (seg_begin[mid] <= slot) lo = mid; else hi = mid; }
    return lo;
}
// the same for a whole wave asking about one slot (all 64 lanes call it): three rounds of 64 probes instead of a chain of seventeen
// dependent loads in front of the wave's run
__device__ __forceinline__ uint32_t wave_seg_find(const uint32_t* __restrict__ seg_begin, uint32_t nseg, uint64_t slot)
{
    const uint32_t lb = wave_kary_lower_bound<uint32_t>(seg_begin, 0, nseg, slot + 1);       // first segment that begins behind the slot
    return uniform(lb ? lb - 1 : 0u);
}

// ---- documents (vlg_queries_set_documents; doc_cut.hpp holds the arithmetic) -----------------------------------------------------
// What the kDocs instantiations of the passes below receive beside their other arguments: the starts of the documents with the
// sentinel n_text (B[0, nB), ascending), their fences (BF[g] = B[64 g + 63], g < nB >> 6) and, per segment of the chunk, the symbols of
// its sub-pattern -- beside SegMeta, which the passes without documents read too and which therefore stays as it is.
struct DocRef { const uint64_t* B; const uint64_t* BF; uint32_t nB; const uint64_t* seg_len; };

// The rank of x, the index of the first entry > x (nB: none), one lane on its own: the fences first (dense lines), then one block
// of 64.  Every single-lane lookup goes through it; the document of a position x < n_text = B[nB - 1] is its rank - 1 (B[0] = 0 <= x).
__device__ __forceinline__ uint64_t doc_rank_dev(const DocRef& d, uint64_t x)
{
    const uint64_t g = vlg::doc_upper_bound(d.BF, 0, d.nB >> 6, x);          // first block whose last entry is > x
    const uint64_t w0 = g << 6, w1 = w0 + 64 < d.nB ? w0 + 64 : d.nB;
    return vlg::doc_upper_bound(d.B, w0, w1, x);
}
// the first entry > x
__device__ __forceinline__ uint64_t doc_next_boundary_dev(const DocRef& d, uint64_t x)
{
    const uint64_t r = doc_rank_dev(d, x);
    return d.B[r < d.nB ? r : d.nB - 1];                                     // (x < n_text = B[nB - 1] for every list element)
}

// The documents of a wave's step: the next boundary of every lane's key (nb, the join passes) or its document (doc, the listing and
// span passes of result_passes.hpp).  Most steps lie inside the document of the step before: the wave keeps that document
// [c_lo, c_hi) and asks nothing while the step's smallest and largest key fall into it (the keys of a join step ascend from lane 0
// to lane `last`: its first and last key).  Otherwise it ranks both among the starts, once per wave (64-ary through the fences,
// wave-uniform addresses); if they share a document the step shares one boundary, else every lane bisects between the two ranks.
// The keys of the listing and span passes are < n_text = B[nB - 1] (their callers clamp), so their ranks lie in [1, nB - 1]: there
// sat_add, both clamps and the test of r1 change no value.
struct DocWave {
    uint64_t c_lo = 1, c_hi = 0;        // wave-uniform; empty at first
    uint32_t r0 = 0, r1 = 0;            // ranks (index of the first entry > key) of the step's smallest and largest key
    bool shared = false;
    // (all 64 lanes call it; xf <= xl wave-uniform)
    __device__ __forceinline__ void locate(const DocRef& d, uint64_t xf, uint64_t xl)
    {
        shared = xf >= c_lo && xl < c_hi;
        if (shared) return;
        const uint32_t top = d.nB - 1;
        r0 = wave_kary_lower_bound<uint64_t>(d.B, d.BF, 0, d.nB, sat_add(xf, 1));
        r0 = uniform(r0 < top ? r0 : top);
        r1 = wave_kary_lower_bound<uint64_t>(d.B, d.BF, r0, d.nB, sat_add(xl, 1));
        r1 = uniform(r1 < top ? r1 : top);
        c_hi = d.B[r1];
        c_lo = r1 ? d.B[r1 - 1] : 0;                                        // the last key's document: the next step most likely starts in it
        shared = r0 == r1;
    }
    __device__ __forceinline__ uint64_t nb(const DocRef& d, uint64_t x) const
    {
        if (shared) return c_hi;
        const uint64_t r = vlg::doc_upper_bound(d.B, r0, r1, x);            // in [r0, r1]: both are entries
        return d.B[r];
    }
    __device__ __forceinline__ uint32_t doc(const DocRef& d, uint64_t x) const
    {
        if (shared) return r1 - 1;
        return (uint32_t)vlg::doc_upper_bound(d.B, r0, r1, x) - 1;          // the rank of x lies in [r0, r1]
    }
};

// gap window of the element at x under documents: false = the element crosses its boundary or no next sub-pattern fits behind it;
// otherwise the upper end is capped (doc_cut.hpp)
template <typename pos_t>
__device__ __forceinline__ bool doc_window(uint64_t x, uint64_t m, uint64_t m_next, uint64_t nb, pos_t& thi)
{
    if (x >= nb || vlg::doc_straddles(x, m, nb)) return false;
    uint64_t t = (uint64_t)thi;
    if (!vlg::doc_cap_window(x, m_next, nb, t)) return false;
    thi = (pos_t)t;
    return true;
}
// restart key of a chain that ends at `end`: end + end_len, capped at the boundary nb when kDocs; false = beyond the positions' range
template <typename pos_t, bool kDocs>
__device__ __forceinline__ bool restart_key(uint64_t end, uint64_t end_len, uint64_t nb, pos_t& key)
{
    if (!kDocs) { pos_t unused; return gap_window<pos_t>(end, end_len, end_len, key, unused); }
    const uint64_t k = vlg::doc_cap_restart(end, end_len, nb);
    key = (pos_t)k;
    return k <= (uint64_t)(pos_t)~(pos_t)0;
}

// Feasibility of every slot is ONE BIT; "nearest feasible slot at or after j" is a successor query on a hierarchical
// bitset: level 0 = the feasibility bits, bit i of level l+1 = (word i of level l != 0).  A query reads one word per
// level it has to climb (almost always just level 0), so the per-level reverse scans of a 4-byte-per-slot array are gone.
constexpr uint32_t kBitLevels = 6;          // 64^6 slots > 2^32
struct FeasBits { const uint64_t* lvl[kBitLevels]; uint64_t words[kBitLevels]; };

// Kernels get level 0 as a plain pointer (the fast path) and the level table through device memory (the rare climb).
struct FeasRef { const uint64_t* lvl0; const FeasBits* table; };

__device__ __noinline__ uint32_t next_feasible_slow(const FeasBits* __restrict__ fb, uint64_t w0)
{
    // no set bit in word w0 behind the position: climb until a set bit is found, then descend to the lowest such bit
    uint64_t pos = w0 + 1;
    uint32_t l = 1;
    for (;; ++l) {
        if (l == kBitLevels) return kNone;
        const uint64_t w = pos >> 6;
        if (w >= fb->words[l]) return kNone;
        const uint64_t bits = fb->lvl[l][w] >> (pos & 63);
        if (bits) { pos += (uint64_t)__ffsll((long long)bits) - 1; break; }
        pos = w + 1;
    }
    while (l) {                                         // pos = index of a non-zero word of level l-1
        --l;
        const uint64_t bits = fb->lvl[l][pos];
        pos = pos * 64 + (uint64_t)__ffsll((long long)bits) - 1;
    }
    return pos < 0xFFFFFFFFull ? (uint32_t)pos : kNone;
}
__device__ __forceinline__ uint32_t next_feasible(const FeasRef& fb, uint64_t j)
{
    const uint64_t w0 = j >> 6;
    const uint64_t bits = fb.lvl0[w0] >> (j & 63);                   // almost always answers the query
    if (bits) return (uint32_t)(j + (uint64_t)__ffsll((long long)bits) - 1);
    return next_feasible_slow(fb.table, w0);
}
__device__ __forceinline__ bool is_feasible(const FeasRef& fb, uint64_t e) { return (fb.lvl0[e >> 6] >> (e & 63)) & 1; }

// one level of the summary: out word i = bitmap of (in[64 i + b] != 0)
__global__ void bits_summary_kernel(const uint64_t* __restrict__ in, uint64_t in_words, uint64_t w0, uint64_t w1 /* output word range */,
                                    uint64_t* __restrict__ out)
{
    for (uint64_t i = w0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < w1; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < 64; ++b) {
            const uint64_t idx = i * 64 + b;
            if (idx < in_words && in[idx]) v |= 1ull << b;
        }
        out[i] = v;
    }
}

// single-sub-pattern queries (class dist 0): every element is a feasible chain that ends at itself
// kDocs: except the elements that cross a document boundary
template <typename pos_t, bool kDocs>
__device__ __forceinline__ void join_init_body(const pos_t* __restrict__ P, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                               const SegMeta* __restrict__ sm, uint64_t r0, uint64_t r1, uint64_t* __restrict__ fbits,
                                               pos_t* __restrict__ endp, const DocRef& dr)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t run_begin = r0 + wave * kRun;
    if (run_begin >= r1) return;
    const uint64_t run_end = run_begin + kRun < r1 ? run_begin + kRun : r1;
    uint32_t s_w = seg_find(seg_begin, nseg, run_begin);
    for (uint64_t base = run_begin; base < run_end; base += 64) {
        const uint64_t e = base + lane;
        bool inside = e < run_end;
        if (e < run_end) {
            uint32_t s = s_w;
            while (seg_begin[s + 1] <= e) ++s;
            const SegMeta m = sm[s];
            const pos_t x = P[phys_of(m, (uint32_t)e)];
            endp[e] = x;
            if (kDocs) {
                const uint64_t nb = doc_next_boundary_dev(dr, (uint64_t)x);
                inside = (uint64_t)x < nb && !vlg::doc_straddles((uint64_t)x, dr.seg_len[s], nb);
            }
            s_w = s;
        }
        const unsigned long long act = __ballot(inside);
        if (lane == 0) fbits[base >> 6] = act;         // class ranges and runs are 64-aligned: one word per step
        s_w = __shfl(s_w, 0);                          // lane 0 is always in range and holds the smallest segment
    }
}
template <typename pos_t>
__global__ void __launch_bounds__(256) join_init_kernel(const pos_t* __restrict__ P, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                                        const SegMeta* __restrict__ sm, uint64_t r0, uint64_t r1, uint64_t* __restrict__ fbits,
                                                        pos_t* __restrict__ endp)
{
    join_init_body<pos_t, false>(P, seg_begin, nseg, sm, r0, r1, fbits, endp, DocRef());
}
template <typename pos_t>
__global__ void __launch_bounds__(256) join_init_docs_kernel(const pos_t* __restrict__ P, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                                             const SegMeta* __restrict__ sm, uint64_t r0, uint64_t r1, uint64_t* __restrict__ fbits,
                                                             pos_t* __restrict__ endp, DocRef dr)
{
    join_init_body<pos_t, true>(P, seg_begin, nseg, sm, r0, r1, fbits, endp, dr);
}

// what a slot does with its lower bound j (value v) in the next list: the first FEASIBLE element at or after it, if still
// inside the window, becomes its link
// (`end`: the chain end of a slot that is ok; store_end false: the caller uses it at once and nobody reads endp[e] -- level 0 of the
// fused pass)
template <typename pos_t, bool kLast>
__device__ __forceinline__ bool link_finish(const pos_t* __restrict__ P, const SegMeta& nx, const FeasRef& fb, uint32_t e, bool want, uint32_t j,
                                            pos_t v, pos_t thi, pos_t* __restrict__ endp, uint32_t* __restrict__ link, bool store_end, pos_t& end)
{
    bool ok = false;
    if (want && j < nx.pend) {
        if (kLast) {
            ok = v <= thi;
            if (ok) { if (link) link[e] = j; if (store_end) endp[e] = v; end = v; }
        } else {
            const uint32_t at = nx.begin + (j - nx.pbegin);
            const uint32_t ej = next_feasible(fb, at);     // nearest feasible logical element at or after it
            if (ej < nx.end) {
                const pos_t pv = ej == at ? v : P[phys_of(nx, ej)];
                if (pv <= thi) { ok = true; if (link) link[e] = ej; end = endp[ej]; if (store_end) endp[e] = end; }
            }
        }
    }
    return ok;
}

// ---- the level-0 jump inside the link pass -----------------------------------------------------------------------------------------
// jump[a] of a level-0 slot is the lower bound of end(a) + end_len in the slot's OWN list, behind the slot.  A wave of the link pass
// that has just linked a step of level-0 slots holds their chain ends and the list elements themselves in registers; the answers
// lie a few elements on (the window is two gaps and the pattern lengths wide), so the wave stages kStretch elements of the list from
// the step's first slot on in LDS -- its own keys from registers, the rest is the next steps' keys, which it prefetches anyway -- and
// every lane bisects there.  What it writes is the RAW target, the lower bound as a logical slot: whether that slot is feasible is
// still being decided by other waves of the same launch, so the tile pass settles it (chain_tiles_kernel).
constexpr uint32_t kStretch = 256;          // list elements staged per step (64 or 128 of them are the step's own)

// keys the staged stretch does not reach: the blocked search from its end (a call, to keep it out of the link loop's registers)
template <typename pos_t>
__device__ __noinline__ uint32_t jump_far_lower_bound(const pos_t* __restrict__ P, const pos_t* __restrict__ F, uint32_t wb, uint32_t b, pos_t key, bool need)
{
    uint32_t j = b;
    pos_t v = 0;
    wave_far_lower_bound(P, F, wb < b ? wb : b, b, key, need, j, v);
    return j < b ? j : b;
}

// Raw jump targets of kN keys per lane (key i belongs to the slot at tile offset 64 i + lane) in the list of segment m, whose
// elements [pb, pb + kStretch) are staged in `tile` (+inf behind the list).  kNone: no key, or no element at or after it.
template <typename pos_t, uint32_t kN>
__device__ __forceinline__ void stretch_jump_targets(const pos_t* __restrict__ P, const pos_t* __restrict__ F, const SegMeta& m, uint32_t pb,
                                                     const pos_t* __restrict__ tile, const pos_t (&key)[kN], const bool (&need)[kN], uint32_t (&out)[kN])
{
    const uint32_t lane = threadIdx.x & 63;
    const pos_t tile_last = tile[kStretch - 1];
    uint32_t pos[kN];
    bool far[kN], any_far = false;
#pragma unroll
    for (uint32_t i = 0; i < kN; ++i) { pos[i] = 0; far[i] = need[i] && key[i] > tile_last; any_far |= far[i]; }
#pragma unroll
    for (uint32_t step = kStretch / 2; step; step >>= 1) {
#pragma unroll
        for (uint32_t i = 0; i < kN; ++i)
            if (tile[pos[i] + step - 1] < key[i]) pos[i] += step;
    }
    uint32_t j[kN];
#pragma unroll
    for (uint32_t i = 0; i < kN; ++i) {
        const uint32_t own = 64 * i + lane;                            // an answer lies behind its own element (end_len >= 1)
        j[i] = pb + (pos[i] > own ? pos[i] : own + 1);
    }
    if (__any(any_far)) {                                              // tile_last is an element of the list (+inf is above every key)
#pragma unroll
        for (uint32_t i = 0; i < kN; ++i) {
            const uint32_t jf = jump_far_lower_bound<pos_t>(P, F, pb + kStretch, m.pend, key[i], far[i]);
            if (far[i]) j[i] = jf;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kN; ++i) out[i] = need[i] && j[i] < m.pend ? m.begin + (j[i] - m.pbegin) : kNone;
}

// (link == nullptr: only the chain ends are wanted -- first positions without tuples)
// link pass over the class [r0,r1) of slots that have `dist` sub-patterns after them (kLast: dist == 1, the next list is the
// query's last one: all its elements are feasible and it has no join state).
// Steps that lie inside one segment (almost all of them: lists are long) keep the segment's metadata in registers,
// search as a wave behind the previous step's answer and have the next step's positions already in flight.
// Slot numbers are 32-bit inside a chunk (r1 <= 0xF0000000 + alignment), so all loop arithmetic is.
// kJump: the pass also leaves jump[] for the slots of the class inside [jlo, jhi), the slot range of the chain passes: the raw target
// (stretch_jump_targets above) for the slots of a first list, whose endp[] it then does not write -- the jump was its only reader --
// and kNone for every other level.
// kDocs (a batch with documents, DocRef above): an element whose sub-pattern crosses its next boundary nb(x) links to nothing, the
// window of the others ends at min(x + hi, nb(x) - symbols of the next sub-pattern), and the restart key of a level-0 slot is capped
// at nb(x).  The searches themselves are the same: the lower bound of tlo is found for every element and the next step's fence comes
// from it; only what link_finish may accept changes.  The body is shared; the kernels without documents instantiate it with kDocs =
// false and are what they were.
template <typename pos_t, bool kLast, bool kJump, bool kDocs>
__device__ __forceinline__ void join_link_body(const pos_t* __restrict__ P, const pos_t* __restrict__ F /* fences of P, or null */,
                                               const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                               const SegMeta* __restrict__ sm, uint32_t r0, uint32_t r1,
                                               FeasRef fb, uint64_t* __restrict__ fbits_out,
                                               pos_t* __restrict__ endp, uint32_t* __restrict__ link,
                                               const QueryMeta* __restrict__ qm, uint32_t jlo, uint32_t jhi, uint32_t* __restrict__ jump,
                                               const DocRef& dr)
{
    __shared__ pos_t s_stretch[kJump ? 4 : 1][kJump ? kStretch : 1];
    constexpr pos_t kInf = (pos_t)~(pos_t)0;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave * kLinkRun >= (uint64_t)(r1 - r0)) return;
    pos_t* const tile = s_stretch[kJump ? threadIdx.x >> 6 : 0];
    const uint32_t run_begin = r0 + (uint32_t)wave * kLinkRun;
    const uint32_t run_end = r1 - run_begin > kLinkRun ? run_begin + kLinkRun : r1;
    uint32_t s_w = wave_seg_find(seg_begin, nseg, run_begin);     // wave-uniform: segment of `base`
    uint32_t seg_end = seg_begin[s_w + 1];
    SegMeta m = sm[s_w], nx = sm[m.next];
    bool lvl0 = kJump && m.level == 0;                             // wave-uniform: the steps inside this segment find their jumps
    uint64_t end_len = lvl0 ? qm[m.query].end_len : 0;
    uint64_t m_len = kDocs ? dr.seg_len[s_w] : 0, m_next = kDocs ? dr.seg_len[m.next] : 0;     // wave-uniform: symbols of the segment's sub-pattern and of the next
    DocWave dw;
    uint32_t hint_seg = kNone, hint = 0;                           // answer of the last lane of the previous step and its segment
    pos_t x_pre = 0, x_pre1 = 0;
    bool have_pre = false, have_pre1 = false;
    for (uint32_t base = run_begin; base < run_end; base += 64) {
        if (base >= seg_end) {                                     // entered a new segment (skips empty ones)
            while (seg_begin[s_w + 1] <= base) ++s_w;
            seg_end = seg_begin[s_w + 1];
            m = sm[s_w]; nx = sm[m.next];
            lvl0 = kJump && m.level == 0;
            end_len = lvl0 ? qm[m.query].end_len : 0;
            if (kDocs) { m_len = dr.seg_len[s_w]; m_next = dr.seg_len[m.next]; }
            have_pre = false; have_pre1 = false;
        }
        if (run_end - base >= 128 && base + 127 < seg_end) {
            // ---- two full steps inside one segment: 128 keys per window ---------------------------------
            const uint32_t e0 = base + lane, e1 = e0 + 64;
            const pos_t x0 = have_pre ? x_pre : P[phys_of(m, e0)];
            const pos_t x1 = have_pre1 ? x_pre1 : P[phys_of(m, e1)];
            const uint32_t left = run_end - base - 128;            // slots of the run behind this pair of steps
            const uint32_t room = seg_end - base - 128;            // and of the segment
            have_pre = left > 0 && (left < 64 ? left : 64u) <= room;
            have_pre1 = left >= 128 && room >= 128;
            if (lvl0) {                                            // the stretch behind the pair: the next pair's keys where there is one
                x_pre = e0 + 128 < m.end ? P[phys_of(m, e0 + 128)] : kInf;
                x_pre1 = e1 + 128 < m.end ? P[phys_of(m, e1 + 128)] : kInf;
            } else {
                if (have_pre) x_pre = e0 + 128 < run_end ? P[phys_of(m, e0 + 128)] : (pos_t)0;
                if (have_pre1) x_pre1 = P[phys_of(m, e1 + 128)];
            }
            pos_t tlo0, thi0, tlo1, thi1, v0 = 0, v1 = 0;
            const bool want0 = gap_window<pos_t>((uint64_t)x0, nx.lo, nx.hi, tlo0, thi0);
            const bool want1 = gap_window<pos_t>((uint64_t)x1, nx.lo, nx.hi, tlo1, thi1);
            uint32_t j0 = nx.pend, j1 = nx.pend;
            if (hint_seg != s_w)                                   // first step of the run in this segment: the smallest key's bound is the fence
                hint = wave_kary_lower_bound(P, F, nx.pbegin, nx.pend, (uint64_t)__shfl(tlo0, 0));
            // (the early window load: not with documents and 64-bit positions, where its register costs the kLast pass a wave per SIMD
            // -- 74 VGPRs against 72, six waves against seven: the resource table of DESIGN 9)
            wave_lower_bound2<pos_t, VLG_LINK_EARLY != 0 && !(kDocs && sizeof(pos_t) == 8)>(P, F, hint, nx.pend, tlo0, want0, tlo1, want1, j0, v0, j1, v1);
            if (!want0) j0 = nx.pend;
            if (!want1) j1 = nx.pend;
            bool in0 = want0, in1 = want1;                         // (the searches above ran for every element: j1 is the next step's fence)
            uint64_t nb0 = 0, nb1 = 0;
            if (kDocs) {
                dw.locate(dr, (uint64_t)__shfl(x0, 0), (uint64_t)__shfl(x1, 63));
                nb0 = dw.nb(dr, (uint64_t)x0); nb1 = dw.nb(dr, (uint64_t)x1);
                in0 = want0 && doc_window<pos_t>((uint64_t)x0, m_len, m_next, nb0, thi0);
                in1 = want1 && doc_window<pos_t>((uint64_t)x1, m_len, m_next, nb1, thi1);
            }
            pos_t end0 = 0, end1 = 0;
            const bool ok0 = link_finish<pos_t, kLast>(P, nx, fb, e0, in0, j0, v0, thi0, endp, link, !lvl0, end0);
            const bool ok1 = link_finish<pos_t, kLast>(P, nx, fb, e1, in1, j1, v1, thi1, endp, link, !lvl0, end1);
            const unsigned long long okm0 = __ballot(ok0), okm1 = __ballot(ok1);
            if (lane == 0) { fbits_out[base >> 6] = okm0; fbits_out[(base >> 6) + 1] = okm1; }
            if (kJump) {
                if (lvl0) {
                    pos_t key[2] = {0, 0};
                    const bool need[2] = {ok0 && restart_key<pos_t, kDocs>((uint64_t)end0, end_len, nb0, key[0]),
                                          ok1 && restart_key<pos_t, kDocs>((uint64_t)end1, end_len, nb1, key[1])};
                    tile[lane] = x0; tile[64 + lane] = x1; tile[128 + lane] = x_pre; tile[192 + lane] = x_pre1;
                    wave_sync();
                    uint32_t out[2];
                    stretch_jump_targets<pos_t, 2>(P, F, m, phys_of(m, base), tile, key, need, out);
                    wave_sync();                                   // the next step overwrites the stretch
                    jump[e0] = out[0]; jump[e1] = out[1];
                } else {
                    if (e0 >= jlo && e0 < jhi) jump[e0] = kNone;
                    if (e1 >= jlo && e1 < jhi) jump[e1] = kNone;
                }
            }
            hint_seg = s_w;
            hint = __shfl(j1, 63);
            base += 64;                                            // the loop adds the other 64
            continue;
        }
        have_pre1 = false;
        const uint32_t e = base + lane;
        const bool active = e < run_end;
        const uint32_t step_last = run_end - base > 64 ? base + 63 : run_end - 1;
        uint32_t j = 0, s_last = s_w;
        if (step_last < seg_end) {
            // ---- fast path: one segment ---------------------------------------------------------------
            const pos_t x = have_pre ? x_pre : (active ? P[phys_of(m, e)] : (pos_t)0);
            const uint32_t en = e + 64;                            // next step's position, in flight during the search
            have_pre = run_end - base > 64 && (run_end - base > 128 ? base + 127 : run_end - 1) < seg_end;
            if (have_pre) x_pre = en < run_end ? P[phys_of(m, en)] : (pos_t)0;
            pos_t tlo, thi, v = 0;
            const bool want = gap_window<pos_t>((uint64_t)x, nx.lo, nx.hi, tlo, thi) && active;    // false: no position can be in the window
            j = nx.pend;
            if (hint_seg != s_w) hint = wave_kary_lower_bound(P, F, nx.pbegin, nx.pend, (uint64_t)__shfl(tlo, 0));
            j = wave_lower_bound(P, F, hint, nx.pend, tlo, want, v);
            if (!want) j = nx.pend;
            bool in = want;
            uint64_t nb = 0;
            if (kDocs) {                                           // (lanes behind the run's end hold no key: the last key is lane step_last's)
                dw.locate(dr, (uint64_t)__shfl(x, 0), (uint64_t)__shfl(x, (int)(step_last - base)));
                nb = dw.nb(dr, (uint64_t)x);
                in = want && doc_window<pos_t>((uint64_t)x, m_len, m_next, nb, thi);
            }
            pos_t end = 0;
            const bool ok = link_finish<pos_t, kLast>(P, nx, fb, e, in, j, v, thi, endp, link, !lvl0, end);
            const unsigned long long okm = __ballot(ok);
            if (lane == 0) fbits_out[base >> 6] = okm;
            if (kJump) {
                if (lvl0) {                                        // (a run or a list ends here: the stretch is loaded, not carried)
                    pos_t key[1] = {0};
                    const bool need[1] = {ok && restart_key<pos_t, kDocs>((uint64_t)end, end_len, nb, key[0])};
                    tile[lane] = active ? x : (e < m.end ? P[phys_of(m, e)] : kInf);
#pragma unroll
                    for (uint32_t r = 1; r < kStretch / 64; ++r) tile[64 * r + lane] = e + 64 * r < m.end ? P[phys_of(m, e + 64 * r)] : kInf;
                    wave_sync();
                    uint32_t out[1];
                    stretch_jump_targets<pos_t, 1>(P, F, m, phys_of(m, base), tile, key, need, out);
                    wave_sync();
                    if (active) jump[e] = out[0];
                } else if (active && e >= jlo && e < jhi) {
                    jump[e] = kNone;
                }
            }
        } else {
            // ---- a segment border inside the step: every lane looks its own segment up ------------------
            have_pre = false;
            uint32_t s = s_w;
            bool ok = false;
            if (active) {
                while (seg_begin[s + 1] <= e) ++s;
                const SegMeta ml = sm[s];
                const SegMeta nl = sm[ml.next];
                const uint64_t x = P[phys_of(ml, e)];
                const uint64_t tlo = sat_add(x, nl.lo);
                uint64_t thi = sat_add(x, nl.hi), nb = 0;
                j = gallop_lower_bound(P, (s == hint_seg) ? hint : nl.pbegin, nl.pend, tlo);
                const bool first = kJump && ml.level == 0;         // a slot of a first list: its end goes into its jump, not into endp
                pos_t end = 0;
                bool in = e < ml.end;                              // padding slots between classes belong to no segment
                if (kDocs && in) {
                    nb = doc_next_boundary_dev(dr, x);
                    in = doc_window<uint64_t>(x, dr.seg_len[s], dr.seg_len[ml.next], nb, thi);
                }
                if (in) {
                    if (kLast) {
                        ok = j < nl.pend && (uint64_t)P[j] <= thi;
                        if (ok) { if (link) link[e] = j; end = P[j]; if (!first) endp[e] = end; }
                    } else if (j < nl.pend) {
                        const uint32_t ej = next_feasible(fb, (uint64_t)nl.begin + (j - nl.pbegin));
                        if (ej < nl.end && (uint64_t)P[phys_of(nl, ej)] <= thi) {
                            ok = true;
                            if (link) link[e] = ej;
                            end = endp[ej];
                            if (!first) endp[e] = end;
                        }
                    }
                }
                if (kJump && e >= jlo && e < jhi) {
                    uint32_t out = kNone;
                    if (first && ok) {                             // (a key beyond the positions' range has no element at or after it)
                        const uint64_t lim = kDocs ? vlg::doc_cap_restart((uint64_t)end, qm[ml.query].end_len, nb) : sat_add((uint64_t)end, qm[ml.query].end_len);
                        const uint32_t jp = gallop_lower_bound(P, phys_of(ml, e) + 1, ml.pend, lim);
                        if (jp < ml.pend) out = ml.begin + (jp - ml.pbegin);
                    }
                    jump[e] = out;
                }
            }
            const unsigned long long okm = __ballot(ok);
            if (lane == 0) fbits_out[base >> 6] = okm;
            s_last = __shfl(s, (int)(step_last - base));
        }
        hint_seg = s_last;
        hint = __shfl(j, (int)(step_last - base));
    }
}
template <typename pos_t, bool kLast, bool kJump>
__global__ void __launch_bounds__(256) join_link_kernel(const pos_t* __restrict__ P, const pos_t* __restrict__ F /* fences of P, or null */,
                                                        const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                                        const SegMeta* __restrict__ sm, uint32_t r0, uint32_t r1,
                                                        FeasRef fb, uint64_t* __restrict__ fbits_out,
                                                        pos_t* __restrict__ endp, uint32_t* __restrict__ link,
                                                        const QueryMeta* __restrict__ qm, uint32_t jlo, uint32_t jhi, uint32_t* __restrict__ jump)
{
    join_link_body<pos_t, kLast, kJump, false>(P, F, seg_begin, nseg, sm, r0, r1, fb, fbits_out, endp, link, qm, jlo, jhi, jump, DocRef());
}
template <typename pos_t, bool kLast, bool kJump>
__global__ void __launch_bounds__(256) join_link_docs_kernel(const pos_t* __restrict__ P, const pos_t* __restrict__ F, const uint32_t* __restrict__ seg_begin,
                                                             uint32_t nseg, const SegMeta* __restrict__ sm, uint32_t r0, uint32_t r1, FeasRef fb,
                                                             uint64_t* __restrict__ fbits_out, pos_t* __restrict__ endp, uint32_t* __restrict__ link,
                                                             const QueryMeta* __restrict__ qm, uint32_t jlo, uint32_t jhi, uint32_t* __restrict__ jump, DocRef dr)
{
    join_link_body<pos_t, kLast, kJump, true>(P, F, seg_begin, nseg, sm, r0, r1, fb, fbits_out, endp, link, qm, jlo, jhi, jump, dr);
}

// jump[e] for level-0 elements: first feasible element of list 0 at or after end(e)+end_len (kNone = none);
// slots of other levels get kNone so the tile pass can treat every slot alike.
// Same walk as the link pass; the list searched is the element's own (the answers lie behind the element itself).
// The pass of the single-list queries (class 0: every element is feasible and ends at itself, join_init_kernel), and of every
// class when the workspace option "fuse_jump" is 0; with longer queries the link pass finds the jumps of its level-0 slots itself.
// kDocs: the restart key is capped at the next boundary of the slot's own element (every lane looks its boundary up on its own: this
// pass runs for the single-list queries and with "fuse_jump" = 0 only).
template <typename pos_t, bool kDocs>
__device__ __forceinline__ void join_jump_body(const pos_t* __restrict__ P, const pos_t* __restrict__ F, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                               const SegMeta* __restrict__ sm, const QueryMeta* __restrict__ qm, uint64_t r0,
                                               uint64_t r1, FeasRef fb, const pos_t* __restrict__ endp,
                                               uint32_t* __restrict__ jump, const DocRef& dr)
{
    __shared__ pos_t s_tile[4][kTB];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t wave = uniform(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint64_t run_begin = r0 + wave * kRun;
    if (run_begin >= r1) return;
    const uint64_t run_end = run_begin + kRun < r1 ? run_begin + kRun : r1;
    pos_t* tile = s_tile[wv];
    uint32_t s = wave_seg_find(seg_begin, nseg, run_begin);
    uint64_t cur = run_begin;
    while (cur < run_end) {
        while (seg_begin[s + 1] <= cur) ++s;
        const SegMeta m = sm[s];
        const uint64_t seg_end = seg_begin[s + 1];                     // beyond m.end only behind the last segment of a class
        if (m.level != 0) {
            // ---- not a first sub-pattern: no chain passes through these slots --------------------------------
            const uint64_t piece_end = run_end < seg_end ? run_end : seg_end;
            for (uint64_t a = cur + lane; a < piece_end; a += 64) jump[a] = kNone;
            cur = piece_end;
        } else if (m.end - m.begin >= kMinPiece && cur < m.end) {
            // ---- long list: blocks of kBlk slots against tiles of the same list ------------------------------
            const uint64_t piece_end = run_end < m.end ? run_end : (uint64_t)m.end;
            const uint64_t end_len = qm[m.query].end_len;
            uint32_t fence = 0;
            for (uint64_t blk0 = cur; blk0 < piece_end; blk0 += kBlk) {
                const uint64_t blk1 = blk0 + kBlk < piece_end ? blk0 + kBlk : piece_end;
                pos_t key[kKeys], v[kKeys];
                uint32_t j[kKeys];
                uint32_t need = 0;
#pragma unroll
                for (uint32_t i = 0; i < kKeys; ++i) {
                    const uint64_t a = blk0 + lane + 64 * i;
                    key[i] = 0;
                    if (a < blk1 && is_feasible(fb, a)) {                                  // feasible start
                        const uint64_t nb = kDocs ? doc_next_boundary_dev(dr, (uint64_t)P[phys_of(m, (uint32_t)a)]) : 0;
                        if (restart_key<pos_t, kDocs>((uint64_t)endp[a], end_len, nb, key[i])) need |= 1u << i;
                    }
                }
                const uint32_t own = phys_of(m, (uint32_t)blk0) + 1;                       // every answer lies behind its own element
                fence = fence > own ? fence : own;
                const uint32_t asked = need;
                tile_lower_bounds<pos_t>(P, F, fence, m.pend, tile, key, need, j, v);
                uint32_t jm = fence;
#pragma unroll
                for (uint32_t i = 0; i < kKeys; ++i) {
                    const uint64_t a = blk0 + lane + 64 * i;
                    if (a < blk1) {
                        uint32_t out = kNone;
                        if ((asked >> i) & 1) {
                            jm = j[i] > jm ? j[i] : jm;
                            if (j[i] < m.pend) {
                                const uint32_t ej = next_feasible(fb, (uint64_t)m.begin + (j[i] - m.pbegin));
                                if (ej < m.end) out = ej;
                            }
                        }
                        jump[a] = out;
                    }
                }
                // ends ascend along a list: the largest answer of this block is a fence for the next one
                jm = wave_max<uint32_t>(jm);
                fence = jm;
            }
            cur = piece_end;
        } else {
            // ---- short lists (and the slots between two classes): 64 slots, every lane on its own --------------
            const uint64_t e = cur + lane;
            const uint64_t grp_end = cur + 64 < run_end ? cur + 64 : run_end;
            if (e < grp_end) {
                uint32_t sl = s;
                while (seg_begin[sl + 1] <= e) ++sl;
                const SegMeta ml = sm[sl];
                uint32_t out = kNone;
                if (ml.level == 0 && e < ml.end) {
                    if (is_feasible(fb, e)) {
                        const uint64_t lim = kDocs ? vlg::doc_cap_restart((uint64_t)endp[e], qm[ml.query].end_len,
                                                                          doc_next_boundary_dev(dr, (uint64_t)P[phys_of(ml, (uint32_t)e)]))
                                                   : sat_add((uint64_t)endp[e], qm[ml.query].end_len);
                        const uint32_t jp = gallop_lower_bound(P, phys_of(ml, (uint32_t)e) + 1, ml.pend, lim);
                        if (jp < ml.pend) {
                            const uint32_t ej = next_feasible(fb, (uint64_t)ml.begin + (jp - ml.pbegin));
                            if (ej < ml.end) out = ej;
                        }
                    }
                }
                jump[e] = out;
            }
            cur = grp_end;
        }
    }
}
template <typename pos_t>
__global__ void __launch_bounds__(256) join_jump_kernel(const pos_t* __restrict__ P, const pos_t* __restrict__ F, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                                        const SegMeta* __restrict__ sm, const QueryMeta* __restrict__ qm, uint64_t r0,
                                                        uint64_t r1, FeasRef fb, const pos_t* __restrict__ endp,
                                                        uint32_t* __restrict__ jump)
{
    join_jump_body<pos_t, false>(P, F, seg_begin, nseg, sm, qm, r0, r1, fb, endp, jump, DocRef());
}
template <typename pos_t>
__global__ void __launch_bounds__(256) join_jump_docs_kernel(const pos_t* __restrict__ P, const pos_t* __restrict__ F, const uint32_t* __restrict__ seg_begin,
                                                             uint32_t nseg, const SegMeta* __restrict__ sm, const QueryMeta* __restrict__ qm, uint64_t r0,
                                                             uint64_t r1, FeasRef fb, const pos_t* __restrict__ endp, uint32_t* __restrict__ jump, DocRef dr)
{
    join_jump_body<pos_t, true>(P, F, seg_begin, nseg, sm, qm, r0, r1, fb, endp, jump, dr);
}

// positions -> (document, offset): vlg_documents_locate_batch
__global__ void __launch_bounds__(256) doc_locate_kernel(DocRef dr, const uint64_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ doc,
                                                         uint64_t* __restrict__ offset)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t x = pos[i];
        uint64_t dj = ~0ull, off = ~0ull;
        if (x < dr.B[dr.nB - 1]) {
            dj = doc_rank_dev(dr, x) - 1;                                // (B[0] = 0 <= x: the rank is at least 1)
            off = x - dr.B[dj];
        }
        if (doc) doc[i] = dj;
        if (offset) offset[i] = off;
    }
}

// The chain a -> jump[a] -> ... of a query is resolved in three data-parallel passes instead of one serial walk:
//   tiles : inside every tile of kTile slots, pointer doubling in LDS gives each slot its exit (first chain
//           element beyond the tile) and the number of chain elements it covers inside the tile;
//   walk  : one lane per query hops tile to tile (a heavy query costs |list|/kTile dependent loads, not |matches|),
//           leaving one record per tile visited and the query's match count;
//   emit  : one lane per record lists the matches inside its tile.
constexpr uint32_t kTile = 1024;
constexpr uint32_t kTileFeasWords = 32;     // feasibility words the tile pass stages: the tile's own 16 and as many behind them

// per-slot state of the doubling, one word: [0,10) next element inside the tile, bit 10 = chain left the tile,
// [11,21) chain elements covered so far minus one, [21,31) last chain element inside the tile
//
// The pass first SETTLES the jump words, in place: the link pass leaves the raw target of a slot, the lower bound of its key in its own
// list, because the feasibility of that list was still being written when it ran.  The settled word is the first feasible slot at or
// after the raw one, if that is still a slot of the same segment (padding slots are never feasible, so "below the begin of the next
// segment" is "below the end of this one"), else kNone.  A word that is settled already -- the separate jump pass writes such -- is a
// feasible slot of its own segment and stays as it is.
__device__ __forceinline__ void chain_tiles_doubling(uint32_t* __restrict__ jump, uint64_t t0, uint64_t r1, const FeasRef& fb,
                                                     const uint32_t* __restrict__ seg_begin, uint32_t nseg, uint2* __restrict__ xh)
{
    static_assert(kTile == 1024, "the packed word holds 10-bit tile offsets");
    __shared__ uint32_t s_ext[kTile];
    __shared__ uint32_t s_st[2][kTile];
    constexpr uint32_t kDone = 1u << 10;
    __shared__ uint64_t s_fb[kTileFeasWords];
    const uint64_t base = t0 + (uint64_t)blockIdx.x * kTile;
    const uint64_t tile_end = base + kTile;
    // The targets lie a few slots behind their slot: the feasibility words of the tile and of the slots behind it are staged in LDS
    // by loads that wait for nothing, so a settled word costs no second round trip after the jump word's own.  (every target is a
    // slot below r1, so no word behind that of r1 - 1 is asked for)
    uint32_t jw[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t e = base + threadIdx.x + 256 * r;
        jw[r] = e < r1 ? jump[e] : kNone;
    }
    const uint64_t w_base = base >> 6;
    if (threadIdx.x < kTileFeasWords) s_fb[threadIdx.x] = w_base + threadIdx.x <= ((r1 - 1) >> 6) ? fb.lvl0[w_base + threadIdx.x] : 0;
    __syncthreads();
    uint32_t moved = 0;                                              // bit r: the target of slot r is not the raw one
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t j = jw[r];
        if (j != kNone) {
            const uint64_t wi = ((uint64_t)j >> 6) - w_base;
            const uint64_t bits = wi < kTileFeasWords ? s_fb[wi] >> (j & 63) : 0;
            const uint32_t ej = bits ? j + (uint32_t)__ffsll((long long)bits) - 1 : next_feasible(fb, j);
            moved |= (uint32_t)(ej != j) << r;
            jw[r] = ej;
        }
    }
    // a target that moved may have left its segment: the segment of the tile's first slot, once per wave that has such a target; the
    // lanes walk on from it only where a border falls inside the tile
    if (__any(moved != 0)) {
        const uint32_t s_t = wave_seg_find(seg_begin, nseg, base);
        const uint32_t t_next = seg_begin[s_t + 1];                  // begin of the next segment with slots (seg_begin[nseg + 1] = 2^32 - 1)
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint64_t e = base + threadIdx.x + 256 * r;
            if ((moved >> r) & 1) {
                uint32_t lim = t_next;
                if ((uint64_t)lim < tile_end) {
                    uint32_t s = s_t;
                    while (seg_begin[s + 1] <= e) ++s;
                    lim = seg_begin[s + 1];
                }
                if (jw[r] >= lim) jw[r] = kNone;
                jump[e] = jw[r];
            }
        }
    }
    uint32_t st[4];
    bool open = false;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t li = threadIdx.x + 256 * r;
        const uint32_t j = jw[r];
        const bool inside = j != kNone && (uint64_t)j < tile_end;
        s_ext[li] = j;                                   // where the chain goes when this is its last element inside the tile
        st[r] = (inside ? (uint32_t)(j - base) : kDone) | (li << 21);
        s_st[0][li] = st[r];
        open |= inside;
    }
    uint32_t cur = 0;
    // jump[e] > e, so a chain inside a tile has fewer than 2^10 elements: at most 10 doublings
    for (uint32_t round = 0; round < 10 && __syncthreads_or(open); ++round) {
        open = false;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t li = threadIdx.x + 256 * r;
            if (!(st[r] & kDone)) {
                const uint32_t nx = s_st[cur][st[r] & 1023u];
                const uint32_t hops = ((st[r] >> 11) & 1023u) + ((nx >> 11) & 1023u) + 1;
                st[r] = (nx & 0x7FFu) | (hops << 11) | (nx & (1023u << 21));
                open |= !(st[r] & kDone);
            }
            s_st[cur ^ 1][li] = st[r];
        }
        cur ^= 1;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t li = threadIdx.x + 256 * r;
        const uint64_t e = base + li;
        if (e < r1) xh[e] = make_uint2(s_ext[st[r] >> 21], ((st[r] >> 11) & 1023u) + 1);
    }
}

// The same words by one backward scan (workspace option "tile_scan", the default).  jump[e] > e: the chains of a tile form an ORDERED
// forest, every target lies behind its slot, so a slot is finished by one look-up once everything behind it is.  Two levels keep that
// parallel: the tile is 32 blocks of 32 slots,
//   phase 1 : a lane per block walks it from its last slot to its first; a slot whose target lies inside the block takes the target's
//             state (final for the block already), one whose target lies outside keeps its own;
//   phase 2 : the blocks from the last to the first, a lane per slot; a slot whose chain leaves its block composes with the slot it
//             lands on, which lies in a later block and is final.
// 32 + 32 dependent LDS steps whatever the chains look like, against up to 10 rounds over all slots.  A tile belongs to HALF a wave
// (32 lanes, 32 slots each; a wave takes two tiles, a workgroup eight), so nothing here waits for a workgroup barrier.  The state
// word is the doubling's.  The state array is padded by one word per block: in phase 1 lane l addresses slot 32 l + k, word 33 l + k,
// and the 32 lanes of a tile hit 32 different banks; in phase 2 the lanes address consecutive words.  The two tiles of a wave lie in
// different lane groups of an LDS access and never meet.  The settled jump words stay in registers through the scan and go into the
// state array when it is done, where `last` finds the exit: 4.2 KB of LDS per tile.
constexpr uint32_t kScanBlock = 32;                                  // slots of a block, and blocks of a tile
constexpr uint32_t kScanTiles = 8;                                   // tiles of a workgroup: two per wave
constexpr uint32_t kScanWords = kTile + kTile / kScanBlock;          // state words of a tile, padded
__device__ __forceinline__ uint32_t scan_word(uint32_t li) { return li + li / kScanBlock; }

__device__ __forceinline__ void chain_tiles_scan(uint32_t* __restrict__ jump, uint64_t t0, uint64_t r1, const FeasRef& fb,
                                                 const uint32_t* __restrict__ seg_begin, uint32_t nseg, uint2* __restrict__ xh)
{
    static_assert(kTile == 1024 && kScanBlock * kScanBlock == kTile, "the packed word holds 10-bit tile offsets; 32 blocks of 32 slots");
    __shared__ uint32_t s_st[kScanTiles][kScanWords];
    __shared__ uint64_t s_fb[kScanTiles][kTileFeasWords];
    constexpr uint32_t kDone = 1u << 10;
    constexpr uint32_t kPer = kTile / 32;                            // slots per lane
    const uint32_t l = threadIdx.x & 31, tl = threadIdx.x >> 5;      // lane of the tile, tile of the workgroup
    uint32_t* const S = s_st[tl];
    const uint64_t base = t0 + ((uint64_t)blockIdx.x * kScanTiles + tl) * kTile;       // (may lie at or behind r1: such a tile writes nothing)
    const uint64_t wave_base = uniform(t0 + ((uint64_t)blockIdx.x * kScanTiles + (tl & ~1u)) * kTile);
    const uint64_t tile_end = base + kTile;
    // ---- settling, as in the doubling kernel: a lane holds slots l + 32 r of its tile ------------------------------------------------
    uint32_t jw[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
        const uint64_t e = base + l + 32 * r;
        jw[r] = e < r1 ? jump[e] : kNone;
    }
    const uint64_t w_base = base >> 6;
    s_fb[tl][l] = w_base + l <= ((r1 - 1) >> 6) ? fb.lvl0[w_base + l] : 0;             // (kTileFeasWords = 32: a word per lane)
    static_assert(kTileFeasWords == 32, "one feasibility word per lane of the tile");
    wave_sync();
    uint32_t moved = 0;                                              // bit r: the target of slot r is not the raw one
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
        const uint32_t j = jw[r];
        if (j != kNone) {
            const uint64_t wi = ((uint64_t)j >> 6) - w_base;
            const uint64_t bits = wi < kTileFeasWords ? s_fb[tl][wi] >> (j & 63) : 0;
            const uint32_t ej = bits ? j + (uint32_t)__ffsll((long long)bits) - 1 : next_feasible(fb, j);
            moved |= (uint32_t)(ej != j) << r;
            jw[r] = ej;
        }
    }
    // the segment of the wave's first slot, once per wave that has a moved target; the lanes walk on from it only where a border falls
    // before the end of their tile
    if (__any(moved != 0)) {
        const uint32_t s_t = wave_seg_find(seg_begin, nseg, wave_base);
        const uint32_t t_next = seg_begin[s_t + 1];                  // begin of the next segment with slots (seg_begin[nseg + 1] = 2^32 - 1)
#pragma unroll
        for (uint32_t r = 0; r < kPer; ++r) {
            const uint64_t e = base + l + 32 * r;
            if ((moved >> r) & 1) {
                uint32_t lim = t_next;
                if ((uint64_t)lim < tile_end) {
                    uint32_t s = s_t;
                    while (seg_begin[s + 1] <= e) ++s;
                    lim = seg_begin[s + 1];
                }
                if (jw[r] >= lim) jw[r] = kNone;
                jump[e] = jw[r];
            }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
        const uint32_t li = l + 32 * r;
        const uint32_t j = jw[r];
        const bool inside = j != kNone && (uint64_t)j < tile_end;
        S[li + r] = (inside ? (uint32_t)(j - base) : kDone) | (li << 21);                // (scan_word(li) = li + r)
    }
    wave_sync();
    // ---- phase 1: lane l owns block l, words 33 l + k; it reads and writes no other block ---------------------------------------------
    {
        uint32_t* const B = S + l * (kScanBlock + 1);
        uint32_t v = B[kScanBlock - 1];
        for (uint32_t k = kScanBlock; k-- > 0;) {
            const uint32_t below = k ? B[k - 1] : 0;                 // (asked for before slot k is written: slot k - 1 does not wait for it)
            const uint32_t t = v & 1023u;
            if (!(v & kDone) && t / kScanBlock == l) {
                const uint32_t nx = S[scan_word(t)];
                const uint32_t hops = ((v >> 11) & 1023u) + ((nx >> 11) & 1023u) + 1;
                B[k] = (nx & 0x7FFu) | (hops << 11) | (nx & (1023u << 21));
            }
            v = below;
        }
    }
    wave_sync();
    // ---- phase 2: block b, lane l takes slot 32 b + l, word 33 b + l; an open slot lands in a block that is final -----------------------
    {
        uint32_t v = S[(kScanBlock - 1) * (kScanBlock + 1) + l];
        for (uint32_t b = kScanBlock; b-- > 0;) {
            const uint32_t below = b ? S[(b - 1) * (kScanBlock + 1) + l] : 0;          // (block b - 1 is written in its own step only)
            if (!(v & kDone)) {
                const uint32_t nx = S[scan_word(v & 1023u)];
                const uint32_t hops = ((v >> 11) & 1023u) + ((nx >> 11) & 1023u) + 1;
                S[b * (kScanBlock + 1) + l] = kDone | (hops << 11) | (nx & (1023u << 21));
            }
            wave_sync();
            v = below;
        }
    }
    // ---- the exits: the states leave the array, the settled jump words take their place -------------------------------------------------
    uint32_t st[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) st[r] = S[l + 33 * r];
    wave_sync();
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) S[l + 33 * r] = jw[r];
    wave_sync();
#pragma unroll
    for (uint32_t r = 0; r < kPer; ++r) {
        const uint64_t e = base + l + 32 * r;
        if (e < r1) xh[e] = make_uint2(S[scan_word(st[r] >> 21)], ((st[r] >> 11) & 1023u) + 1);
    }
}

template <bool kScan>
__global__ void __launch_bounds__(256) chain_tiles_kernel(uint32_t* __restrict__ jump, uint64_t t0 /* multiple of kTile */,
                                                          uint64_t r1, FeasRef fb, const uint32_t* __restrict__ seg_begin, uint32_t nseg,
                                                          uint2* __restrict__ xh)
{
    if constexpr (kScan) chain_tiles_scan(jump, t0, r1, fb, seg_begin, nseg, xh);
    else chain_tiles_doubling(jump, t0, r1, fb, seg_begin, nseg, xh);
}

// (a chain starts at the first feasible element of the query's first list)
//
// A lane that walks a heavy query pays one dependent xh[] round trip per tile while the other 63 lanes of its wave have long finished.
// Queries whose level-0 segment overlaps at least `wave_tiles` tiles (workspace option "walk_wave"; layout() lists them in `heavy`) are
// therefore walked by a wave each, the first n_heavy waves of the launch, in rounds: together with xh[cur] the wave asks for the first
// kWalkHeadSlots words of the next kWalkHeadTiles tiles, one word per lane, clipped to the segment.  A chain's exit lands a few slots
// into a following tile, so the entry's word is usually one of these heads: the wave hops exit to entry through them by cross-lane
// reads, a record per tile visited, and one latency covers up to kWalkHeadTiles + 1 tiles.  The first entry the heads do not hold opens
// the next round.  Records, record counts and match counts are those of the lane loop, in the same order.
constexpr uint32_t kWalkWaveTiles = 64;      // tiles of a level-0 segment from which a wave walks it
constexpr uint32_t kWalkHeadTiles = 4, kWalkHeadSlots = 16;
static_assert(kWalkHeadTiles * kWalkHeadSlots == 64, "one head word per lane");
// -DVLG_WALK_STATS: rounds of the heavy waves, tiles they visited, and entries that lay outside the fetched heads (each opens a round);
// search.hip prints and clears them behind every walk launch.  A diagnostic build.
#ifdef VLG_WALK_STATS
enum { WS_QUERIES = 0, WS_ROUNDS, WS_TILES, WS_MISSES, WS_COUNT };
__device__ unsigned long long g_walk_stats[WS_COUNT];
#define VLG_WALK_STAT(i, n) do { const unsigned long long n_ = (unsigned long long)(n); if ((threadIdx.x & 63) == 0 && n_) atomicAdd(&g_walk_stats[i], n_); } while (0)
#else
#define VLG_WALK_STAT(i, n) do { } while (0)
#endif
__global__ void __launch_bounds__(64) chain_walk_kernel(const SegMeta* __restrict__ sm, const QueryMeta* __restrict__ qm, uint32_t nq, FeasRef fb,
                                                        const uint2* __restrict__ xh, const uint32_t* __restrict__ rec_begin,
                                                        uint2* __restrict__ records, uint32_t* __restrict__ rec_count,
                                                        unsigned long long* __restrict__ counts, const uint32_t* __restrict__ heavy,
                                                        uint32_t n_heavy, uint32_t wave_tiles /* 2^32 - 1: no query is heavy */)
{
    if (blockIdx.x < n_heavy) {
        // ---- a wave per heavy query (its segment is not empty) -------------------------------------------------------------------
        const uint32_t lane = threadIdx.x;
        const uint32_t q = heavy[blockIdx.x];
        const uint32_t seg0 = qm[q].seg0;
        const uint32_t mbegin = sm[seg0].begin, mend = sm[seg0].end;
        const uint32_t n_tiles = rec_begin[q + 1] - rec_begin[q];    // tiles the segment overlaps: no chain visits more
        uint2* rec = records + rec_begin[q];
        uint32_t cur = uniform(next_feasible(fb, mbegin));
        if (cur >= mend) cur = kNone;
        unsigned long long n_match = 0;
        uint32_t nrec = 0;
        VLG_WALK_STAT(WS_QUERIES, 1);
        // The records wait in the lanes, the n-th since the last store in lane n, and are stored 60 or more at a time: loads and stores
        // leave one counter in issue order, so a store per hop in front of the next round's loads would be waited for with them.
        uint2 pend = make_uint2(0, 0);
        uint32_t pend_at = 0, pend_n = 0;
        while (cur != kNone && nrec < n_tiles) {                     // a round; every hop below leaves a record, so this ends
            if (pend_n > 64 - (kWalkHeadTiles + 1)) {                // (a round leaves at most kWalkHeadTiles + 1 records)
                if (lane < pend_n) rec[pend_at + lane] = pend;
                pend_at = nrec; pend_n = 0;
            }
            const uint64_t first = (uint64_t)(cur / kTile + 1) * kTile;          // first slot of the tile behind cur's
            const uint64_t hs = first + (uint64_t)(lane / kWalkHeadSlots) * kTile + lane % kWalkHeadSlots;
            uint2 head = make_uint2(kNone, 0);
            if (hs < mend) head = xh[hs];
            uint2 v = xh[cur];
            v.x = uniform(v.x); v.y = uniform(v.y);
            VLG_WALK_STAT(WS_ROUNDS, 1);
            while (nrec < n_tiles) {
                if (lane == pend_n) pend = make_uint2(cur, mbegin + (uint32_t)n_match);
                ++pend_n;
                ++nrec;
                n_match += v.y;
                cur = v.x;
                VLG_WALK_STAT(WS_TILES, 1);
                if (cur == kNone) break;
                // the entry: head word (tile i behind the round's first, slot j) if i and j are small enough.  (cur < mend: a settled
                // target is a slot of its own segment, so a head that was clipped is never asked for)
                const uint64_t i = ((uint64_t)cur - first) / kTile;
                const uint32_t j = cur % kTile;
                if (i >= kWalkHeadTiles || j >= kWalkHeadSlots) { VLG_WALK_STAT(WS_MISSES, 1); break; }
                const uint32_t src = (uint32_t)i * kWalkHeadSlots + j;
                v.x = uniform(__shfl(head.x, src)); v.y = uniform(__shfl(head.y, src));
            }
        }
        if (lane < pend_n) rec[pend_at + lane] = pend;
        if (lane == 0) { rec_count[q] = nrec; counts[q] = n_match; }
        return;
    }
    uint32_t q = (blockIdx.x - n_heavy) * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (rec_begin[q + 1] - rec_begin[q] >= wave_tiles) return;      // a heavy query: a wave above walks it
    const QueryMeta Q = qm[q];
    unsigned long long n_match = 0;
    uint32_t nrec = 0;
    if (Q.seg0 != kNone) {
        const uint32_t mbegin = sm[Q.seg0].begin, mend = sm[Q.seg0].end;
        uint2* rec = records + rec_begin[q];
        uint32_t cur = mbegin < mend ? next_feasible(fb, mbegin) : kNone;
        if (cur >= mend) cur = kNone;
        while (cur != kNone) {
            uint2 v = xh[cur];
            rec[nrec++] = make_uint2(cur, mbegin + (uint32_t)n_match);
            n_match += v.y;
            cur = v.x;
        }
    }
    rec_count[q] = nrec;
    counts[q] = n_match;
}

// A wave per record: the matches inside its tile are entry, jump(entry), jump^2(entry), ..., `cnt` of them (the hop count the tile pass
// left in xh).  The tile's jump targets are staged in LDS as tile-relative 16-bit offsets and the wave builds jump^(2^k) by doubling
// there; lane r composes the tables selected by the bits of its rank r, so every match is found by <= 10 independent LDS lookups
// instead of one lane hopping through the whole chain (380 dependent hops per tile on BASELINE config 3).
// kDirect (first positions only: workspace options "tuples" = 0, "emit_direct" = 1): the wave knows its record's query, the number of that
// query's first match inside the tile (rc.y - m.begin) and every slot, so it writes the first positions themselves,
// out_first[Q.out_first + match number] = P[phys_of(m, slot)], and adds them into the checksum as the gather pass does -- no mlist[] and
// no gather pass behind it.  It then runs after the counts went to the host and qm[].out_first came back.
template <typename pos_t, bool kDirect>
__global__ void __launch_bounds__(256) chain_emit_kernel(const uint32_t* __restrict__ rec_begin, const uint32_t* __restrict__ rec_count,
                                                         const uint2* __restrict__ records, uint32_t total_rec_slots,
                                                         const uint32_t* __restrict__ rec_query, const uint32_t* __restrict__ jump,
                                                         const uint2* __restrict__ xh, uint64_t r1 /* end of the slots that have a jump */,
                                                         uint32_t* __restrict__ mlist, const pos_t* __restrict__ P, const SegMeta* __restrict__ sm,
                                                         const QueryMeta* __restrict__ qm, pos_t* __restrict__ out_first,
                                                         unsigned long long* __restrict__ checksum)
{
    constexpr uint16_t kOut = 0xFFFFu;                               // the chain leaves the tile
    constexpr uint32_t kPer = kTile / 64;                            // slots (and ranks) per lane
    __shared__ uint16_t s_t[4][2][kTile];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t r = uniform((uint32_t)(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    // (wave-uniform; no early return: with kDirect every wave of the workgroup reaches the barriers of the checksum)
    bool live = r < total_rec_slots;
    uint32_t q = 0;
    if (live) {
        q = rec_query[r];                                    // slot r belongs to query q; used only if r - rec_begin[q] < rec_count[q]
        live = r - rec_begin[q] < rec_count[q];
    }
    unsigned long long local = 0;
    if (live) {
        const uint2 rc = records[r];
        const uint64_t tile_base = (uint64_t)(rc.x / kTile) * kTile;
        const uint32_t cnt = uniform(xh[rc.x].y);                    // chain elements inside the tile, entry included (1 .. kTile)
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const uint64_t e = tile_base + lane + 64 * i;
            const uint32_t j = e < r1 ? jump[e] : kNone;
            s_t[wv][0][lane + 64 * i] = (j != kNone && (uint64_t)j < tile_base + kTile) ? (uint16_t)(j - (uint32_t)tile_base) : kOut;
        }
        wave_sync();
        uint32_t cur[kPer];
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) cur[i] = rc.x - (uint32_t)tile_base;
        uint32_t buf = 0;
        for (uint32_t k = 0; (1u << k) < cnt; ++k) {
            const uint16_t* __restrict__ T = s_t[wv][buf];
#pragma unroll
            for (uint32_t i = 0; i < kPer; ++i) {
                const uint32_t rank = lane + 64 * i;
                if (rank < cnt && ((rank >> k) & 1)) cur[i] = T[cur[i]];     // (rank < cnt: the walk stays inside the tile)
            }
            if ((2u << k) < cnt) {                                           // jump^(2^(k+1)) for the next round
                uint16_t* __restrict__ N = s_t[wv][buf ^ 1];
#pragma unroll
                for (uint32_t i = 0; i < kPer; ++i) {
                    const uint32_t sl = lane + 64 * i;
                    const uint16_t a = T[sl];
                    N[sl] = a == kOut ? kOut : T[a];
                }
                wave_sync();
                buf ^= 1;
            }
        }
        if (kDirect) {
            const QueryMeta Q = qm[q];
            const SegMeta m = sm[Q.seg0];
            pos_t* const out = out_first + Q.out_first + (rc.y - m.begin);   // the record's first match is the query's match rc.y - m.begin
#pragma unroll
            for (uint32_t i = 0; i < kPer; ++i) {
                const uint32_t rank = lane + 64 * i;
                if (rank < cnt) {
                    const pos_t first = P[phys_of(m, (uint32_t)tile_base + cur[i])];
                    out[rank] = first;
                    local += first;
                }
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kPer; ++i) {
                const uint32_t rank = lane + 64 * i;
                if (rank < cnt) mlist[rc.y + rank] = (uint32_t)tile_base + cur[i];
            }
        }
    }
    if (kDirect) {
        // one atomic per workgroup, spread over kChecksumSlots words, as in join_gather_kernel
        __shared__ unsigned long long s_sum;
        if (threadIdx.x == 0) s_sum = 0;
        __syncthreads();
        for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
        if (lane == 0 && local) atomicAdd(&s_sum, local);
        __syncthreads();
        if (threadIdx.x == 0 && s_sum) atomicAdd(checksum + (blockIdx.x % kChecksumSlots), s_sum);
    }
}

// tuples of every match: walk the links from the level-0 element.  One thread per MATCH of the chunk (match g belongs to the query q with
// out_first[q] <= g < out_first[q + 1]; it is that query's match number g - out_first[q]) -- the kernel used to run over every slot of
// every first list and let three quarters of its lanes find out that their slot held no match.
// Results are written as wide as the positions are (ResultPiece::width); vlg_result_fetch widens them on the way to the host.
template <typename pos_t>
__global__ void __launch_bounds__(256) join_gather_kernel(const pos_t* __restrict__ P, const SegMeta* __restrict__ sm, const QueryMeta* __restrict__ qm,
                                                          const unsigned long long* __restrict__ first_of /* [nq] = qm[.].out_first, dense */, uint32_t nq,
                                                          uint64_t n_matches, const uint32_t* __restrict__ link, const uint32_t* __restrict__ mlist,
                                                          pos_t* __restrict__ out_first, pos_t* __restrict__ out_tuples, unsigned long long* __restrict__ checksum)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t run_begin = wave * kRun;
    const bool live = run_begin < n_matches;               // (no early return: every wave of the workgroup reaches the barriers below)
    const uint64_t run_end = !live ? run_begin : (run_begin + kRun < n_matches ? run_begin + kRun : n_matches);
    // the query of the run's first match: the last one that starts at or before it (queries without matches start where their successor starts)
    uint32_t q_w = 0, q_end = 0;                           // ... and the query of its last match: a lane looks its own query up between the two
    if (live) {                                            // (`live` is wave-uniform)
        const uint32_t ub = wave_kary_lower_bound<unsigned long long>(first_of, 0, nq, run_begin + 1);
        q_w = uniform(ub ? ub - 1 : 0u);
        const uint32_t ue = wave_kary_lower_bound<unsigned long long>(first_of, 0, nq, run_end);
        q_end = uniform(ue ? ue - 1 : 0u);
    }
    unsigned long long local = 0;
    for (uint64_t base = run_begin; base < run_end; base += 64) {
        const uint64_t g = base + lane;
        uint32_t q = q_w;
        if (g < run_end) {
            uint32_t hi = q_end;                                       // last query that starts at or before match g (a batch with few matches has
            while (q < hi) {                                           // thousands of queries between two of them: no walk from query to query)
                const uint32_t mid = q + ((hi - q + 1) >> 1);
                if (first_of[mid] <= g) q = mid; else hi = mid - 1;
            }
            const QueryMeta Q = qm[q];
            const SegMeta m = sm[Q.seg0];
            const uint64_t t = g - Q.out_first;
            const uint32_t el = mlist[m.begin + t];                    // logical element of level 0
            const pos_t first = P[phys_of(m, el)];
            out_first[g] = first;
            local += first;
            if (out_tuples) {                                          // null: first positions only (workspace option "tuples" = 0)
                pos_t* tp = out_tuples + Q.out_tuple + t * Q.k;
                tp[0] = first;
                uint32_t cur = Q.k > 1 ? link[el] : 0;
                uint32_t sg = m.next;
                for (uint32_t i = 1; i < Q.k; ++i) {
                    const SegMeta mi = sm[sg];
                    if (mi.dist == 0) { tp[i] = P[cur]; }              // link of a dist-1 element is a physical index
                    else { tp[i] = P[phys_of(mi, cur)]; cur = link[cur]; sg = mi.next; }
                }
            }
        }
        const uint32_t last = (uint32_t)((run_end - base < 64 ? run_end - base : 64) - 1);
        q_w = __shfl(q, (int)last);                                    // the next step's matches come behind this step's last one
    }
    // one atomic per workgroup, spread over kChecksumSlots words (a single word takes ~90 atomics per microsecond; there are
    // 10^5..10^6 waves here); the host adds the slots up
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
    if (lane == 0 && local) atomicAdd(&s_sum, local);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(checksum + (blockIdx.x % kChecksumSlots), s_sum);
}


}  // namespace
