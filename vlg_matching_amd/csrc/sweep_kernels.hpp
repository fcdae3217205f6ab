// The locate family, written once over the LF-walk policy (lf_walk.hpp): the sorted sweep's rounds (sweep_first_kernel,
// sweep_step_kernel) and the refilling-lane walk that locates in place and finishes the sweep's stragglers (locate_kernel).
// bind_sweep (at the end) fills the sweep's three launches for one <Walk, Sampling, pos_t, kWide>; which one an index gets is decided
// through shape_dispatch.hpp by its launcher -- launch_locate_sweep (kernels.hip: ByteWalk) or launch_int_locate_sweep (int_index.hpp:
// IntWalk, kWide = false, pos_t = uint32_t, front = nullptr) -- and run_locate_sweep (kernels.hip) drives both.
#pragma once
#include "lf_walk.hpp"
#include "kernels.hpp"
#include "shape_dispatch.hpp"

namespace vlg {

// Statistics counters: a wave-level sum, then ONE atomic per workgroup and counter -- a single word takes ~90 atomics per
// microsecond, so one per wave (16 k waves a launch) would cost every launch of the sweep a fifth of a millisecond.
template <int N>
__device__ __forceinline__ void block_add(unsigned long long (&v)[N], unsigned long long* const (&dst)[N])
{
    __shared__ unsigned long long s_acc[N];
    if (threadIdx.x < N) s_acc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        unsigned long long x = v[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s_acc[k], x);
    }
    __syncthreads();
    if (threadIdx.x < N && s_acc[threadIdx.x] && dst[threadIdx.x]) atomicAdd(dst[threadIdx.x], s_acc[threadIdx.x]);
}

// rec[slot] of a trail-sharing sweep (sweep_element): a position (high bits 0), or delta << kShift | slot of the element it follows; ~0
// while the element is still walking.  The record of an element that stands, `delta` steps into its walk, on the index where element
// `owner` started:
template <uint32_t kShift>
__device__ __forceinline__ uint64_t follow_owner(const uint64_t* rec, uint32_t owner, uint64_t delta)
{
    const uint64_t ro = rec[owner];
    if (ro == ~0ull) return (delta << kShift) | owner;                        // still walking: follow it
    if ((ro >> kShift) == 0) return ro + delta;                               // its position is known
    return ro + (delta << kShift);                                            // it follows someone itself: follow that one
}

// A wave's slice [next, end) of `total` elements, dealt to its lanes as they ask: every lane that needs an element gets the next ones
// of the slice in lane order (ballot + prefix popcount), take(candidate) does with it what the kernel wants (the candidate may lie
// behind the slice's end).
struct WaveSlice {
    uint32_t lane;
    uint64_t next, end;                                    // (wave-uniform)
    __device__ __forceinline__ WaveSlice(uint64_t total, uint32_t per_wave)
    {
        lane = threadIdx.x & 63;
        const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        next = wave * per_wave;
        end = next + per_wave < total ? next + per_wave : total;
    }
    template <class Take>
    __device__ __forceinline__ void refill(bool need, const Take& take)
    {
        const unsigned long long m = __ballot(need);
        if (m) {
            const uint32_t before = __popcll(m & ((1ull << lane) - 1ull));
            if (need) take(next + before);
            next += __popcll(m);
        }
    }
};

// =============================================================================================
// K3: csa[i] = LF iteration to the next sampled SA index (include/sdsl/csa_wt.hpp:335-348,
//     LF = C[c] + inverse_select(i): suffix_array_helper.hpp:336-349, wt_pc.hpp:385-402).
//
// io[t] holds the SA index on entry and the text position on exit (in place).
// Work is dealt to lanes, not to waves: a wave owns a contiguous slice of io[] and every lane that
// finishes an occurrence immediately pulls the next one of the slice (WaveSlice), so
// all 64 lanes issue one 32-byte super-block read per iteration whatever the (geometric) number
// of LF steps and whatever the code lengths.
// =============================================================================================
// kTail: the same walk for the stragglers of the sorted sweep (K3s below): the elements are val[] = slot << kShift | SA index, they
// have walked `step` steps already, positions go to out[slot] -- or to rec[slot0 + slot] when LF steps are shared, and then a walk
// also ends on the first index that is an element of the batch itself (sweep_element explains the records and `member`).
// How long an element still walks is geometrically distributed (one SA index in `dens` is sampled), so a lane that kept one element
// to its end would idle most of the time behind the longest walk of its wave; here a lane that has finished takes the next element.
// kWide: SA indices need 33 bits and the samples are 64-bit words (n > 2^32, or VLG_FORCE_POS64); the positions written may still be
// 32-bit (pos_t) when the text has at most 2^32 characters -- only the tail mode can split the two, the in-place mode keeps the SA
// index in io[] itself.
template <class Walk, class Sampling, typename pos_t, bool kTail = false, bool kWide = (sizeof(pos_t) == 8)>
__global__ void __launch_bounds__(256) locate_kernel(typename Walk::View iv, pos_t* __restrict__ io, uint64_t total, uint32_t per_wave,
                                                     unsigned long long* __restrict__ stats /* [2]: lf steps, levels */,
                                                     const uint64_t* __restrict__ val = nullptr, uint32_t step = 0,
                                                     uint64_t* __restrict__ rec = nullptr, uint64_t slot0 = 0,
                                                     const Block* __restrict__ member = nullptr)
{
    static_assert(kTail || kWide == (sizeof(pos_t) == 8), "in place, io[] holds the SA index: its width is the index width");
    constexpr uint32_t kShift = kWide ? 33 : 32;
    constexpr uint64_t kPosMask = (1ull << kShift) - 1;
    __shared__ typename Walk::Lds s;
    Walk::stage(s, iv);
    const Walk walk{iv, s};
    WaveSlice slice(total, per_wave);
    const Sampling sampling(iv);

    uint64_t t = 0;          // slot being worked on
    uint64_t i = 0;          // SA index at the root, node-relative index below it
    typename Walk::Cursor k;
    uint32_t off = 0;
    bool active = false, need = true;
    uint32_t n_lf = 0, n_lv = 0;
    for (;;) {
        slice.refill(need, [&](uint64_t cand) {
            if (cand < slice.end) {
                if (kTail) { const uint64_t e = val[cand]; t = e >> kShift; i = e & kPosMask; off = step; }
                else { t = cand; i = io[cand]; off = 0; }
                k = typename Walk::Cursor();
                active = true;
            }
            else active = false;
            need = false;
        });
        if (!__any(active)) break;
        if (active) {
            uint64_t sv = 0;
            uint32_t owner = 0, c;
            if (k.at_root() && sampling.probe(i, sv)) {    // csa_sampling_strategy.hpp:102-111 / :185-194
                uint64_t r = sv + off;
                if (r >= walk.n()) r -= walk.n();          // csa_wt.hpp:343-347
                if (kTail && rec) rec[slot0 + t] = r;
                else io[t] = (pos_t)r;
                need = true;
                active = false;
            } else if (kTail && member && k.at_root() && off != 0 && member_probe(member, i, owner)) {
                // this index is where element `owner` started: the rest of the walk is that element's (sweep_element)
                rec[slot0 + t] = follow_owner<kShift>(rec, owner, off);
                need = true;
                active = false;
            } else if (walk.degenerate()) {                // only the sentinel exists
                i = 0; ++off;
            } else if (walk.level(k, i, c, n_lv)) {
                ++off;
                ++n_lf;
            }
        }
    }
    if (stats) {
        unsigned long long v[2] = {n_lf, n_lv};
        unsigned long long* const dst[2] = {&stats[0], &stats[1]};
        block_add<2>(v, dst);
    }
}

// =============================================================================================
// K3s: locate as a synchronous SORTED SWEEP (n <= 2^32).
//
// All occurrences advance one LF step per round.  The round's elements are kept in ascending SA-index order:
// LF restricted to one symbol is monotone (LF(i) = C[c] + rank_c(i)), so after a round a STABLE partition of the
// elements by the symbol they read restores the order -- no comparison sort.  With ascending positions the 64
// lanes of a wave read the same or neighbouring super-blocks at every level of the tree (coalesced loads instead
// of 64 unrelated 64-byte requests), which is what lifts the kernel off the random-access wall of HBM
// (tools/k1_bench.py: ~50 G random ranks/s vs ~280 G sorted ranks/s).
// An element leaves the sweep when it reaches a sampled SA index (csa_sampling_strategy.hpp:102-111).
// val = slot << 32 | position;  key = comp of the symbol read, or sigma for "finished".
// (val = slot << kShift | position in general: kernels.hip, sweep_init_kernel.)
// =============================================================================================

// The lists that hold the elements [base, end) of a workgroup's turn, staged in LDS: looking an element's list up (whose interval it
// belongs to, where that starts) is a chain of dependent reads in front of everything else the element does, and the next element's
// chain starts where this one's ended -- out of LDS it costs tens of cycles instead of L2 round trips.  A turn whose elements spread
// over more than kListStage lists (lists of a few elements each) walks the global arrays as before.  VLG_STAGE_LISTS=0: never staged;
// a walk policy may also decline (Walk::kStageLists) when the 4.1 KiB cost it a resident workgroup.
#ifndef VLG_STAGE_LISTS
#define VLG_STAGE_LISTS 1
#endif
constexpr bool kStageLists = VLG_STAGE_LISTS != 0;
static_assert(VLG_STAGE_LISTS == 0 || VLG_STAGE_LISTS == 1, "VLG_STAGE_LISTS: 0 or 1");
constexpr uint32_t kListStage = 256;
struct ListStage { uint64_t off[kListStage + 1]; uint64_t l[kListStage]; };
__device__ __forceinline__ bool stage_lists(ListStage& ls, const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ l, uint64_t n_pat,
                                            uint64_t first, uint64_t end)
{
    for (uint32_t j = threadIdx.x; j <= kListStage; j += blockDim.x) {
        const uint64_t p = first + j;
        ls.off[j] = out_off[p < n_pat ? p : n_pat];
        if (j < kListStage) ls.l[j] = l[p < n_pat ? p : n_pat - 1];
    }
    __syncthreads();
    return ls.off[kListStage] >= end;                      // (the same word in every thread: the branch on it is uniform)
}

// Where a round's elements go.  ArraySink: every element keeps its place e in val / key, a finished one gets key = sigma and is
// carried through the round's partition into its last bucket (the workspace option "sweep_compact" = 0).
struct ArraySink {
    uint64_t* __restrict__ val;
    uint16_t* __restrict__ key;
    uint16_t sigma;
    __device__ __forceinline__ void emit(uint64_t e, uint64_t word, uint32_t c) const { val[e] = word; key[e] = (uint16_t)c; }
    __device__ __forceinline__ void finish(uint64_t e) const { key[e] = sigma; }
};

// ---------------------------------------------------------------------------------------------
// Compaction (round 0, sweep_first_kernel<.., kCompact>): a finished element never reaches the partition -- six in ten of C3's
// occurrences end in round 0.  A workgroup takes its elements in TURNS of kSweepChunk consecutive
// ones, row by row (kSweepRows rows of 256); what goes on to another round stays with the thread that walked it, the word in
// registers and the key in LDS (TurnRegs: the walks exchange nothing), and when the turn's walks are done its survivors are written to
//     val / key [survivors of all earlier turns + stable rank inside the turn),
// in the order of the elements themselves (row, then thread): the survivors stay in ascending SA-index order, the round's outcome
// does not depend on which workgroup ran which turn, and the partition sorts `alive - done` elements instead of `alive`.
// The survivors of all earlier turns come from a decoupled look-back over one 64-bit status word per turn, tag << 62 | count:
// tag 1 = the turn's own survivors (stored when its walks are done), tag 2 = the survivors up to and including it (stored when its
// look-back ends).  The words are written and read with relaxed agent-scope atomics -- the word is its own flag, nothing else is
// handed from workgroup to workgroup inside the launch -- and one wave looks back, 64 predecessors per load.
// Turn numbers are drawn from a counter, not taken from blockIdx: the grid is capped and not fully resident, and a workgroup must
// never wait for a turn that no running workgroup has drawn.  A workgroup that holds turn k is running, so every turn before k has
// been drawn by a workgroup that is running or done, and each stores its tag-1 word before it waits for anything: the look-back
// always ends.  Its spins are bounded all the same (kTurnSpins polls per window of 64 turns, all its waits together): on give-up the workgroup raises the word beside
// n_done, writes nothing further and returns; the driver reads that word with `done`.
// In place: round 0 reads no words (an element's word follows from its place), so the survivors go to the front of the arrays that
// the round would have filled anyway; the chunk_list scratch lies in the other buffer.
// The control block (driver: cleared before every launch): ctl[kSweepDone] = n_done, [kSweepStalled], [kSweepTicket],
// [kSweepStatus + turn].
// Why registers: the kernels live on their waves (round 0 of C3: 45 VGPRs, 14.4 KiB of LDS, eight waves per SIMD).  An LDS stage of the
// turn (10 B per element, 20.5 KB) left four workgroups per CU where there were eight -- DESIGN.md section 9.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kNoKey = 0xFFFF;                        // (keys are symbols < sigma < 0xFFFF: run_locate_sweep)
constexpr uint32_t kSweepRows = kSweepChunk / 256;
constexpr uint32_t kTurnSpins = 1u << 21;
// A thread's elements of one turn: row r is element r * 256 + threadIdx.x of the turn.  The row index is a loop counter at run time
// (the walks are not unrolled), so a row is written by selects over all rows: the arrays stay registers.
// kHigh: the high halves of the words are kept too (33-bit indices); without them the word is slot << 32 | low and the slot follows
// from the element's place.
struct TurnShared {
    uint16_t key[kSweepChunk];                             // the turn's keys, each written and read by its own thread; kNoKey: finished, or behind the end
    uint32_t cnt[kSweepRows * 4];                          // survivors per (row, wave)
    uint64_t base;
    uint32_t turn, stalled;
};
template <bool kHigh>
struct TurnRegs {
    TurnShared& st;
    uint32_t low[kSweepRows];
    uint32_t high[kHigh ? kSweepRows : 1];
    __device__ __forceinline__ void emit(uint64_t row, uint64_t word, uint32_t c)
    {
#pragma unroll
        for (uint32_t r = 0; r < kSweepRows; ++r) {
            low[r] = row == r ? (uint32_t)word : low[r];
            if (kHigh) high[r] = row == r ? (uint32_t)(word >> 32) : high[r];
        }
        st.key[row * 256 + threadIdx.x] = (uint16_t)c;
    }
    __device__ __forceinline__ void finish(uint64_t row) { st.key[row * 256 + threadIdx.x] = (uint16_t)kNoKey; }
    __device__ __forceinline__ uint32_t key_of(uint32_t r) const { return st.key[r * 256 + threadIdx.x]; }
};
using gu64 = __attribute__((address_space(1))) unsigned long long;
__device__ __forceinline__ void status_store(unsigned long long* p, unsigned long long x)
{
    __hip_atomic_store((gu64*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long status_load(unsigned long long* p)
{
    return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the next turn of this workgroup
__device__ __forceinline__ uint32_t draw_turn(TurnShared& st, unsigned long long* ctl)
{
    __syncthreads();                                       // (everyone has read what the last turn left in `st`)
    if (threadIdx.x == 0) st.turn = (uint32_t)atomicAdd(&ctl[kSweepTicket], 1ull);
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(st.turn);       // (one word for all: scalar, like everything the turn derives from it)
}

// The survivors of `turn` to their places; slot_word: the high half's worth of the word of row r where the registers do not hold it
// (kHigh = false: slot << 32 of the turn's first element + this thread's).  false: the look-back gave up (nothing was written; the
// whole workgroup returns).
template <bool kHigh>
__device__ __forceinline__ bool commit_turn(const TurnRegs<kHigh>& regs, TurnShared& st, unsigned long long* ctl, uint32_t turn, uint64_t first_slot,
                                            uint64_t* __restrict__ val, uint16_t* __restrict__ key)
{
    constexpr unsigned long long kValue = (1ull << 62) - 1;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t r = 0; r < kSweepRows; ++r) {
        const unsigned long long m = __ballot(regs.key_of(r) != kNoKey);
        if (lane == 0) st.cnt[r * 4 + wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    // every wave scans the counts for itself: lane (row, wave) ends up with the survivors in front of that row of that wave
    const uint32_t mine = lane < kSweepRows * 4 ? st.cnt[lane] : 0u;
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    const uint32_t total = __shfl(incl, 63);
    const uint32_t excl = incl - mine;
    if (wave == 0) {
        unsigned long long* status = ctl + kSweepStatus;
        if (lane == 0) status_store(&status[turn], ((turn ? 1ull : 2ull) << 62) | total);
        unsigned long long before = 0;
        bool stalled = false;
        if (turn) {
            long long hi = (long long)turn - 1;                                  // the nearest turn not yet counted
            uint32_t spins = 0;
            for (;;) {
                const long long j = hi - (long long)lane;
                const unsigned long long w = j >= 0 ? status_load(&status[j]) : (2ull << 62);      // (in front of turn 0: nothing)
                const uint32_t tag = (uint32_t)(w >> 62);
                const unsigned long long ready = __ballot(tag != 0), prefixed = __ballot(tag == 2);
                unsigned long long need = ~0ull;                                 // the turns of this window the sum cannot do without
                if (prefixed) {                                                  // the nearest turn that knows its prefix ends the look-back,
                    const uint32_t f = (uint32_t)__ffsll((long long)prefixed) - 1;      // once every turn between it and this one has its count
                    need = f == 63 ? ~0ull : (1ull << (f + 1)) - 1;
                    if ((ready & need) == need) {
                        unsigned long long x = lane <= f ? (w & kValue) : 0ull;
                        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
                        before += x;
                        break;
                    }
                } else if (ready == ~0ull) {                                     // 64 turns with their own counts only: take them, look further back
                    unsigned long long x = w & kValue;
                    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
                    before += x;
                    hi -= 64;
                    spins = 0;
                    continue;
                }
                // Some of them are still walking.  Turns end roughly in the order they were drawn in, so the nearest of the missing
                // ones is the last to come: the wave waits on that one word alone -- one 8-byte request per poll instead of 64 from
                // each of a thousand waiting workgroups, beside the walks' own loads -- and then reads the window again.
                const long long late = hi - (long long)((uint32_t)__ffsll((long long)(~ready & need)) - 1);
                // (`spins` counts on from wait to wait and starts again only when the window moves: kTurnSpins bounds a window's waits together)
                while ((status_load(&status[late]) >> 62) == 0) {
                    if (++spins > kTurnSpins) { stalled = true; break; }
                    __builtin_amdgcn_s_sleep(16);
                }
                if (stalled) break;
            }
            if (lane == 0) {
                if (stalled) status_store(&ctl[kSweepStalled], 1ull);
                else status_store(&status[turn], (2ull << 62) | (before + total));
            }
        }
        if (lane == 0) { st.base = before; st.stalled = stalled ? 1u : 0u; }
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(st.stalled)) return false;
    const uint64_t base = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(st.base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)st.base);
#pragma unroll
    for (uint32_t r = 0; r < kSweepRows; ++r) {
        const uint32_t k = regs.key_of(r);
        const unsigned long long m = __ballot(k != kNoKey);
        const uint32_t pre = __shfl(excl, r * 4 + wave);
        if (k != kNoKey) {
            const uint64_t to = base + pre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            const uint64_t high = kHigh ? (uint64_t)regs.high[kHigh ? r : 0] : first_slot + r * 256 + threadIdx.x;
            val[to] = (high << 32) | regs.low[r];
            key[to] = (uint16_t)k;
        }
        __builtin_amdgcn_sched_barrier(0);                 // (row by row: the rows' addresses side by side cost the walks their registers)
    }
    return true;
}

// kTrail: LF steps are shared inside the batch.  An LF walk from SA index i visits the indices of the text positions SA[i] - 1,
// SA[i] - 2, ...; when it stands on an index that is ITSELF an element of the batch (the start of another occurrence's walk: text
// position SA[i] - k is an occurrence too) the rest of the walk is that element's walk, so it stops there and records
// (that element, k): csa[i] = csa[LF^k(i)] + k (csa_wt.hpp:335-348 applied to a value another lane computes).  Which indices are
// elements is known before the sweep starts -- the batch's lists are SA intervals -- and kept as a rank-enabled bit-vector over
// the SA indices in the usual 256-bit super-blocks (`member`, member_build_kernel): one 32-byte read says whether index i is an
// element AND which one (its slot = the number of member indices before it: the lists lie in SA order in the slot space).
// This replaces the table of round 2 / 3 (8 bytes per text position, written and read at random by every step, told apart by
// generation stamps) with n / 7 bytes that are only read; a walk also stops wherever it can, not only where another one has passed
// EARLIER, so every non-member index is visited by at most one walk.
// rec[slot]: follow_owner above.  slot0 = first slot of the sweep.
// one element of one round: v64 = its word (slot << kShift | SA index), e = its place in val / key
// kAhead (round 0): the index an element steps ONTO is looked up at once -- six in ten elements of a dense batch stand next to
// another occurrence in the text -- so that they leave the sweep before its largest partition instead of after it; `probed` tells
// round 1 that its elements have been looked up already.
template <class Walk, class Sampling, typename pos_t, bool kTrail, bool kWide, bool kFirst = false, bool kAhead = false, class Sink = ArraySink>
__device__ __forceinline__ void sweep_element(const Walk& walk, const Sampling& sampling, uint64_t e, uint64_t v64,
                                              Sink& sink, uint32_t step, pos_t* __restrict__ out,
                                              const Block* __restrict__ member, uint64_t* __restrict__ rec, uint64_t slot0,
                                              uint32_t& n_lv, uint32_t& n_lf, uint32_t& n_fin, bool probed = false, uint8_t* __restrict__ front = nullptr)
{
    constexpr uint32_t kShift = kWide ? 33 : 32;
    constexpr uint64_t kPosMask = (1ull << kShift) - 1;
    uint64_t i = v64 & kPosMask;
    uint8_t in_front = 0xFF;                             // (kFirst: the symbol in front of an element that stops on its first step)
    uint64_t sv = 0;
    uint32_t owner = 0;
    if (sampling.probe(i, sv)) {
        uint64_t r = sv + step;
        if (r >= walk.n()) r -= walk.n();                // csa_wt.hpp:343-347
        if (kTrail) rec[slot0 + (v64 >> kShift)] = r;
        else out[v64 >> kShift] = (pos_t)r;
        sink.finish(e);
        ++n_fin;
    } else if (kTrail && !kFirst && !probed && member_probe(member, i, owner)) {
        // (round 0: every element stands on its own index.)  Index i is where element `owner` started: same text trail, `step`
        // positions further left
        rec[slot0 + (v64 >> kShift)] = follow_owner<kShift>(rec, owner, step);
        sink.finish(e);
        ++n_fin;
    } else {
        if (kTrail && kFirst) rec[slot0 + (v64 >> kShift)] = ~0ull;               // still walking (no pass clears the records beforehand)
        uint32_t c;
        const uint64_t j = walk.lf(i, c, n_lv);
        ++n_lf;
        if (kTrail && kAhead && member_probe(member, j, owner)) {
            // (the owner is in its own round 0 right now: its record reads "still walking" or is not written yet -- either way this
            // element follows it)
            rec[slot0 + (v64 >> kShift)] = ((uint64_t)(step + 1) << kShift) | owner;
            sink.finish(e);
            ++n_fin;
            in_front = (uint8_t)c;
        } else {
            sink.emit(e, (v64 & ~kPosMask) | j, c);
        }
    }
    if (kTrail && kFirst && front) front[slot0 + (v64 >> kShift)] = in_front;
}

#ifndef VLG_SWEEP_PAIRS
#define VLG_SWEEP_PAIRS 1
#endif
constexpr bool kSweepPairs = VLG_SWEEP_PAIRS != 0;
static_assert(VLG_SWEEP_PAIRS == 0 || VLG_SWEEP_PAIRS == 1, "VLG_SWEEP_PAIRS: 0 or 1");
// The later rounds do not compact (measured on C3, DESIGN.md section 9: the turns cost these kernels 1.5 ms per batch and saved their
// partitions 0.85 ms): every element keeps its place, and a finished one is carried through the round's partition.
template <class Walk, class Sampling, typename pos_t, bool kTrail, bool kWide>
__global__ void __launch_bounds__(256) sweep_step_kernel(typename Walk::View iv, uint64_t* __restrict__ val, uint16_t* __restrict__ key, uint64_t count,
                                                         uint32_t step, pos_t* __restrict__ out,
                                                         unsigned long long* __restrict__ stats /* lf, levels */,
                                                         unsigned long long* __restrict__ n_done, const Block* __restrict__ member,
                                                         uint64_t* __restrict__ rec, uint64_t slot0, bool probed)
{
    __shared__ typename Walk::Lds s;
    Walk::stage(s, iv);
    const Walk walk{iv, s};
    const Sampling sampling(iv);
    uint32_t n_lv = 0, n_lf = 0, n_fin = 0;
    ArraySink sink{val, key, (uint16_t)walk.sigma()};
    // (pairs of elements as in round 0 -- sweep_first_pair -- were measured here too, on C4: nothing; the later rounds' elements are sparse)
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (uint64_t)gridDim.x * blockDim.x)
        sweep_element<Walk, Sampling, pos_t, kTrail, kWide>(walk, sampling, e, val[e], sink, step, out, member, rec, slot0, n_lv, n_lf, n_fin, probed);
    unsigned long long v[3] = {n_lf, n_lv, n_fin};
    unsigned long long* const dst[3] = {&stats[0], &stats[1], n_done};
    block_add<3>(v, dst);
}

// Two elements of round 0 side by side (plain bit-vectors): every tree level and the look-ahead probe of both are loaded before either
// is used, so a lane has two dependent chains in flight instead of one (the kernel runs at full occupancy on 46 registers and waits
// ~1 us per wave-wide dependent load: more waves cannot come, more loads per wave can).  Same outcome as two sweep_element calls.
template <typename pos_t, bool kTrail, bool kWide, bool kAhead, class Sampling, class Sink>
__device__ __forceinline__ void sweep_first_pair(const IndexView& iv, const WalkLds<PlainBV>& s, const Sampling& sampling, bool onA, uint64_t eA, uint64_t wA,
                                                 bool onB, uint64_t eB, uint64_t wB, Sink& sink,
                                                 pos_t* __restrict__ out, const Block* __restrict__ member, uint64_t* __restrict__ rec, uint64_t slot0,
                                                 uint32_t& n_lv, uint32_t& n_lf, uint32_t& n_fin, uint8_t* __restrict__ front)
{
    constexpr uint32_t kShift = kWide ? 33 : 32;
    constexpr uint64_t kPosMask = (1ull << kShift) - 1;
    using walk_t = typename std::conditional<kWide, uint64_t, uint32_t>::type;
    const uint64_t iA = wA & kPosMask, iB = wB & kPosMask;
    const bool hadA = onA, hadB = onB;
    uint64_t sv = 0;
    if (onA && sampling.probe(iA, sv)) {                                     // csa_wt.hpp:343-347 (round 0: no steps yet)
        if (kTrail) rec[slot0 + (wA >> kShift)] = sv; else out[wA >> kShift] = (pos_t)sv;
        sink.finish(eA); ++n_fin; onA = false;
    }
    if (onB && sampling.probe(iB, sv)) {
        if (kTrail) rec[slot0 + (wB >> kShift)] = sv; else out[wB >> kShift] = (pos_t)sv;
        sink.finish(eB); ++n_fin; onB = false;
    }
    if (kTrail) {                                                            // still walking (no pass clears the records beforehand)
        if (onA) rec[slot0 + (wA >> kShift)] = ~0ull;
        if (onB) rec[slot0 + (wB >> kShift)] = ~0ull;
    }
    // inverse_select of both (wt_pc.hpp:385-402), level by level
    uint32_t vA = 0, vB = 0, cA = 0, cB = 0;
    walk_t pA = (walk_t)iA, pB = (walk_t)iB;
    bool a = onA, b = onB;
    while (a || b) {
        const DNode ndA = s.nodes[vA], ndB = s.nodes[vB];
        uint32_t blkA, offA, blkB, offB;
        split224((uint64_t)pA, blkA, offA);
        split224((uint64_t)pB, blkB, offB);
        BlockRegs rA, rB;
        if (a) rA = load_block(iv.blocks, ndA.base + blkA);
        if (b) rB = load_block(iv.blocks, ndB.base + blkB);
        if (a) {
            uint32_t bit;
            const walk_t r1 = (walk_t)block_rank_bit(rA, offA, bit);
            ++n_lv;
            pA = bit ? r1 : pA - r1;
            const uint32_t ch = bit ? ndA.child[1] : ndA.child[0];
            if (ch & kLeafFlag) { cA = ch & ~kLeafFlag; a = false; } else vA = ch;
        }
        if (b) {
            uint32_t bit;
            const walk_t r1 = (walk_t)block_rank_bit(rB, offB, bit);
            ++n_lv;
            pB = bit ? r1 : pB - r1;
            const uint32_t ch = bit ? ndB.child[1] : ndB.child[0];
            if (ch & kLeafFlag) { cB = ch & ~kLeafFlag; b = false; } else vB = ch;
        }
    }
    const uint64_t jA = s.C[cA] + (uint64_t)pA, jB = s.C[cB] + (uint64_t)pB;  // LF: suffix_array_helper.hpp:341-348
    n_lf += (onA ? 1u : 0u) + (onB ? 1u : 0u);
    bool stopA = false, stopB = false;
    uint32_t ownA = 0, ownB = 0;
    if (kTrail && kAhead) {                                                  // the look-ahead probes of both, their blocks in flight together
        uint32_t blkA, offA, blkB, offB, bit;
        split224(jA, blkA, offA);
        split224(jB, blkB, offB);
        BlockRegs rA, rB;
        if (onA) rA = load_block(member, blkA);
        if (onB) rB = load_block(member, blkB);
        if (onA) { ownA = block_rank_bit(rA, offA, bit); stopA = bit != 0; }
        if (onB) { ownB = block_rank_bit(rB, offB, bit); stopB = bit != 0; }
    }
    if (onA) {
        if (stopA) { rec[slot0 + (wA >> kShift)] = (1ull << kShift) | ownA; sink.finish(eA); ++n_fin; }
        else sink.emit(eA, (wA & ~kPosMask) | jA, cA);
    }
    if (onB) {
        if (stopB) { rec[slot0 + (wB >> kShift)] = (1ull << kShift) | ownB; sink.finish(eB); ++n_fin; }
        else sink.emit(eB, (wB & ~kPosMask) | jB, cB);
    }
    if (kTrail && front) {                                                   // the symbol in front of an element that stopped on its first step
        if (hadA) front[slot0 + (wA >> kShift)] = (onA && stopA) ? (uint8_t)cA : (uint8_t)0xFF;
        if (hadB) front[slot0 + (wB >> kShift)] = (onB && stopB) ? (uint8_t)cB : (uint8_t)0xFF;
    }
}

// Round 0 without the pass that would write the elements' words first and the read that would fetch them again: an element's word
// follows from its place -- slot t - t0, SA index l[list] + (t - first slot of the list) -- so a workgroup looks its list up once per
// 2048 consecutive elements (as sweep_init_kernel does) and walks them at once.
// The pairs are the byte tree's with plain bit-vectors (Walk::kPlainTree); every other walk takes its elements one by one.
// kCompact: the turns are drawn from the round's counter and their survivors go to the front of val / key (commit_turn; round 0
// reads no words, so nothing is overwritten that anyone needs).
template <class Walk, class Sampling, typename pos_t, bool kTrail, bool kWide, bool kAhead, bool kCompact>
__global__ void __launch_bounds__(256) sweep_first_kernel(typename Walk::View iv, const uint64_t* __restrict__ l, const uint64_t* __restrict__ out_off, uint64_t n_pat,
                                                          uint64_t t0, uint64_t total, uint64_t* __restrict__ val, uint16_t* __restrict__ key,
                                                          pos_t* __restrict__ out, unsigned long long* __restrict__ stats,
                                                          unsigned long long* __restrict__ n_done, const Block* __restrict__ member,
                                                          uint64_t* __restrict__ rec, const uint32_t* __restrict__ chunk_list, uint8_t* __restrict__ front)
{
    constexpr bool kStage = kStageLists && Walk::kStageLists;
    __shared__ typename Walk::Lds s;
    __shared__ ListStage s_lists;                                                // (takes no LDS where it is never staged)
    Walk::stage(s, iv);
    const Walk walk{iv, s};
    const Sampling sampling(iv);
    constexpr uint32_t kShift = kWide ? 33 : 32;
    constexpr uint32_t kPer = kSweepRows;
    uint32_t n_lv = 0, n_lf = 0, n_fin = 0;
    // one turn: the elements [base, base + kSweepChunk) through `sink`, which knows element t by place(t, its row in the turn)
    auto take_turn = [&](uint64_t base, auto& sink, auto place) {
        uint64_t p = chunk_list[(base - t0) / kSweepChunk];                      // the list of the chunk's first element (sweep_chunk_lists_kernel)
        const uint64_t end = base + 256 * kPer < total ? base + 256 * kPer : total;
        const bool staged = kStage && stage_lists(s_lists, out_off, l, n_pat, p, end);
        uint32_t q = 0;
        auto word_of = [&](uint64_t t) -> uint64_t {                            // slot << kShift | SA index of element t (t ascends from call to call)
            uint64_t sai;
            if (staged) {
                while (s_lists.off[q + 1] <= t) ++q;
                sai = s_lists.l[q] + (t - s_lists.off[q]);
            } else {
                while (out_off[p + 1] <= t) ++p;
                sai = l[p] + (t - out_off[p]);
            }
            return ((t - t0) << kShift) | sai;
        };
        // (measured, round 4: C4 -- 33-bit indices, a deeper tree -- locate 98 -> 93 ms; C3 16.9 -> 17.4 ms: there the kernel has no issue slots
        //  to spare and loses a wave per SIMD to the registers: pairs for wide indices only)
        if constexpr (Walk::kPlainTree && kSweepPairs && kWide) {
            static_assert(kPer % 2 == 0, "VLG_SWEEP_CHUNK: elements are taken in pairs of rows");
#pragma unroll 1
            for (uint32_t i = 0; i < kPer; i += 2) {
                const uint64_t tA = base + i * 256 + threadIdx.x, tB = tA + 256;
                const bool onA = tA < total, onB = tB < total;
                const uint64_t wA = onA ? word_of(tA) : 0, wB = onB ? word_of(tB) : 0;
                if (kCompact) { if (!onA) sink.finish(place(tA, i)); if (!onB) sink.finish(place(tB, i + 1)); }
                sweep_first_pair<pos_t, kTrail, kWide, kAhead>(iv, s, sampling, onA, place(tA, i), wA, onB, place(tB, i + 1), wB, sink, out, member, rec, t0, n_lv, n_lf, n_fin, front);
            }
        } else {
#pragma unroll 1
            for (uint32_t i = 0; i < kPer; ++i) {
                const uint64_t t = base + i * 256 + threadIdx.x;
                if (t < total)
                    sweep_element<Walk, Sampling, pos_t, kTrail, kWide, true, kAhead>(walk, sampling, place(t, i), word_of(t), sink, 0u, out, member, rec, t0, n_lv, n_lf, n_fin, false, front);
                else if (kCompact) sink.finish(place(t, i));
            }
        }
    };
    if constexpr (kCompact) {
        __shared__ TurnShared st;
        TurnRegs<kWide> regs{st, {}, {}};                                                  // (32-bit indices: slot << 32 | index, and the slot is the element's place)
        const uint64_t turns = (total - t0 + kSweepChunk - 1) / kSweepChunk;
        for (;;) {
            const uint32_t turn = draw_turn(st, n_done);                         // (and the lists staged for the previous turn have been read)
            if (turn >= turns) break;
            take_turn(t0 + (uint64_t)turn * kSweepChunk, regs, [](uint64_t, uint32_t row) -> uint64_t { return row; });
            if (!commit_turn(regs, st, n_done, turn, (uint64_t)turn * kSweepChunk, val, key)) return;
        }
    } else {
        ArraySink sink{val, key, (uint16_t)walk.sigma()};
        for (uint64_t base = t0 + (uint64_t)blockIdx.x * kSweepChunk; base < total; base += (uint64_t)gridDim.x * kSweepChunk) {
            __syncthreads();                                                     // (the lists staged for the previous turn have been read)
            take_turn(base, sink, [t0](uint64_t t, uint32_t) -> uint64_t { return t - t0; });
        }
    }
    unsigned long long v[3] = {n_lf, n_lv, n_fin};
    unsigned long long* const dst[3] = {&stats[0], &stats[1], n_done};
    block_add<3>(v, dst);
}

// The sweep's launches over one walk and one sampling.  run_locate_sweep calls them after this frame has gone, so they hold the view
// and everything else by value.  front: null unless the resolve regroups by it (SweepKernels).
template <class Walk, class Sampling, typename pos_t, bool kWide>
SweepKernels bind_sweep(const typename Walk::View& iv, const SweepJob<pos_t>& job, uint8_t* front)
{
    const uint64_t* const d_l = job.d_l; const uint64_t* const d_out_off = job.d_out_off; const uint64_t n_pat = job.n_lists;      // (of the job, the launches hold these five)
    unsigned long long* const d_stats = job.d_stats; const hipStream_t stream = job.stream;
    SweepKernels K;
    K.n = iv.n;
    K.sigma = (uint32_t)iv.sigma;
    K.front = front;
    K.first = [=](uint64_t t0, uint64_t t1, uint64_t* val, uint16_t* key, void* out, unsigned long long* counter, const Block* mem, uint64_t* rc, bool ahead,
                  uint32_t* chunk_list, bool compact) {
        launch_sweep_chunk_lists(d_out_off, n_pat, t0, t1, chunk_list, stream);
        const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(sweep_turns(t1 - t0), 8192)));
        return on_trails_ahead(mem != nullptr, ahead, [&](auto tr, auto ah) { return on_flag(compact, [&](auto cm) {
            return launch(sweep_first_kernel<Walk, Sampling, pos_t, decltype(tr)::value, kWide, decltype(ah)::value, decltype(cm)::value>, grid, stream, iv,
                          d_l, d_out_off, n_pat, t0, t1, val, key, static_cast<pos_t*>(out), d_stats, counter, mem, rc, chunk_list, front);
        }); });
    };
    K.step = [=](uint64_t* val, uint16_t* key, uint64_t alive, uint32_t step, void* out, unsigned long long* counter, const Block* mem, uint64_t* rc, uint64_t t0, bool probed) {
        return on_flag(mem != nullptr, [&](auto tr) {
            return launch(sweep_step_kernel<Walk, Sampling, pos_t, decltype(tr)::value, kWide>, launch_grid(alive, 4096), stream, iv, val, key, alive, step,
                          static_cast<pos_t*>(out), d_stats, counter, mem, rc, t0, probed);
        });
    };
    K.tail = [=](void* out, uint64_t alive, uint32_t per_wave, const uint64_t* val, uint32_t step, uint64_t* rc, uint64_t t0, const Block* mem, uint32_t blocks) {
        return launch(locate_kernel<Walk, Sampling, pos_t, true, kWide>, dim3(blocks), stream, iv, static_cast<pos_t*>(out), alive, per_wave, d_stats, val, step, rc, t0, mem);
    };
    return K;
}

// Every SA index is sampled (SA-order samples of density 1): no walk, no trails, no records -- the sweep is `copy`, one launch
template <typename pos_t, class Copy>
vlg_status sweep_dense_copy(const SweepJob<pos_t>& job, const Copy& copy)
{
    if (vlg_status s = timed(job.timer, 0, 0, copy)) return s;
    return job.while_first_step ? (*job.while_first_step)() : VLG_OK;
}

}  // namespace vlg
