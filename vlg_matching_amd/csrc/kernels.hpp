// Internal launch interface between kernels.hip and search.hip.  A launcher takes a view and decides nothing about its shape by hand:
// which instantiation runs -- bit-vector kind, index width, sampling -- is chosen through shape_dispatch.hpp, inside the launcher.
#pragma once
#include <algorithm>
#include <functional>
#include "common.hpp"
#include "sweep_scratch.hpp"

namespace vlg {

vlg_status launch_backward_search(const IndexView& iv, const uint8_t* d_blob, const uint64_t* d_off, uint64_t n_pat, uint64_t* d_l,
                                  uint64_t* d_r, unsigned long long* d_stat_levels, hipStream_t stream);
// Branching backward search (branching_search_kernel): the SA intervals of n_tasks sub-patterns whose positions are sets of bytes.
// d_task[2 t] = first row of d_masks (32 bytes per position), d_task[2 t + 1] = positions; d_frontier: 2 x n_tasks x cap intervals
// (l, r) of scratch, 16-byte aligned -- task t's result is d_frontier[2 (t cap + i)], [.. + 1] for i < d_count[t], ascending and
// disjoint; d_count[t] = kClassSearchOverflow when the frontier of t would have passed `cap` intervals (nothing is written beyond it).
// budget: d_task[2 t + 1] carries a mismatch budget k (1 .. 255, at most the positions) in its top byte, and task t's result is one
// interval per distinct string within Hamming distance k of the rows that occurs in the text; without it, one per member string.
constexpr uint32_t kClassIntervalsMax = 1u << 20;
constexpr uint32_t kClassSearchOverflow = 0xFFFFFFFFu;
vlg_status launch_branching_search(const IndexView& iv, bool budget, const uint8_t* d_masks, const uint64_t* d_task, uint64_t n_tasks, uint32_t cap,
                                   uint64_t* d_frontier, uint32_t* d_count, unsigned long long* d_stat_levels, hipStream_t stream);
template <typename pos_t>
vlg_status launch_expand(const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, pos_t* d_io, uint32_t* d_seg,
                         hipStream_t stream);
template <typename pos_t>
vlg_status launch_locate(const IndexView& iv, pos_t* d_io, uint64_t total, unsigned long long* d_stats, hipStream_t stream);

// the build-time constants kernels.hip was compiled with (VLG_RESOLVE_HOPS, ...; reported by vlg_build_constants)
struct KernelConstants { int64_t resolve_hops, resolve_chunk, group_chunk, stage_lists, sweep_pairs, sweep_chunk; };
KernelConstants kernel_constants();

// Optional per-launch timing hooks (HIP events on the stream), implemented by the workspace.
struct LaunchTimer {
    virtual ~LaunchTimer() {}
    virtual void begin(int which, uint64_t algorithmic_bytes = 0) = 0;     // which: 0 = LF step kernel, 1 = stable partition by symbol, 2 = trail record resolution
    virtual void end(int which) = 0;
};
template <class F> vlg_status timed(LaunchTimer* timer, int which, uint64_t algorithmic_bytes, const F& launch)    // `launch` between the timer's two events
{
    if (timer) timer->begin(which, algorithmic_bytes);
    const vlg_status s = launch();
    if (timer) timer->end(which);
    return s;
}

// The slices the refilling-lane kernels (locate_kernel, unsample_tail_kernel) cut `count` elements into, one per wave: enough waves to
// fill 256 CUs x 32 waves several times over, but slices long enough (min_per_wave) that the drain tail -- the slowest element of a
// slice -- stays a small fraction of the slice.  blocks: workgroups of four waves.
struct LocateSlices { uint32_t per_wave, blocks; };
inline LocateSlices locate_slices(uint64_t count, uint64_t min_per_wave = 64 * 16)
{
    const uint64_t target_waves = 256ull * 32 * 4;
    const uint64_t per_wave = std::min<uint64_t>(std::max<uint64_t>((count + target_waves - 1) / target_waves, min_per_wave), 1u << 20);
    const uint64_t waves = (count + per_wave - 1) / per_wave;
    return LocateSlices{(uint32_t)per_wave, (uint32_t)((waves + 3) / 4)};
}

size_t sweep_temp_bytes(uint64_t total, uint32_t sigma, hipStream_t stream);
// occurrences one sweep can cover: slots share a 64-bit word with the SA index (32 + 32 bits, or 31 + 33 when SA indices are wide)
template <bool kWide> constexpr uint64_t sweep_batch_max() { return kWide ? (1ull << 31) : 0xFFFFFF00ull; }
template <typename pos_t> struct SweepJob {      // what a sorted sweep is asked to do
    // lists: SA interval starts and output offsets of the n_lists lists; d_out receives their `total` positions (unsorted, SA order)
    const uint64_t* d_l = nullptr; const uint64_t* d_out_off = nullptr; uint64_t n_lists = 0, total = 0; pos_t* d_out = nullptr;
    SweepScratch scratch{};     // for min(total, sweep_batch_max) elements (sweep_scratch.hpp)
    // sharing LF steps, all null or zero when none is shared: member_blocks(n) super-blocks, made up of the first n_member_lists lists
    // (pairwise disjoint, ascending); rec: `total` words; front: a byte per element, the symbol in front of it (SweepKernels; byte index)
    Block* member = nullptr; uint32_t n_member_lists = 0; uint64_t* rec = nullptr; uint8_t* front = nullptr;
    // run: at most tail_threshold elements go to the stragglers' kernel.  h_round: 16 pinned bytes for the `done` and give-up word of a
    // compacting round 0 (workspace option "sweep_compact"), null: round 0 does not compact.  while_first_step: host work, or null
    uint64_t tail_threshold = 0; unsigned long long* h_round = nullptr; unsigned long long* d_stats = nullptr;
    hipStream_t stream = nullptr; LaunchTimer* timer = nullptr; const std::function<vlg_status()>* while_first_step = nullptr;
};
// kWide: the index keeps 64-bit samples and SA indices may need 33 bits (n > 2^32, or VLG_FORCE_POS64); pos_t is the width of the
// text positions written -- uint32_t whenever the text has at most 2^32 characters, whatever the width of the SA indices.
template <typename pos_t, bool kWide> vlg_status launch_locate_sweep(const IndexView& iv, const SweepJob<pos_t>& job);
// the list that holds the first element of every chunk of a sweep [t0, t1): looked up for all chunks at once, in parallel, instead of by
// one lane of every workgroup in front of its work (a binary search is seventeen dependent loads)
void launch_sweep_chunk_lists(const uint64_t* d_out_off, uint64_t n_pat, uint64_t t0, uint64_t t1, uint32_t* chunk_list, hipStream_t stream);
// The three launches of a sorted sweep over some index (filled by bind_sweep, sweep_kernels.hpp; each returns the launch's status); run_locate_sweep
// owns the rounds, the partitions, the member bit-vector, the records and their resolution.  `out` is the sweep's slice of the position array (pos_t*).
struct SweepKernels {
    // front[slot] (optional, with records): the compact symbol read in front of an element that stopped on its first step, 0xFF otherwise
    // -- what the resolve regroups a workgroup's records by, so that the first hop of neighbouring lanes reads neighbouring records
    uint8_t* front = nullptr;
    uint64_t n = 0;
    uint32_t sigma = 0;                  // partition keys are the symbols 0 .. sigma - 1 (16 bits at most); sigma = finished
    // round 0 of the elements [t0, t1): their words follow from their places (lists l / out_off are the launcher's business)
    // compact: the survivors are written densely, in order, to the front of val / key and nothing else is (n_done then heads a
    // cleared block of sweep_control_bytes); otherwise, and in every later round, an element keeps its place and a finished one gets
    // key = sigma
    std::function<vlg_status(uint64_t t0, uint64_t t1, uint64_t* val, uint16_t* key, void* out, unsigned long long* n_done, const Block* member, uint64_t* rec, bool ahead,
                       uint32_t* chunk_list /* scratch, one word per kSweepChunk elements: sweep_chunk_lists_kernel */, bool compact)> first;
    // one round of the elements val / key [0, alive)
    std::function<vlg_status(uint64_t* val, uint16_t* key, uint64_t alive, uint32_t step, void* out, unsigned long long* n_done, const Block* member, uint64_t* rec, uint64_t t0,
                       bool probed)> step;
    // the stragglers, unsorted: a wave owns per_wave elements of val
    std::function<vlg_status(void* out, uint64_t alive, uint32_t per_wave, const uint64_t* val, uint32_t step, uint64_t* rec_or_null, uint64_t t0, const Block* member,
                       uint32_t blocks)> tail;
};
template <typename pos_t, bool kWide> vlg_status run_locate_sweep(const SweepKernels& K, const SweepJob<pos_t>& job);
// super-blocks of the member bit-vector over the SA indices of a text of n - 1 characters (kernels.hip: sweep_element)
inline uint64_t member_blocks(uint64_t n) { return n / kBlockBits + 1; }
// K3u: the whole suffix array reconstructed from the samples (one LF walker per sample, n LF steps in all) into sa_full (n x 4 B),
// then the SA intervals of the lists copied into d_out.  For batches that locate a large part of all text positions.
// job.scratch: UnsampleScratch's walkers (n_samples of them); h_done: 8 pinned bytes.
template <bool kWide> vlg_status launch_unsample(const IndexView& iv, const SweepJob<uint32_t>& job, uint32_t* sa_full, unsigned long long* h_done);
template <typename T> vlg_status launch_narrow(const uint64_t* d_in, T* d_out, uint64_t count, hipStream_t stream);
template <typename T> vlg_status launch_widen(const T* d_in, uint64_t* d_out, uint64_t count, hipStream_t stream);

// integer-alphabet FM-index (int_index.hpp): backward_search over uint32_t symbols, csa[i] in place (n <= 2^32)
vlg_status launch_int_backward_search(const IntView& v, const uint8_t* d_blob, const uint64_t* d_off, uint64_t n_pat, uint64_t* d_l, uint64_t* d_r,
                                      unsigned long long* d_stat_levels, hipStream_t st);
vlg_status launch_int_locate(const IntView& v, uint32_t* d_io, uint64_t total, unsigned long long* d_stats, hipStream_t st);
vlg_status launch_int_locate_sweep(const IntView& v, const SweepJob<uint32_t>& job);
// SA-order density 1 (vlg_index_resample): locate copies SA intervals of the samples, which are the suffix array (sa_dense_copy_kernel)
vlg_status launch_sa_dense_copy(const uint32_t* sa, const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, uint32_t* d_out,
                                hipStream_t stream);
vlg_status launch_int_dense_copy(const IntView& v, const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, uint32_t* d_out, hipStream_t stream);
// every SA value of an SA-order integer index (n words), and its ISA samples ((n - 1) / inv_dens + 1 words): LF walks from the samples
vlg_status launch_int_sa_expand(const IntView& v, uint32_t* d_sa, hipStream_t st);
vlg_status launch_int_isa_samples(const IntView& v, uint32_t inv_dens, uint32_t* d_out, hipStream_t st);
// text access on an integer index (extract.hpp): extract of the job's segments into original symbols, ISA[d_i[j]] (a bad position raises *d_bad)
struct ExtractJob;
vlg_status launch_int_extract(const IntView& v, const ExtractJob& job, const uint32_t* d_isa, uint32_t* d_out, hipStream_t st);
vlg_status launch_int_isa(const IntView& v, uint32_t d, const uint32_t* d_isa, const uint64_t* d_i, uint64_t* d_out, uint64_t count,
                          unsigned long long* d_bad, hipStream_t st);
// select on an integer index (select.hpp): wt_int::select(d_arg[j], d_sym[j]), or with d_sym null csa.psi[d_arg[j]]; csa.lf / csa.bwt of
// d_i (either output may be null; bwt in original symbols)
struct SelView;
vlg_status launch_int_select(const IntView& v, const SelView& sv, const uint64_t* d_arg, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, hipStream_t st);
vlg_status launch_int_lf_bwt(const IntView& v, const uint64_t* d_i, uint64_t* d_lf, uint32_t* d_bwt, uint64_t count, hipStream_t st);
// can this index's occurrences be located by the sorted sweep at all (the byte index always; the integer index with a 16-bit key)
inline bool int_sweep_possible(const IntView& v) { return v.sigma < 0xFFFFu && v.n_levels >= 1 && v.n <= (1ull << 32); }

}  // namespace vlg
