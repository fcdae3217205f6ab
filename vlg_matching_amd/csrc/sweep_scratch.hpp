// Sorted sweep: where its arrays lie in the scratch the physical pass carves and what its control block takes, written so that a CPU
// program compiles it too (tests/sweep_scratch_check.cpp), like filter_shape.hpp: no HIP header, no workspace, no allocation.
// Per element of one sweep: val[0], val[1] (8 B each; val[1] doubles as round 0's chunk_list), key[0], key[1] (2 B each) -- DESIGN.md
// section 3 has the table.  The sorted lists reuse all of it once locate is done; K3u lays UnsampleScratch over the same bytes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vlg {
#ifndef VLG_SWEEP_CHUNK
#define VLG_SWEEP_CHUNK 2048
#endif
constexpr uint32_t kSweepChunk = VLG_SWEEP_CHUNK;   // consecutive elements a workgroup of a sweep round takes per turn
static_assert(kSweepChunk >= 256 && kSweepChunk % 256 == 0, "VLG_SWEEP_CHUNK: whole rows of the 256-thread workgroup");
static_assert(kSweepChunk <= 4096, "VLG_SWEEP_CHUNK: one wave scans a turn's (row, wave) survivor counts, 64 at most");
inline uint64_t sweep_turns(uint64_t elements) { return (elements + kSweepChunk - 1) / kSweepChunk; }
// a word and a partition key per element, twice: the partition alternates between the two pairs
constexpr uint64_t kSweepScratchPerElem = 2 * sizeof(uint64_t) + 2 * sizeof(uint16_t);
static_assert(kSweepScratchPerElem == 20, "the arena's plan and the sorted lists that reuse the scratch count 20 B per occurrence");

// Control block: the round's counter of finished elements; a compacting round 0 (sweep_kernels.hpp: commit_turn) adds the give-up
// word, the ticket counter and one status word per turn behind it -- sweep_control_words, a multiple of two: 16-byte clears.
constexpr uint32_t kSweepDone = 0, kSweepStalled = 1, kSweepTicket = 2, kSweepStatus = 4;
inline uint64_t sweep_control_words(uint64_t elements) { return kSweepStatus + ((sweep_turns(elements) + 1) & ~1ull); }
// bytes a round over `elements` occurrences clears and reads.  The carve never takes less than kSweepControlFloor (the counter and the
// three diagnostic words of VLG_RESOLVE_STATS behind it); the arena's plan charges a compacting sweep kSweepControlSlack on top.
inline uint64_t sweep_control_bytes(uint64_t elements, bool compact) { return 8 * (compact ? sweep_control_words(elements) : 1); }
constexpr uint64_t kSweepControlFloor = 32, kSweepControlSlack = 256;

struct SweepScratch {
    uint64_t* val[2];                   // [0]: the elements as they stand; [1]: where the next partition puts them (it swaps the two)
    uint16_t* key[2];
    void* temp; size_t temp_bytes;      // sweep_temp_bytes
    unsigned long long* control;        // sweep_control_bytes, at least kSweepControlFloor
    // the four regions over kSweepScratchPerElem x cap bytes at `scratch` (aligned for uint64_t)
    static SweepScratch over(uint8_t* scratch, uint64_t cap, void* temp, size_t temp_bytes, unsigned long long* control)
    {
        uint64_t* const v = reinterpret_cast<uint64_t*>(scratch);
        uint16_t* const k = reinterpret_cast<uint16_t*>(v + 2 * cap);
        return SweepScratch{{v, v + cap}, {k, k + cap}, temp, temp_bytes, control};
    }
    // round 0's scratch, one word per turn (sweep_chunk_lists_kernel writes it, sweep_first_kernel reads it): the round writes val[0] / key[0] only
    uint32_t* chunk_list() const { return reinterpret_cast<uint32_t*>(val[1]); }
};
// sweep_turns(cap) <= cap words of chunk_list fit the cap words of val[1] as long as a word of the one is no larger than a word of the other
static_assert(sizeof(*SweepScratch().chunk_list()) <= sizeof(*SweepScratch().val[1]), "chunk_list: 4 B per kSweepChunk elements <= 8 B per element");

// K3u (kernels.hip: launch_unsample): the whole suffix array, n words of 32 bits, and behind it the sweep's regions for n_samples walkers
inline uint64_t unsample_sa_bytes(uint64_t n) { return (n * 4 + 255) / 256 * 256; }
inline uint64_t unsample_scratch_bytes(uint64_t n, uint64_t n_samples) { return unsample_sa_bytes(n) + n_samples * kSweepScratchPerElem + 1024; }
struct UnsampleScratch {
    uint32_t* sa_full;
    SweepScratch walkers;
    static UnsampleScratch over(uint8_t* scratch, uint64_t n, uint64_t n_samples, void* temp, size_t temp_bytes, unsigned long long* control)
    {
        return UnsampleScratch{reinterpret_cast<uint32_t*>(scratch), SweepScratch::over(scratch + unsample_sa_bytes(n), n_samples, temp, temp_bytes, control)};
    }
};
}  // namespace vlg
