// CPU check of the sorted sweep's scratch layout (vlg_matching_amd/csrc/sweep_scratch.hpp), built and run by tests/test_sweep_scratch.py:
// the header the physical pass and the sweep's driver compile, against
//   1. the rules a layout must keep: regions pairwise disjoint, each aligned for its type, all inside the bytes the arena carves for
//      them, round 0's chunk_list inside val[1];
//   2. a literal restatement of the expressions the header replaced (commit faf97f6: PhysicalPass::locate, choose_physical,
//      plan_super_chunk, PhysicalPass::carve and run_locate_sweep): same pointers, same byte counts.
// Large capacities are arithmetic on a made-up base address: nothing is dereferenced.
#include "sweep_scratch.hpp"
#include <algorithm>
#include <cstdio>
#include <initializer_list>
using namespace vlg;

struct Region { const char* name; uintptr_t begin, end, align; };

// pairwise disjoint, aligned, inside [base, base + bytes)
static bool regions_ok(const char* what, std::initializer_list<Region> rs, uintptr_t base, uint64_t bytes)
{
    for (const Region& a : rs) {
        if (a.begin % a.align) { printf("%s: %s is not aligned to %llu\n", what, a.name, (unsigned long long)a.align); return false; }
        if (a.begin < base || a.end < a.begin || a.end > base + bytes) { printf("%s: %s leaves the scratch\n", what, a.name); return false; }
        for (const Region& b : rs)
            if (&a != &b && a.begin < b.end && b.begin < a.end) { printf("%s: %s and %s overlap\n", what, a.name, b.name); return false; }
    }
    return true;
}
static uintptr_t at(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ---- the parent commit's expressions -----------------------------------------------------------------
static uint64_t old_align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
static uint64_t old_sweep_turns(uint64_t elements) { return (elements + kSweepChunk - 1) / kSweepChunk; }
static uint64_t old_sweep_control_words(uint64_t elements) { return 4 + ((old_sweep_turns(elements) + 1) & ~1ull); }
static uint64_t old_plan_bytes(uint64_t phys, bool sweep_compact) { return sweep_compact ? old_sweep_control_words(phys) * 8 + 256 : 0; }
static uint64_t old_carve_words(uint64_t sweep_cap, bool sweep_compact) { return std::max<uint64_t>(4, sweep_compact ? old_sweep_control_words(sweep_cap) : 0); }
static uint64_t old_clear_bytes(uint64_t alive, bool compact) { return compact ? old_sweep_control_words(alive) * 8 : 8; }
static uint64_t old_unsample_bytes(uint64_t n, uint64_t n_walkers) { return old_align_up(n * 4, 256) + n_walkers * 20 + 1024; }

int main()
{
    uint8_t* const base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 40);       // what Arena::take returns is aligned to 256
    unsigned long long checked = 0;

    for (uint64_t cap : {1ull, 63ull, 64ull, 65ull, (unsigned long long)kSweepChunk - 1, (unsigned long long)kSweepChunk, (unsigned long long)kSweepChunk + 1, 1ull << 31,
                         0xFFFFFF00ull}) {
        int temp_here = 0;
        unsigned long long control_here = 0;
        const SweepScratch s = SweepScratch::over(base, cap, &temp_here, 77, &control_here);
        const uintptr_t list = at(s.chunk_list()), list_end = list + sweep_turns(cap) * sizeof(uint32_t);
        bool ok = regions_ok("sweep", {{"val[0]", at(s.val[0]), at(s.val[0] + cap), alignof(uint64_t)}, {"val[1]", at(s.val[1]), at(s.val[1] + cap), alignof(uint64_t)},
                                       {"key[0]", at(s.key[0]), at(s.key[0] + cap), alignof(uint16_t)}, {"key[1]", at(s.key[1]), at(s.key[1] + cap), alignof(uint16_t)}},
                              at(base), cap * kSweepScratchPerElem);
        ok = ok && list % alignof(uint32_t) == 0 && list >= at(s.val[1]) && list_end <= at(s.val[1] + cap);
        // the parent's arithmetic: val_a = scratch; val_b = val_a + cap; key_a = (uint16_t*)(val_b + cap); key_b = key_a + cap; chunk_list = (uint32_t*)val_b
        uint64_t* const val_a = reinterpret_cast<uint64_t*>(base);
        uint64_t* const val_b = val_a + cap;
        uint16_t* const key_a = reinterpret_cast<uint16_t*>(val_b + cap);
        ok = ok && s.val[0] == val_a && s.val[1] == val_b && s.key[0] == key_a && s.key[1] == key_a + cap && at(s.chunk_list()) == at(val_b);
        ok = ok && s.temp == &temp_here && s.temp_bytes == 77 && s.control == &control_here;
        if (!ok) { printf("sweep layout: cap %llu\n", (unsigned long long)cap); return 1; }
        ++checked;
    }

    for (uint64_t m : {1ull, 5ull, 1000ull, 1ull << 24}) for (int d : {-1, 0, 1}) for (uint64_t dens : {2ull, 32ull}) {
        const uint64_t n = m * 64 + d, n_samples = (n + dens - 1) / dens;
        const uint64_t bytes = unsample_scratch_bytes(n, n_samples);
        const UnsampleScratch u = UnsampleScratch::over(base, n, n_samples, nullptr, 0, nullptr);
        const SweepScratch& w = u.walkers;
        bool ok = regions_ok("K3u", {{"sa_full", at(u.sa_full), at(u.sa_full + n), alignof(uint32_t)},
                                     {"val[0]", at(w.val[0]), at(w.val[0] + n_samples), alignof(uint64_t)}, {"val[1]", at(w.val[1]), at(w.val[1] + n_samples), alignof(uint64_t)},
                                     {"key[0]", at(w.key[0]), at(w.key[0] + n_samples), alignof(uint16_t)}, {"key[1]", at(w.key[1]), at(w.key[1] + n_samples), alignof(uint16_t)}},
                             at(base), bytes);
        ok = ok && bytes == old_unsample_bytes(n, n_samples);
        // the parent's arithmetic: sa_full = scratch; val_a = scratch + align_up(n * 4, 256); val_b = val_a + n_walkers; key_a behind val_b; key_b = key_a + n_walkers
        uint64_t* const val_a = reinterpret_cast<uint64_t*>(base + old_align_up(n * 4, 256));
        uint16_t* const key_a = reinterpret_cast<uint16_t*>(val_a + 2 * n_samples);
        ok = ok && at(u.sa_full) == at(base) && w.val[0] == val_a && w.val[1] == val_a + n_samples && w.key[0] == key_a && w.key[1] == key_a + n_samples;
        if (!ok) { printf("K3u layout: n %llu, %llu samples\n", (unsigned long long)n, (unsigned long long)n_samples); return 1; }
        ++checked;
    }

    for (uint64_t e : {0ull, 1ull, (unsigned long long)kSweepChunk - 1, (unsigned long long)kSweepChunk, (unsigned long long)kSweepChunk + 1, 1000000000ull}) for (bool compact : {false, true}) {
        // the three places that size the block, each as its line reads now (search.hip: plan_super_chunk, PhysicalPass::carve; kernels.hip: SweepRun::round)
        const uint64_t plan = compact ? sweep_control_bytes(e, true) + kSweepControlSlack : 0;
        const uint64_t carve_words = std::max(kSweepControlFloor, sweep_control_bytes(e, compact)) / 8;
        const uint64_t clear = sweep_control_bytes(e, compact);
        if (plan != old_plan_bytes(e, compact) || carve_words != old_carve_words(e, compact) || clear != old_clear_bytes(e, compact) || clear % 8 || (compact && clear % 16) ||
            clear > carve_words * 8 || sweep_control_words(e) != old_sweep_control_words(e)) {
            printf("control block: %llu elements, compact %d: plan %llu, carve %llu words, clear %llu\n", (unsigned long long)e, (int)compact, (unsigned long long)plan,
                   (unsigned long long)carve_words, (unsigned long long)clear);
            return 1;
        }
        ++checked;
    }
    printf("ok %llu layouts\n", checked);
    return 0;
}
