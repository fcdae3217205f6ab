// Text access on the device (vlg_hip.h: vlg_text_access_create, vlg_extract_batch, vlg_isa_batch): the walks behind
// sdsl::extract(csa, begin, end) (include/sdsl/suffix_array_algorithm.hpp:645-745, lf_tag) and csa.isa[i] (csa_wt.hpp:145-151), from
// ISA samples ISA[0], ISA[d], ISA[2d], ... kept in HBM.  The bodies are generic in the LF step (lf_walk.hpp): kernels.hip instantiates
// them with ByteWalk on the Huffman-shaped tree, int_index.hpp with IntWalk on the wavelet matrix.
//
// Extract: a range [b, e] is cut at the multiples of d into segments, segment s = [s d, (s + 1) d) & [b, e], and one lane owns one
// segment.  It starts at ISA[(s + 1) d] -- or at ISA[0] when (s + 1) d >= n, which stands for ISA[n] because the text is cyclic:
// bwt[ISA[0]] = T[n - 1], the sentinel -- and walks LF backward: at SA index ISA[q] the BWT symbol is T[q - 1] and LF gives ISA[q - 1].
// It writes a symbol only once its position lies in the range, so no lane takes more than d steps however long the range is.
// Lanes take consecutive segments (a grid-stride loop over the global segment number), so the lanes of a wave mostly walk the same
// number of steps.  The writes go straight to HBM: DESIGN §8 (text access) has the measurement that decided against staging them in LDS.
// ISA: one lane per query p starts at the sample at ceil(p / d) d (the same wrap to ISA[0]) and takes fewer than d LF steps.
#pragma once
#include "common.hpp"

namespace vlg {

// what an extract launch reads (by value); seg_off: exclusive scan of the ranges' segment counts, n_ranges + 1 words
struct ExtractJob {
    const uint64_t* begin;
    const uint64_t* end;
    const uint64_t* out_off;
    const uint64_t* seg_off;
    uint64_t n_ranges, n_segs, n;
    uint32_t d;
};

// bytes of one ISA sample: SA indices are < n
inline uint32_t isa_sample_bytes(uint64_t n) { return n < (1ull << 32) ? 4u : 8u; }

// the range of global segment g: the last r with seg_off[r] <= g (every range has at least one segment)
__device__ __forceinline__ uint64_t extract_range_of(const uint64_t* __restrict__ seg_off, uint64_t n_ranges, uint64_t g)
{
    uint64_t lo = 0, hi = n_ranges;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (seg_off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Walk: lf(i, c) -> LF(i) with c = the compact symbol bwt[i]; sym(c) -> the original symbol (comp2char)
template <typename isa_t, typename sym_t, class Walk>
__device__ __forceinline__ void extract_segments(const ExtractJob& job, const isa_t* __restrict__ isa, sym_t* __restrict__ out, const Walk& walk)
{
    const uint64_t d = job.d;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < job.n_segs; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = extract_range_of(job.seg_off, job.n_ranges, g);
        const uint64_t b = job.begin[r], e = job.end[r], o = job.out_off[r];
        const uint64_t s = b / d + (g - job.seg_off[r]);
        const uint64_t lo = b > s * d ? b : s * d, last = s * d + d - 1, hi = e < last ? e : last;
        uint64_t q = (s + 1) * d, i;
        if (q < job.n) i = (uint64_t)isa[s + 1];
        else { q = job.n; i = (uint64_t)isa[0]; }
        while (q > lo) {                                     // at SA index ISA[q]: bwt = T[q - 1], LF = ISA[q - 1]
            uint32_t c;
            const uint64_t i2 = walk.lf(i, c);
            --q;
            if (q <= hi) out[o + (q - b)] = walk.sym(c);
            i = i2;
        }
    }
}

// out[j] = ISA[p[j]]; a p >= n raises *bad and leaves out[j] as it is
template <typename isa_t, class Walk>
__device__ __forceinline__ void isa_queries(const uint64_t* __restrict__ p_in, uint64_t* __restrict__ out, uint64_t count, uint64_t n, uint32_t d,
                                            const isa_t* __restrict__ isa, const Walk& walk, unsigned long long* __restrict__ bad)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = p_in[j];
        if (p >= n) { atomicAdd(bad, 1ull); continue; }
        const uint64_t k = (p + d - 1) / d;
        uint64_t q = k * d, i;
        if (q < n) i = (uint64_t)isa[k];
        else { q = n; i = (uint64_t)isa[0]; }
        for (; q > p; --q) {
            uint32_t c;
            i = walk.lf(i, c);
        }
        out[j] = i;
    }
}

}  // namespace vlg
