// K1 batched bit-rank, K2 wavelet-tree rank / backward search, K3 locate (LF iteration).
#include <algorithm>
#include <cstring>
#include <string.h>
#include <vector>
#include "common.hpp"
#include "kernels.hpp"
#include "sweep_kernels.hpp"
#include "extract.hpp"
#include "select.hpp"
#include <rocprim/rocprim.hpp>

using namespace vlg;

// =============================================================================================
// K1: rank_support_v<1,1>::rank on a plain bit-vector (include/sdsl/rank_support_v.hpp:114-124)
// =============================================================================================
struct vlg_bitvector {
    Block* d_blocks = nullptr;
    uint64_t nbits = 0;
    uint64_t n_blocks = 0;
};

namespace {

// host words -> blocks. One thread per block: 7 data words + running count comes from a scan.
__global__ void bv_pack_kernel(const uint64_t* __restrict__ src, uint64_t src_words, uint64_t nbits, Block* __restrict__ blocks,
                               uint64_t n_blocks, uint32_t* __restrict__ pops)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t pc = 0;
        Block B;
#pragma unroll
        for (uint32_t w = 0; w < 7; ++w) {
            uint64_t bit = b * kBlockBits + 32u * w;
            uint32_t val = 0;
            if (bit < nbits) {
                uint64_t wi = bit >> 6;
                uint32_t s = (uint32_t)(bit & 63);
                uint64_t lo = src[wi] >> s;
                if (s > 32 && wi + 1 < src_words) lo |= src[wi + 1] << (64 - s);
                val = (uint32_t)lo;
                uint64_t left = nbits - bit;
                if (left < 32) val &= (1u << left) - 1u;
            }
            B.w[w] = val;
            pc += __popc(val);
        }
        B.cnt = 0;
        blocks[b] = B;
        pops[b] = pc;
    }
}

// single-workgroup-per-tile scan is plenty for a creation-time pass: serial over tiles of 1024 blocks
__global__ void bv_count_kernel(Block* __restrict__ blocks, const uint32_t* __restrict__ pops, uint64_t n_blocks)
{
    // one workgroup, chunked inclusive scan with a running carry
    __shared__ uint32_t s[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < n_blocks; base += 1024) {
        uint64_t i = base + threadIdx.x;
        uint32_t v = i < n_blocks ? pops[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {
            uint32_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n_blocks) blocks[i].cnt = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) bitrank_kernel(const Block* __restrict__ blocks, const uint64_t* __restrict__ idx,
                                                       uint64_t* __restrict__ out, uint64_t count)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x)
        out[j] = node_rank1(blocks, 0, idx[j]);
}

}  // namespace

extern "C" vlg_status vlg_bitvector_create(const uint64_t* h_words, uint64_t nbits, vlg_bitvector** out)
{
    if (!out || (nbits && !h_words)) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available");
    if (nbits >= (1ull << 32)) return fail(VLG_E_UNSUPPORTED, "stand-alone bit-vectors are limited to 2^32-1 bits (32-bit block counts)");
    Building<vlg_bitvector, vlg_bitvector_destroy> bv(new vlg_bitvector());
    bv->nbits = nbits;
    bv->n_blocks = nbits / kBlockBits + 1;
    uint64_t words = (nbits + 63) / 64;
    DevBuf d_src, d_pops;
    VLG_HIP_TRY(hipMalloc((void**)&bv->d_blocks, bv->n_blocks * sizeof(Block)));
    VLG_HIP_TRY(d_src.alloc(words * 8 + 8));
    VLG_HIP_TRY(d_pops.alloc(bv->n_blocks * 4));
    if (words) VLG_HIP_TRY(hipMemcpy(d_src.p, h_words, words * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(bv_pack_kernel, launch_grid(bv->n_blocks, 8192), dim3(256), 0, nullptr, d_src.as<uint64_t>(), words, nbits, bv->d_blocks, bv->n_blocks,
                       d_pops.as<uint32_t>());
    hipLaunchKernelGGL(bv_count_kernel, dim3(1), dim3(1024), 0, nullptr, bv->d_blocks, d_pops.as<uint32_t>(), bv->n_blocks);
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipDeviceSynchronize());
    *out = bv.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_bitvector_rank_batch(const vlg_bitvector* bv, const uint64_t* d_idx, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!bv || (count && (!d_idx || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipLaunchKernelGGL(bitrank_kernel, launch_grid(count, 8192), dim3(256), 0, (hipStream_t)stream, bv->d_blocks, d_idx, d_out, count);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

extern "C" uint64_t vlg_bitvector_hbm_bytes(const vlg_bitvector* bv) { return bv ? bv->n_blocks * sizeof(Block) : 0; }

extern "C" void vlg_bitvector_destroy(vlg_bitvector* bv)
{
    if (!bv) return;
    if (bv->d_blocks) (void)hipFree(bv->d_blocks);
    delete bv;
}

// =============================================================================================
// K6: rank on an H0-compressed bit-vector -- rrr_vector<63> / rank_support_rrr<1,63>
//     (include/sdsl/rrr_vector.hpp:444-480; coding include/sdsl/rrr_helper.hpp:304-320, 411-460).
// Blocks of 63 bits are stored as (class = popcount, offset = rank of the block among all blocks of that class in
// the combinatorial number system); 32 blocks form a super-block.  HBM layout, one aligned 32-byte header per
// super-block: { u32 ones before it, u32 bit position of its first offset, 32 x 6-bit classes }, offsets in a
// separate bit stream.  One rank = the header read + one read of <= 61 offset bits; the block is decoded on the fly
// against the binomial table C(n,k), n < 64, staged in LDS (32 KiB).
// =============================================================================================
struct vlg_rrr_bitvector {
    uint64_t nbits = 0, n_sb = 0, stream_words = 0;
    uint4* d_hdr = nullptr;          // 2 x uint4 per super-block
    uint64_t* d_stream = nullptr;
    uint64_t* d_binom = nullptr;     // [64][64]
};

namespace {

constexpr uint32_t kRrrBlock = 63, kRrrSuper = 32;

struct RrrLds {
    uint64_t binom[64][64];
    uint8_t space[64];
};

// the binomial table into LDS and, from its row 63, the offset widths (every K6 kernel starts with this; ends with a barrier)
__device__ __forceinline__ void stage_rrr_lds(RrrLds& s, const uint64_t* __restrict__ binom)
{
    for (uint32_t i = threadIdx.x; i < 64 * 64; i += blockDim.x) (&s.binom[0][0])[i] = binom[i];
    __syncthreads();
    if (threadIdx.x < 64) {                      // space_for_bt: bits of C(63,k), 0 for the two uniform classes
        uint64_t c = s.binom[63][threadIdx.x];
        s.space[threadIdx.x] = (c == 1) ? 0 : (uint8_t)(64 - __clzll((long long)c));
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t rrr_class(uint64_t c0, uint64_t c1, uint64_t c2, uint32_t j)
{
    uint32_t bit = 6u * j;                       // classes are packed little-endian into 192 bits
    uint32_t w = bit >> 6, o = bit & 63;
    uint64_t lo = w == 0 ? c0 : (w == 1 ? c1 : c2);
    uint64_t hi = w == 0 ? c1 : c2;
    uint64_t v = lo >> o;
    if (o > 58) v |= hi << (64 - o);
    return (uint32_t)v & 63u;
}

__global__ void __launch_bounds__(256) rrr_rank_kernel(const uint4* __restrict__ hdr, const uint64_t* __restrict__ stream,
                                                       const uint64_t* __restrict__ binom, const uint64_t* __restrict__ idx,
                                                       uint64_t* __restrict__ out, uint64_t count)
{
    __shared__ RrrLds s;
    stage_rrr_lds(s, binom);
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = idx[q];
        const uint64_t sb = i / (kRrrBlock * kRrrSuper);
        const uint32_t r = (uint32_t)(i - sb * (kRrrBlock * kRrrSuper));
        const uint32_t blk = r / kRrrBlock, off = r - blk * kRrrBlock;
        const uint4 h0 = hdr[2 * sb], h1 = hdr[2 * sb + 1];
        uint64_t rank = h0.x;
        uint64_t ptr = h0.y;
        const uint64_t c0 = (uint64_t)h0.z | ((uint64_t)h0.w << 32), c1 = (uint64_t)h1.x | ((uint64_t)h1.y << 32),
                       c2 = (uint64_t)h1.z | ((uint64_t)h1.w << 32);
        for (uint32_t j = 0; j < blk; ++j) {     // rrr_vector.hpp:463-467
            uint32_t k = rrr_class(c0, c1, c2, j);
            rank += k;
            ptr += s.space[k];
        }
        if (off) {
            uint32_t k = rrr_class(c0, c1, c2, blk);
            const uint32_t len = s.space[k];
            uint64_t nr = rrr_stream_bits(stream, ptr, len);
            // decode_popcount (rrr_helper.hpp:411-460): walk the block from bit 0, C(nn-1,k) decides each bit
            uint32_t ones = 0;
            if (k == kRrrBlock) ones = off;
            else if (k) {
                uint32_t nn = kRrrBlock;
                for (uint32_t b = 0; b < off && k; ++b, --nn) {
                    const uint64_t c = s.binom[nn - 1][k];
                    if (nr >= c) { nr -= c; --k; ++ones; }
                }
            }
            rank += ones;
        }
        out[q] = rank;
    }
}

}  // namespace

extern "C" vlg_status vlg_rrr_bitvector_create(const uint64_t* h_words, uint64_t nbits, vlg_rrr_bitvector** out)
{
    if (!out || (nbits && !h_words)) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available");
    if (nbits >= (1ull << 32)) return fail(VLG_E_UNSUPPORTED, "stand-alone bit-vectors are limited to 2^32-1 bits");
    // binomial table (rrr_helper.hpp:173-207)
    std::vector<uint64_t> binom(64 * 64, 0);
    for (int nn = 0; nn < 64; ++nn) binom[nn * 64] = 1;
    for (int nn = 1; nn < 64; ++nn)
        for (int k = 1; k < 64; ++k) binom[nn * 64 + k] = (k == nn) ? 1 : (k > nn ? 0 : binom[(nn - 1) * 64 + k - 1] + binom[(nn - 1) * 64 + k]);
    auto space = [&](uint32_t k) -> uint32_t { uint64_t c = binom[63 * 64 + k]; return c == 1 ? 0 : 64 - (uint32_t)__builtin_clzll(c); };
    auto get = [&](uint64_t pos, uint32_t len) -> uint64_t {      // bits [pos, pos+len) of the input, zero beyond nbits
        uint64_t v = 0;
        for (uint32_t b = 0; b < len; ) {
            uint64_t p = pos + b;
            if (p >= nbits) break;
            uint64_t w = p >> 6, o = p & 63;
            uint32_t take = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(64 - o, len - b), nbits - p);
            uint64_t chunk = (h_words[w] >> o) & (take == 64 ? ~0ull : ((1ull << take) - 1));
            v |= chunk << b;
            b += take;
        }
        return v;
    };
    const uint64_t n_blocks = nbits / kRrrBlock + 1;
    const uint64_t n_sb = (n_blocks + kRrrSuper - 1) / kRrrSuper;
    std::vector<uint32_t> hdr(n_sb * 8, 0);
    std::vector<uint64_t> stream(1, 0);
    uint64_t sbits = 0, ones = 0;
    for (uint64_t sb = 0; sb < n_sb; ++sb) {
        uint32_t* H = &hdr[sb * 8];
        H[0] = (uint32_t)ones;
        H[1] = (uint32_t)sbits;
        uint64_t cls[3] = {0, 0, 0};
        for (uint32_t j = 0; j < kRrrSuper; ++j) {
            uint64_t bin = get((sb * kRrrSuper + j) * kRrrBlock, kRrrBlock);
            uint32_t k = (uint32_t)__builtin_popcountll(bin);
            uint32_t bit = 6 * j, w = bit >> 6, o = bit & 63;
            cls[w] |= (uint64_t)k << o;
            if (o > 58) cls[w + 1] |= (uint64_t)k >> (64 - o);
            ones += k;
            uint32_t len = space(k);
            if (len) {                                               // bin_to_nr: rrr_helper.hpp:304-320
                uint64_t nr = 0, b = bin;
                uint32_t kk = k, nn = kRrrBlock;
                while (b) { if (b & 1) { nr += binom[(nn - 1) * 64 + kk]; --kk; } b >>= 1; --nn; }
                if ((sbits + len + 127) / 64 >= stream.size()) stream.resize(stream.size() * 2 + 4, 0);
                uint64_t w2 = sbits >> 6, o2 = sbits & 63;
                stream[w2] |= nr << o2;
                if (o2 + len > 64) stream[w2 + 1] |= nr >> (64 - o2);
                sbits += len;
            }
        }
        H[2] = (uint32_t)cls[0]; H[3] = (uint32_t)(cls[0] >> 32);
        H[4] = (uint32_t)cls[1]; H[5] = (uint32_t)(cls[1] >> 32);
        H[6] = (uint32_t)cls[2]; H[7] = (uint32_t)(cls[2] >> 32);
    }
    if (sbits >= (1ull << 32)) return fail(VLG_E_UNSUPPORTED, "offset stream longer than 2^32 bits");
    vlg_rrr_bitvector* bv = new vlg_rrr_bitvector();
    bv->nbits = nbits; bv->n_sb = n_sb; bv->stream_words = sbits / 64 + 2;
    stream.resize(bv->stream_words, 0);
    auto run = [&]() -> vlg_status {
        VLG_HIP_TRY(hipMalloc((void**)&bv->d_hdr, n_sb * 32));
        VLG_HIP_TRY(hipMalloc((void**)&bv->d_stream, bv->stream_words * 8));
        VLG_HIP_TRY(hipMalloc((void**)&bv->d_binom, 64 * 64 * 8));
        VLG_HIP_TRY(hipMemcpy(bv->d_hdr, hdr.data(), n_sb * 32, hipMemcpyHostToDevice));
        VLG_HIP_TRY(hipMemcpy(bv->d_stream, stream.data(), bv->stream_words * 8, hipMemcpyHostToDevice));
        VLG_HIP_TRY(hipMemcpy(bv->d_binom, binom.data(), 64 * 64 * 8, hipMemcpyHostToDevice));
        return VLG_OK;
    };
    vlg_status st = run();
    if (st) { vlg_rrr_bitvector_destroy(bv); return st; }
    *out = bv;
    return VLG_OK;
}

extern "C" vlg_status vlg_rrr_bitvector_rank_batch(const vlg_rrr_bitvector* bv, const uint64_t* d_idx, uint64_t* d_out, uint64_t count,
                                                   void* stream)
{
    if (!bv || (count && (!d_idx || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipLaunchKernelGGL(rrr_rank_kernel, launch_grid(count, 2048), dim3(256), 0, (hipStream_t)stream, bv->d_hdr, bv->d_stream, bv->d_binom, d_idx, d_out,
                       count);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

extern "C" uint64_t vlg_rrr_bitvector_hbm_bytes(const vlg_rrr_bitvector* bv) { return bv ? bv->n_sb * 32 + bv->stream_words * 8 : 0; }

extern "C" void vlg_rrr_bitvector_destroy(vlg_rrr_bitvector* bv)
{
    if (!bv) return;
    if (bv->d_hdr) (void)hipFree(bv->d_hdr);
    if (bv->d_stream) (void)hipFree(bv->d_stream);
    if (bv->d_binom) (void)hipFree(bv->d_binom);
    delete bv;
}

// =============================================================================================
// K2: wt_pc::rank (include/sdsl/wt_pc.hpp:350-373) and backward_search
//     (include/sdsl/suffix_array_algorithm.hpp:250-278, 305-326)
// =============================================================================================
namespace vlg {

// #c in BWT[0,i): walk the code of c from the root; one super-block read per level.
template <class BV>
__device__ __forceinline__ uint64_t wt_rank_dev(const IndexView& iv, const WalkLds<BV>& s, uint64_t path, uint64_t i, uint32_t& levels)
{
    uint32_t len = (uint32_t)(path >> 56);
    if (len == 0) return (iv.sigma == 1) ? i : 0;       // sigma==1: wt_pc.hpp:355-357 (the only symbol has an empty code)
    uint64_t res = i;
    uint32_t v = 0;
    for (uint32_t l = 0; l < len && res; ++l, path >>= 1) {       // "and result": wt_pc.hpp:361
        uint32_t bit = (uint32_t)(path & 1);
        uint64_t r1 = BV::rank(iv, s.sh, s.nodes[v].base, res);
        ++levels;
        res = bit ? r1 : res - r1;
        { const DNode nd = s.nodes[v]; v = (bit ? nd.child[1] : nd.child[0]) & ~kLeafFlag; }
    }
    return res;
}

}  // namespace vlg

namespace {

template <class BV>
__global__ void __launch_bounds__(256) wt_rank_kernel(IndexView iv, const uint64_t* __restrict__ pos, const uint8_t* __restrict__ sym,
                                                      uint64_t* __restrict__ out, uint64_t count)
{
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        uint8_t c = sym[j];
        uint64_t path = iv.paths[c];
        uint32_t lv = 0;
        bool present = (c == 0) || iv.char2comp[c] != 0;          // c_to_leaf valid  (wt_pc.hpp:352-354)
        out[j] = present ? wt_rank_dev(iv, s, path, pos[j], lv) : 0;
    }
}

// one lane per pattern; the two ranks of a step are independent loads
template <class BV>
__global__ void __launch_bounds__(256) backward_search_kernel(IndexView iv, const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off,
                                                              uint64_t n_pat, uint64_t* __restrict__ out_l, uint64_t* __restrict__ out_r,
                                                              unsigned long long* __restrict__ stat_levels)
{
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    uint32_t levels = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pat; p += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t b = off[p], e = off[p + 1];
        uint64_t l = 0, r = iv.n - 1;
        while (b < e && r + 1 - l > 0) {                          // suffix_array_algorithm.hpp:319
            --e;
            uint8_t c = blob[e];
            uint32_t cc = iv.char2comp[c];
            if (cc == 0 && c > 0) { l = 1; r = 0; }               // :263-265
            else {
                uint64_t c_begin = s.C[cc];
                if (l == 0 && r + 1 == iv.n) { l = c_begin; r = s.C[cc + 1] - 1; }      // :268-270
                else {
                    uint64_t path = iv.paths[c];
                    uint64_t nl = c_begin + wt_rank_dev(iv, s, path, l, levels);          // :272
                    uint64_t nr = c_begin + wt_rank_dev(iv, s, path, r + 1, levels) - 1;  // :273
                    l = nl; r = nr;
                }
            }
        }
        out_l[p] = l;
        out_r[p] = r;
    }
    if (stat_levels) {
        unsigned long long t = levels;
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(stat_levels, t);
    }
}

// The symbol list of a step of the branching search into one wave's `list`, ascending -> its length: the bytes 1..255 that the text
// has and, without a budget, that the class row holds.
template <bool kBudget>
__device__ __forceinline__ uint32_t list_symbols(const IndexView& iv, const uint8_t* row, uint8_t* list, uint32_t lane, unsigned long long below)
{
    uint32_t nsym = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t c = 64 * j + lane;
        bool on = c > 0 && iv.char2comp[c] != 0;
        if constexpr (!kBudget) on = c > 0 && ((row[c >> 3] >> (c & 7)) & 1u) && iv.char2comp[c] != 0;
        const unsigned long long b = __ballot(on);
        if (on) list[nsym + (uint32_t)__popcll(b & below)] = (uint8_t)c;
        nsym += (uint32_t)__popcll(b);
    }
    // (the list is read by other lanes of this wave than wrote it)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return nsym;
}

// K2c: branching backward search, one wavefront per sub-pattern (task): the SA intervals of every string that the sub-pattern stands
// for and that occurs.  Without a budget (kBudget = false) the positions are SETS of bytes (character classes) and the strings are the
// member strings of S_0 ... S_{m-1}; with one (kBudget = true) they are the strings within Hamming distance k of a member string.
// Scratch: the frontier -- the intervals of the strings of the steps done so far -- ping-pongs between two halves of `cap` intervals
// in global memory: half h of task t is frontier[(h * n_tasks + t) * cap ...].  The result ends in half 0; count[t] = its intervals,
// or kClassSearchOverflow when a step would have kept more than `cap` (nothing is written past the cap; exactly `cap` is legal).
// Order: a step deals the (symbol, parent interval) pairs to the lanes symbol-major, parent-minor, takes the two ranks of
// backward_search_kernel per pair, and compacts the non-empty results with a ballot and a popcount prefix.  The new left borders
// ascend (C[c] dominates; within one c the rank is monotone in the parent's l) whichever pairs are kept, so the frontier stays
// ascending and disjoint without a sort: one interval per distinct string that occurs.
// Tasks: task[2 t] = first mask row of the sub-pattern (32 bytes per position, bit c = byte c), task[2 t + 1] = its positions.
// kBudget adds: the budget k (1 .. 255) in the top byte of task[2 t + 1]; a symbol list of every byte 1..255 the text has -- the
// same at every step of every task, so a wave builds it once, in front of its tasks, where the class search builds the members of
// the step's row per step; the misses e of an entry's string so far in the top byte of its second word (l, r <= 2^33), with
// e' = e + !(row_p bit c) for a (symbol c, parent) pair; and the gate e' <= k, without which a pair takes no rank and keeps nothing.
// The last step writes its intervals without the miss count, so half 0 reads the same for either kind.
template <class BV, bool kBudget>
__global__ void __launch_bounds__(256) branching_search_kernel(IndexView iv, const uint8_t* __restrict__ masks, const uint64_t* __restrict__ task,
                                                               uint64_t n_tasks, uint32_t cap, ulonglong2* frontier, uint32_t* __restrict__ count,
                                                               unsigned long long* __restrict__ stat_levels)
{
    __shared__ WalkLds<BV> s;
    __shared__ uint8_t syms[4][256];                       // per wave, ascending: the members of the step's class that the text has / its bytes 1..255
    stage_walk(s, iv);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr uint64_t kEntryMask = (1ull << 56) - 1;
    uint32_t levels = 0;
    uint32_t nsym = 0;
    if constexpr (kBudget) nsym = list_symbols<true>(iv, nullptr, syms[wv], lane, below);
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < n_tasks; t += (uint64_t)gridDim.x * 4) {
        const uint64_t pos0 = task[2 * t];
        const uint32_t m = (uint32_t)(kBudget ? task[2 * t + 1] & kEntryMask : task[2 * t + 1]);
        [[maybe_unused]] uint32_t k = 0;
        if constexpr (kBudget) k = (uint32_t)(task[2 * t + 1] >> 56);
        ulonglong2* const half[2] = {frontier + t * cap, frontier + (n_tasks + t) * cap};
        uint32_t cur = 0, cnt = 1;                         // before the first step: the whole range (with no miss), which is not stored
        bool whole = true, over = false;
        for (uint32_t p = m; p-- > 0 && cnt && !over;) {
            const uint8_t* row = masks + (pos0 + p) * 32;
            if constexpr (!kBudget) nsym = list_symbols<false>(iv, row, syms[wv], lane, below);
            const ulonglong2* src = half[cur];
            ulonglong2* dst = half[cur ^ 1];
            const uint32_t total = nsym * cnt;             // (255 symbols, cap <= 2^20: fits)
            uint32_t out = 0;
            for (uint32_t base = 0; base < total && !over; base += 64) {
                const uint32_t i = base + lane;
                bool keep = false;
                uint64_t nl = 0, nr = 0;
                [[maybe_unused]] uint32_t e = 0;
                if (i < total) {
                    const uint32_t si = i / cnt, pi = i - si * cnt;
                    const uint8_t c = syms[wv][si];
                    uint64_t l = 0, r = iv.n - 1;
                    if (!whole) {
                        const ulonglong2 par = src[pi];
                        l = par.x; r = par.y;
                        if constexpr (kBudget) { r = par.y & kEntryMask; e = (uint32_t)(par.y >> 56); }
                    }
                    bool take = true;                      // kBudget: a parent at full budget takes its own symbols only
                    if constexpr (kBudget) { e += ((row[c >> 3] >> (c & 7)) & 1u) ^ 1u; take = e <= k; }
                    if (take) {
                        const uint32_t cc = iv.char2comp[c];
                        const uint64_t c_begin = s.C[cc];
                        if (l == 0 && r + 1 == iv.n) { nl = c_begin; nr = s.C[cc + 1] - 1; keep = s.C[cc + 1] > c_begin; }      // as backward_search_kernel
                        else {
                            const uint64_t path = iv.paths[c];
                            const uint64_t a = wt_rank_dev(iv, s, path, l, levels), b = wt_rank_dev(iv, s, path, r + 1, levels);
                            nl = c_begin + a; nr = c_begin + b - 1; keep = b > a;
                        }
                    }
                }
                const unsigned long long kb = __ballot(keep);
                const uint32_t at = out + (uint32_t)__popcll(kb & below);
                out += (uint32_t)__popcll(kb);
                if (out > cap) over = true;                // (wave-uniform) this turn would pass the cap: none of its lanes writes
                else if (keep) dst[at] = make_ulonglong2(nl, kBudget && p ? nr | ((uint64_t)e << 56) : nr);
            }
            cnt = out; cur ^= 1; whole = false;
            __threadfence();                               // the next step's lanes read what other lanes wrote
        }
        if (!over && cnt && cur == 1) for (uint32_t i = lane; i < cnt; i += 64) half[0][i] = half[1][i];
        if (lane == 0) count[t] = over ? kClassSearchOverflow : cnt;
    }
    if (stat_levels) {
        unsigned long long tl = levels;
        for (int o = 32; o > 0; o >>= 1) tl += __shfl_down(tl, o);
        if ((threadIdx.x & 63) == 0 && tl) atomicAdd(stat_levels, tl);
    }
}

// ---- member bit-vector: which SA indices are elements of the batch, and which (sweep_element explains what for) ----------------
// bit i = one of the lists [l[d], l[d] + off[d + 1] - off[d]), d < n_lists, holds SA index i; the lists are pairwise disjoint and
// ascend, and list d owns the slots [off[d], off[d + 1]) -- so the number of set bits before i IS the slot of index i.  Same 256-bit
// super-blocks as the wavelet tree (224 bits + the count before them), built block by block: no clearing pass, no atomics.
__global__ void __launch_bounds__(256) member_build_kernel(const uint64_t* __restrict__ l, const uint64_t* __restrict__ off, uint32_t n_lists,
                                                           uint64_t n_blocks, Block* __restrict__ out)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t B0 = b * kBlockBits, B1 = B0 + kBlockBits;
        uint32_t lo = 0, hi = n_lists;                       // first list that ends behind B0
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (l[mid] + (off[mid + 1] - off[mid]) <= B0) lo = mid + 1; else hi = mid;
        }
        uint32_t d = lo;
        Block B;
#pragma unroll
        for (uint32_t w = 0; w < 7; ++w) B.w[w] = 0;
        B.cnt = (uint32_t)(d < n_lists ? off[d] + (B0 > l[d] ? B0 - l[d] : 0) : off[n_lists]);
        for (; d < n_lists && l[d] < B1; ++d) {
            const uint64_t end = l[d] + (off[d + 1] - off[d]);
            const uint32_t a = (uint32_t)((l[d] > B0 ? l[d] : B0) - B0), e = (uint32_t)((end < B1 ? end : B1) - B0);
#pragma unroll
            for (uint32_t w = 0; w < 7; ++w) {
                const uint32_t x = a > 32 * w ? a : 32 * w, y = e < 32 * w + 32 ? e : 32 * w + 32;
                if (x < y) B.w[w] |= (y - x == 32 ? ~0u : ((1u << (y - x)) - 1u)) << (x - 32 * w);
            }
        }
        out[b] = B;
    }
}

// io[off[p] + j] = l[p] + j : the SA indices of every occurrence (input of locate_kernel), plus seg[]
template <typename pos_t>
__global__ void expand_kernel(const uint64_t* __restrict__ l, const uint64_t* __restrict__ out_off, uint64_t n_pat, uint64_t total,
                              pos_t* __restrict__ io, uint32_t* __restrict__ seg)
{
    // tile of 256 consecutive slots per workgroup iteration; first lane finds the segment by binary search
    __shared__ uint64_t s_first;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < total; base += (uint64_t)gridDim.x * 256) {
        if (threadIdx.x == 0) {
            uint64_t lo = 0, hi = n_pat;                   // last p with out_off[p] <= base
            while (hi - lo > 1) { uint64_t mid = (lo + hi) >> 1; if (out_off[mid] <= base) lo = mid; else hi = mid; }
            s_first = lo;
        }
        __syncthreads();
        uint64_t t = base + threadIdx.x;
        if (t < total) {
            uint64_t p = s_first;
            while (out_off[p + 1] <= t) ++p;               // empty segments are skipped too
            io[t] = (pos_t)(l[p] + (t - out_off[p]));
            if (seg) seg[t] = (uint32_t)p;
        }
        __syncthreads();
    }
}

// K3 (locate_kernel) and the rounds of K3s, the sorted sweep (sweep_first_kernel, sweep_step_kernel), are in sweep_kernels.hpp: the
// integer index runs them too.  What follows here are the sweep's passes that no LF step is taken in.
// val = slot << kShift | position: 32 + 32 bits for n <= 2^32, 31 + 33 bits beyond (then a sweep covers at most 2^31 occurrences
// [t0, t1) at a time and slots are relative to t0).
template <uint32_t kShift>
__global__ void sweep_init_kernel(const uint64_t* __restrict__ l, const uint64_t* __restrict__ out_off, uint64_t n_pat, uint64_t t0, uint64_t total,
                                  uint64_t* __restrict__ val)
{
    constexpr uint32_t kPer = 8;                           // elements per thread: one list lookup per 2048 elements
    __shared__ uint64_t s_first;
    for (uint64_t base = t0 + (uint64_t)blockIdx.x * 256 * kPer; base < total; base += (uint64_t)gridDim.x * 256 * kPer) {
        if (threadIdx.x == 0) {
            uint64_t lo = 0, hi = n_pat;
            while (hi - lo > 1) { uint64_t mid = (lo + hi) >> 1; if (out_off[mid] <= base) lo = mid; else hi = mid; }
            s_first = lo;
        }
        __syncthreads();
        uint64_t p = s_first;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const uint64_t t = base + i * 256 + threadIdx.x;
            if (t < total) {
                while (out_off[p + 1] <= t) ++p;
                val[t - t0] = ((t - t0) << kShift) | (l[p] + (t - out_off[p]));
            }
        }
        __syncthreads();
    }
}

// The suffix array itself resident in HBM (SA-order sampling with density 1: csa_wt<wt_huff<>, 1, .>, 4 B x n -- 4.3 GB for a 1 GiB text,
// what 288 GB of HBM afford and the reference's CPU index does not): locate is a copy of the SA intervals, csa[i] = sample[i]
// (csa_wt.hpp:335-348 with zero LF steps).  Same list lookup as sweep_init_kernel; reads and writes are coalesced inside a list.
template <typename pos_t, typename sample_t>
__global__ void __launch_bounds__(256) sa_dense_copy_kernel(const sample_t* __restrict__ sa, const uint64_t* __restrict__ l, const uint64_t* __restrict__ out_off,
                                                            uint64_t n_pat, uint64_t total, pos_t* __restrict__ out)
{
    constexpr uint32_t kPer = 8;
    __shared__ uint64_t s_first;
    __shared__ ListStage s_lists;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 * kPer; base < total; base += (uint64_t)gridDim.x * 256 * kPer) {
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t lo = 0, hi = n_pat;
            while (hi - lo > 1) { uint64_t mid = (lo + hi) >> 1; if (out_off[mid] <= base) lo = mid; else hi = mid; }
            s_first = lo;
        }
        __syncthreads();
        uint64_t p = s_first;
        const uint64_t end = base + 256 * kPer < total ? base + 256 * kPer : total;
        if (kStageLists && stage_lists(s_lists, out_off, l, n_pat, p, end)) {
            uint32_t q = 0;
#pragma unroll
            for (uint32_t i = 0; i < kPer; ++i) {
                const uint64_t t = base + i * 256 + threadIdx.x;
                if (t < total) {
                    while (s_lists.off[q + 1] <= t) ++q;
                    out[t] = (pos_t)sa[s_lists.l[q] + (t - s_lists.off[q])];
                }
            }
            continue;
        }
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const uint64_t t = base + i * 256 + threadIdx.x;
            if (t < total) {
                while (out_off[p + 1] <= t) ++p;
                out[t] = (pos_t)sa[l[p] + (t - out_off[p])];
            }
        }
    }
}

__global__ void __launch_bounds__(256) sweep_chunk_lists_kernel(const uint64_t* __restrict__ out_off, uint64_t n_pat, uint64_t t0, uint64_t t1,
                                                                uint32_t* __restrict__ chunk_list)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t base = t0 + c * kSweepChunk;
    if (base >= t1) return;
    uint64_t lo = 0, hi = n_pat;                                                 // last list with out_off[p] <= base
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (out_off[mid] <= base) lo = mid; else hi = mid; }
    chunk_list[c] = (uint32_t)lo;
}

// Records of a trail-sharing sweep -> positions: every element follows its chain of records (element it follows, steps apart) to
// the end, at most kResolveHops hops per round, and replaces its record by what it found -- a position, or a shorter pointer for
// the next round.  Records are single 64-bit words, so a reader sees a valid state of the element it follows whatever that
// one's own thread is doing; chains collapse as the elements ahead finish (measured on C3: 2 + 2 hops per round over four
// rounds 24.5 ms, to the end in one round + one checking round 18.6 ms).
// Round 3 measured three ways around that wall, none of which paid (C3, per batch): (1) not looking at the owner's record when an
// element stops in the first rounds, where the owner is all but certainly still walking: the sweep gains 1 ms, this kernel loses 2.5
// -- the looks are nearly free inside the sweep, which is not request-bound; (2) taking the hops in the order the sweep left the
// stopped elements in (the per-round tails of its buffers, last round first, then first to last): 35.5 instead of 17.7 ms --
// neighbours in SA order are not neighbours in slot order; (3) following the chains on a second stream beside the sweep's late rounds:
// this kernel 18.0 -> 13.3 ms, but the rounds and their partitions slow down by 7 ms: the requests are conserved, not hidden.
#ifndef VLG_RESOLVE_HOPS
#define VLG_RESOLVE_HOPS 4096                 // (64 left 2·10⁵ of C3's 6·10⁸ pointers open -- runs of more than 64 occurrences side by side in the text -- and cost a second pass over all records: 1 ms)
#endif
constexpr uint32_t kResolveHops = VLG_RESOLVE_HOPS;
// A record only ever moves further along its chain, and every hop adds the reach of the record it reads: a round of h hops multiplies
// the reach of every open record by at least h + 1 >= 2, so a chain of at most 2^33 records closes within 34 rounds -- inside the cap
// of 64 rounds in run_locate_sweep for any h >= 1.
static_assert(kResolveHops >= 1, "VLG_RESOLVE_HOPS: at least one hop per round (the reach of a record doubles per round at least)");
// A workgroup takes kResolveChunk CONSECUTIVE records per turn (not every gridDim-th group of 256): consecutive elements of a list
// that read the same symbol in front of them follow consecutive elements of another list, so the lines a wave fetches for its hops
// are the lines the next waves of the same chunk need -- through the CU's own L1 when they belong to one workgroup.
#ifndef VLG_RESOLVE_CHUNK
#define VLG_RESOLVE_CHUNK 4096
#endif
constexpr uint32_t kResolveChunk = VLG_RESOLVE_CHUNK;
static_assert(kResolveChunk >= 256 && kResolveChunk % 256 == 0, "VLG_RESOLVE_CHUNK: whole turns of the 256-thread workgroup");
// The first pass, regrouped.  The 64 consecutive elements a wave holds have ~20 different symbols in front of them, so the records they
// follow lie in ~20 other lists, three side by side in each: ~40 lines per wave-wide hop (VLG_RESOLVE_STATS).  Elements with the SAME
// symbol in front follow CONSECUTIVE records (LF restricted to a symbol is monotone), so a workgroup sorts its kGroupChunk records by that
// symbol (front[]: written in round 0 for the elements that stopped on their first step -- six in ten on C3, nine in ten on C4; a counting
// sort in LDS, the kernel's VALU is idle) and takes the hops in that order: the first hop of a wave reads 8 lines.  Results are staged in
// LDS and written back in record order, coalesced.  (Measured, round 4: chunks of 1024 / 2048 / 4096 records -- C3 16.7 / 16.9 / 22.9 ms, C4
// 118 / 109 / 145 ms: the kernel needs its waves; a second, stable regrouping by the symbol in front of the OWNER for the second hop -- rocPRIM's
// match ranking twice per chunk -- 17.4 vs 17.2 ms: not kept.)
#ifndef VLG_GROUP_CHUNK
#define VLG_GROUP_CHUNK 2048
#endif
constexpr uint32_t kGroupChunk = VLG_GROUP_CHUNK;
static_assert(kGroupChunk >= 256 && kGroupChunk % 256 == 0, "VLG_GROUP_CHUNK: kGroupChunk / 256 records per thread");
static_assert(kGroupChunk <= 65536, "VLG_GROUP_CHUNK: s_idx holds a record's place in the chunk in 16 bits");
static_assert(kGroupChunk * (8 + 2) + 258 * 4 <= 160 * 1024, "VLG_GROUP_CHUNK: s_rec + s_idx + s_bin must fit the 160 KiB of LDS a gfx950 workgroup may take");
template <typename pos_t, bool kWide>
__global__ void __launch_bounds__(256) trail_resolve_grouped_kernel(uint64_t* __restrict__ rec, uint64_t count, pos_t* __restrict__ out,
                                                                    const uint8_t* __restrict__ front, unsigned long long* __restrict__ n_open)
{
    constexpr uint32_t kShift = kWide ? 33 : 32, kPer = kGroupChunk / 256;
    constexpr uint64_t kLow = (1ull << kShift) - 1;
    __shared__ uint64_t s_rec[kGroupChunk];
    __shared__ uint16_t s_idx[kGroupChunk];
    __shared__ uint32_t s_bin[258];
    uint32_t open = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kGroupChunk; base < count; base += (uint64_t)gridDim.x * kGroupChunk) {
        const uint32_t n = (uint32_t)(count - base < kGroupChunk ? count - base : kGroupChunk);
        for (uint32_t j = threadIdx.x; j < 258; j += 256) s_bin[j] = 0;
        __syncthreads();
        uint32_t grp[kPer], arr[kPer];
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256 * k;
            grp[k] = 257; arr[k] = 0;
            if (e < n) {
                const uint64_t r = rec[base + e];
                s_rec[e] = r;
                grp[k] = (r >> kShift) ? (uint32_t)front[base + e] : 256u;       // positions (nothing to follow) stand last
                arr[k] = atomicAdd(&s_bin[grp[k]], 1u);
            }
        }
        __syncthreads();
        {   // exclusive scan of the 257 counters (one wave does it: 5 per lane)
            if (threadIdx.x < 64) {
                uint32_t v[5], sum = 0;
#pragma unroll
                for (uint32_t i = 0; i < 5; ++i) { const uint32_t b = threadIdx.x * 5 + i; v[i] = b < 257 ? s_bin[b] : 0; sum += v[i]; }
                uint32_t incl = sum;
                for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if ((int)threadIdx.x >= o) incl += u; }
                uint32_t run = incl - sum;
#pragma unroll
                for (uint32_t i = 0; i < 5; ++i) { const uint32_t b = threadIdx.x * 5 + i; if (b < 257) s_bin[b] = run; run += v[i]; }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256 * k;
            if (e < n) s_idx[s_bin[grp[k]] + arr[k]] = (uint16_t)e;
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t p = threadIdx.x + 256 * k;
            if (p < n) {
                const uint32_t e = s_idx[p];
                uint64_t r = s_rec[e];
                if (r >> kShift) {
                    for (uint32_t h = 0; h < kResolveHops && (r >> kShift); ++h) {
                        const uint64_t ro = rec[r & kLow];
                        const uint64_t delta = r >> kShift;
                        r = (ro >> kShift) == 0 ? ro + delta : ro + (delta << kShift);
                    }
                    s_rec[e] = r;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t e = threadIdx.x + 256 * k;
            if (e < n) {
                const uint64_t r = s_rec[e];
                rec[base + e] = r;
                if ((r >> kShift) == 0) out[base + e] = (pos_t)r;
                else ++open;
            }
        }
        __syncthreads();
    }
    unsigned long long v[1] = {open};
    unsigned long long* const dst[1] = {n_open};
    block_add<1>(v, dst);
}

template <typename pos_t, bool kWide>
__global__ void __launch_bounds__(256) trail_resolve_kernel(uint64_t* __restrict__ rec, uint64_t count, pos_t* __restrict__ out,
                                                            unsigned long long* __restrict__ n_open, uint32_t round, bool diag)
{
    constexpr uint32_t kShift = kWide ? 33 : 32;
    constexpr uint64_t kLow = (1ull << kShift) - 1;
    uint32_t open = 0;
    unsigned long long n_hops = 0, n_lines = 0, n_ptr = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kResolveChunk; base < count; base += (uint64_t)gridDim.x * kResolveChunk) {
        const uint64_t end = base + kResolveChunk < count ? base + kResolveChunk : count;
        for (uint64_t e = base + threadIdx.x; e < end; e += 256) {
            uint64_t r = rec[e];
            if (r >> kShift) {
                ++n_ptr;
                for (uint32_t h = 0; h < kResolveHops && (r >> kShift); ++h) {
                    if (diag) {                                               // hops, and distinct 64-byte lines per wave-wide hop
                        ++n_hops;
                        const uint64_t line = (r & kLow) >> 3;
                        bool first = true;
                        const unsigned long long act = __ballot(true);
                        for (int o = 1; o < 64; ++o) {
                            const int src = (int)((threadIdx.x & 63) - o);
                            const uint64_t other = __shfl(line, src & 63);
                            if (src >= 0 && ((act >> src) & 1) && other == line) first = false;
                        }
                        if (first) ++n_lines;
                    }
                    const uint64_t ro = rec[r & kLow];
                    const uint64_t delta = r >> kShift;
                    r = (ro >> kShift) == 0 ? ro + delta : ro + (delta << kShift);
                }
                rec[e] = r;
                if ((r >> kShift) == 0) out[e] = (pos_t)r;
                else ++open;
            } else if (round == 0) {
                out[e] = (pos_t)r;                                                // elements that never followed anyone
            }
        }
    }
    if (diag) {
        unsigned long long v[4] = {open, n_hops, n_lines, n_ptr};
        unsigned long long* const dst[4] = {n_open, n_open + 1, n_open + 2, n_open + 3};
        block_add<4>(v, dst);
        return;
    }
    unsigned long long v[1] = {open};
    unsigned long long* const dst[1] = {n_open};
    block_add<1>(v, dst);
}

// =============================================================================================
// K3u: locate by UNSAMPLING the suffix array (dense batches).
//
// csa[i] walks LF from i to the next sampled index (csa_wt.hpp:335-348).  Trail sharing (above) already lets the walks of one batch
// share their steps; when a batch asks for a large part of all text positions (BASELINE configs 3 and 4: 60 % of them) the limit of
// that idea is cheaper still: start ONE walker at every SA sample (i = d j, SA[i] = samples[j]) and let it walk LF until it stands on
// the next sampled index, writing SA[LF(i)] = SA[i] - 1 on every step (suffix_array_helper.hpp:336-349).  The walks are disjoint
// and cover every SA index exactly once: n LF steps whatever the batch holds, no trail table (8 B x n), no records, no pointer
// jumping afterwards -- the occurrence lists are then plain copies of SA intervals (sa_dense_copy_kernel).  Everything is recomputed
// from the index's samples for every batch; nothing survives the call.  The walkers are kept in ascending SA-index order exactly as
// in the sorted sweep (stable partition by the symbol read), so neighbouring lanes read neighbouring super-blocks.
// Element words: narrow  val = SA value << 32 | SA index,  key = symbol;
//                wide    val = (SA value & 2^31 - 1) << 33 | SA index (33 bits),  key = symbol | (bit 31 of the SA value) << 15
// (a wide index has n <= 2^32 + 1 here, so every value a walker WRITES is a text position < 2^32: only the sentinel suffix's own
// sample, SA[0] = n - 1, can be 2^32, and it is never written through a walker nor part of a pattern's interval).
// =============================================================================================
constexpr uint16_t kUnsampleDead = 0x7FFFu;                   // key of a walker that has arrived (sorts behind every symbol)

template <bool kWide> struct WalkerWord;
template <> struct WalkerWord<false> {
    static __device__ __forceinline__ void unpack(uint64_t w, uint16_t, uint64_t& i, uint32_t& v) { i = w & 0xFFFFFFFFull; v = (uint32_t)(w >> 32); }
    static __device__ __forceinline__ uint64_t word(uint64_t i, uint32_t v) { return ((uint64_t)v << 32) | i; }
    static __device__ __forceinline__ uint16_t key(uint32_t c, uint32_t) { return (uint16_t)c; }
};
template <> struct WalkerWord<true> {
    static __device__ __forceinline__ void unpack(uint64_t w, uint16_t k, uint64_t& i, uint32_t& v)
    {
        i = w & ((1ull << 33) - 1);
        v = (uint32_t)(w >> 33) | ((uint32_t)(k >> 15) << 31);
    }
    static __device__ __forceinline__ uint64_t word(uint64_t i, uint32_t v) { return ((uint64_t)(v & 0x7FFFFFFFu) << 33) | i; }
    static __device__ __forceinline__ uint16_t key(uint32_t c, uint32_t v) { return (uint16_t)(c | ((v >> 31) << 15)); }
};

// kFirst: round 0 -- element e is sample e (no words read); otherwise the walkers [0, count) of val / key, dead ones skipped (the
// host may pass a count from a few rounds ago: the dead are at the end, the partition keeps them there).
template <class BV, bool kWide, bool kFirst>
__global__ void __launch_bounds__(256) unsample_step_kernel(IndexView iv, uint64_t* __restrict__ val, uint16_t* __restrict__ key, uint64_t count,
                                                            uint32_t* __restrict__ sa, unsigned long long* __restrict__ stats /* lf, levels */,
                                                            unsigned long long* __restrict__ n_done)
{
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    const ByteWalk<BV, kWide> walk{iv, s};
    using sample_t = typename std::conditional<kWide, uint64_t, uint32_t>::type;
    const sample_t* __restrict__ samples = reinterpret_cast<const sample_t*>(iv.samples);
    const uint32_t dens = iv.dens, dmask = dens - 1;
    const bool pow2 = (dens & dmask) == 0;
    uint32_t n_lv = 0, n_lf = 0, n_fin = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t i;
        uint32_t v;
        if (kFirst) {
            i = e * dens;
            const uint64_t sv = (uint64_t)samples[e];
            v = (uint32_t)sv;                                // (2^32 for the sentinel suffix of a wide index: v - 1 below is still right)
            sa[i] = v;
            if (iv.sigma == 1) { key[e] = kUnsampleDead; ++n_fin; continue; }      // degenerate: only the sentinel exists
        } else {
            const uint16_t k = key[e];
            if ((k & 0x7FFFu) == kUnsampleDead) continue;
            WalkerWord<kWide>::unpack(val[e], k, i, v);
        }
        uint32_t c;
        const uint64_t i2 = walk.lf(i, c, n_lv);
        ++n_lf;
        const uint32_t v2 = (!kWide && v == 0) ? (uint32_t)(iv.n - 1) : v - 1;      // SA[LF(i)] = SA[i] - 1 (mod n): csa_wt.hpp:343-347
        const bool arrived = pow2 ? ((i2 & dmask) == 0) : (i2 % dens == 0);
        if (arrived) { key[e] = kUnsampleDead; ++n_fin; }
        else {
            sa[i2] = v2;
            val[e] = WalkerWord<kWide>::word(i2, v2);
            key[e] = WalkerWord<kWide>::key(c, v2);
        }
    }
    unsigned long long v3[3] = {n_lf, n_lv, n_fin};
    unsigned long long* const dst[3] = {&stats[0], &stats[1], n_done};
    block_add<3>(v3, dst);
}

// The last walkers (how long a walk is, is geometrically distributed: a few are still on their way after 100 rounds) finish without
// being sorted any more, lane by lane with refill as in locate_kernel (WaveSlice): a wave owns a slice of the walkers, a lane that
// arrives pulls the next one.
template <class BV, bool kWide>
__global__ void __launch_bounds__(256) unsample_tail_kernel(IndexView iv, const uint64_t* __restrict__ val, const uint16_t* __restrict__ key, uint64_t total,
                                                            uint32_t per_wave, uint32_t* __restrict__ sa, unsigned long long* __restrict__ stats)
{
    using Walk = ByteWalk<BV, kWide>;
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    const Walk walk{iv, s};
    WaveSlice slice(total, per_wave);
    const uint32_t dens = iv.dens, dmask = dens - 1;
    const bool pow2 = (dens & dmask) == 0;
    uint64_t i = 0;
    uint32_t v = 0;
    typename Walk::Cursor node;
    bool active = false, need = true;
    uint32_t n_lf = 0, n_lv = 0;
    for (;;) {
        slice.refill(need, [&](uint64_t cand) {
            active = false;
            if (cand < slice.end) {
                const uint16_t k = key[cand];
                if ((k & 0x7FFFu) != kUnsampleDead) { WalkerWord<kWide>::unpack(val[cand], k, i, v); node = typename Walk::Cursor(); active = true; }
            }
            need = !active && cand < slice.end;              // a dead walker: take another one next turn
        });
        if (!__any(active) && !__any(need)) break;
        uint32_t c;
        if (active && walk.level(node, i, c, n_lv)) {
            v = (!kWide && v == 0) ? (uint32_t)(iv.n - 1) : v - 1;
            ++n_lf;
            const bool arrived = pow2 ? ((i & dmask) == 0) : (i % dens == 0);
            if (arrived) { need = true; active = false; }
            else sa[i] = v;
        }
    }
    if (stats) {
        unsigned long long v2[2] = {n_lf, n_lv};
        unsigned long long* const dst[2] = {&stats[0], &stats[1]};
        block_add<2>(v2, dst);
    }
}

// ISA samples (csa_sampling_strategy.hpp:626-642: isa_sample[SA[i] / d'] = i for every i with SA[i] % d' == 0), computed from the
// index alone: a lane starts at one SA sample (i, SA[i]) and walks LF -- (LF(i), SA[i] - 1) -- until the next sampled
// index, so every SA index is visited exactly once and every text position passes by with its SA index.
template <class BV, typename pos_t, typename out_t>
__global__ void __launch_bounds__(256) isa_samples_kernel(IndexView iv, uint32_t inv_dens, out_t* __restrict__ out)
{
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    const ByteWalk<BV, true> walk{iv, s};                    // (node-relative positions in 64 bits whatever the width of the samples)
    const pos_t* samples = reinterpret_cast<const pos_t*>(iv.samples);
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < iv.n_samples; j += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t i = j * iv.dens, v = samples[j];
        do {
            if (v % inv_dens == 0) out[v / inv_dens] = (out_t)i;
            uint32_t c, n_lv = 0;
            i = walk.lf(i, c, n_lv);
            v = v ? v - 1 : iv.n - 1;
        } while (i % iv.dens);
    }
}

// ---- text access (extract.hpp): sdsl::extract and csa.isa[i] on the Huffman-shaped tree -----------------------------------------------
template <class BV, bool kWide, typename isa_t>
__global__ void __launch_bounds__(256) extract_kernel(IndexView iv, ExtractJob job, const isa_t* __restrict__ isa, const uint8_t* __restrict__ comp2char,
                                                      uint8_t* __restrict__ out)
{
    __shared__ WalkLds<BV> s;
    __shared__ uint8_t c2c[256];
    c2c[threadIdx.x] = comp2char[threadIdx.x];             // (256 threads; stage_walk's barrier covers it)
    stage_walk(s, iv);
    extract_segments(job, isa, out, ByteWalk<BV, kWide>{iv, s, c2c});
}

template <class BV, bool kWide, typename isa_t>
__global__ void __launch_bounds__(256) isa_kernel(IndexView iv, uint32_t d, const isa_t* __restrict__ isa, const uint64_t* __restrict__ p,
                                                  uint64_t* __restrict__ out, uint64_t count, unsigned long long* __restrict__ bad)
{
    __shared__ WalkLds<BV> s;
    stage_walk(s, iv);
    isa_queries(p, out, count, iv.n, d, isa, ByteWalk<BV, kWide>{iv, s}, bad);
}

// comp2char of a byte index from its char2comp (comp 0 is the sentinel; absent characters map to 0 and are skipped)
__global__ void comp2char_kernel(const uint8_t* __restrict__ char2comp, uint8_t* __restrict__ c2c)
{
    const uint32_t ch = threadIdx.x, c = char2comp[ch];
    if (ch == 0 || c != 0) c2c[c] = (uint8_t)ch;
}

// segment counts of the ranges of an extract batch (a bad range counts 0 and raises *bad): seg[r] = e / d - b / d + 1, seg[n_ranges] = 0
__global__ void extract_check_kernel(const uint64_t* __restrict__ begin, const uint64_t* __restrict__ end, const uint64_t* __restrict__ out_off,
                                     uint64_t n_ranges, uint64_t n, uint64_t total, uint32_t d, uint64_t* __restrict__ seg,
                                     unsigned long long* __restrict__ bad)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_ranges; r += (uint64_t)gridDim.x * blockDim.x) {
        if (r == n_ranges) { seg[r] = 0; continue; }
        const uint64_t b = begin[r], e = end[r], o = out_off[r];
        const bool ok = b <= e && e < n && o <= total && e - b + 1 <= total - o;
        seg[r] = ok ? e / d - b / d + 1 : 0;
        if (!ok) atomicAdd(bad, 1ull);
    }
}

template <typename pos_t>
__global__ void widen_kernel(const pos_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t count)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) out[j] = in[j];
}
template <typename pos_t>
__global__ void narrow_kernel(const uint64_t* __restrict__ in, pos_t* __restrict__ out, uint64_t count)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) out[j] = (pos_t)in[j];
}

// the byte index's sampling policy: sample words as wide as its SA indices
template <bool kWide, bool kTextOrder>
using ByteSampling = typename std::conditional<kTextOrder, TextOrderSampling<typename std::conditional<kWide, uint64_t, uint32_t>::type>,
                                               SaOrderSampling<typename std::conditional<kWide, uint64_t, uint32_t>::type>>::type;

}  // namespace

namespace vlg {

vlg_status launch_backward_search(const IndexView& iv, const uint8_t* d_blob, const uint64_t* d_off, uint64_t n_pat, uint64_t* d_l,
                                  uint64_t* d_r, unsigned long long* d_stat_levels, hipStream_t stream)
{
    if (!n_pat) return VLG_OK;
    return on_bv(iv.bv_kind, [&](auto bv) {
        return launch(backward_search_kernel<tag_t<decltype(bv)>>, launch_grid(n_pat, 4096), stream, iv, d_blob, d_off, n_pat, d_l, d_r, d_stat_levels);
    });
}

vlg_status launch_branching_search(const IndexView& iv, bool budget, const uint8_t* d_masks, const uint64_t* d_task, uint64_t n_tasks, uint32_t cap,
                                   uint64_t* d_frontier, uint32_t* d_count, unsigned long long* d_stat_levels, hipStream_t stream)
{
    if (!n_tasks) return VLG_OK;
    if (!cap || cap > kClassIntervalsMax) return fail(VLG_E_INTERNAL, std::string(budget ? "approximate" : "class") + " search: frontier cap out of range");
    // one wave per task, four to a workgroup; enough workgroups to fill the device, the rest of the tasks in turns
    const dim3 grid((uint32_t)std::min<uint64_t>((n_tasks + 3) / 4, 16384));
    return on_bv(iv.bv_kind, [&](auto bv) {
        const auto go = [&](auto kernel) {
            return launch(kernel, grid, stream, iv, d_masks, d_task, n_tasks, cap, reinterpret_cast<ulonglong2*>(d_frontier), d_count, d_stat_levels);
        };
        return budget ? go(branching_search_kernel<tag_t<decltype(bv)>, true>) : go(branching_search_kernel<tag_t<decltype(bv)>, false>);
    });
}

template <typename pos_t>
vlg_status launch_expand(const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, pos_t* d_io, uint32_t* d_seg,
                         hipStream_t stream)
{
    if (!total) return VLG_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(expand_kernel<pos_t>), launch_grid(total, 32768), dim3(256), 0, stream, d_l, d_out_off, n_pat,
                       total, d_io, d_seg);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}
template vlg_status launch_expand<uint32_t>(const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint32_t*, uint32_t*, hipStream_t);
template vlg_status launch_expand<uint64_t>(const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint64_t*, uint32_t*, hipStream_t);

template <typename pos_t>
vlg_status launch_locate(const IndexView& iv, pos_t* d_io, uint64_t total, unsigned long long* d_stats, hipStream_t stream)
{
    if (!total) return VLG_OK;
    const LocateSlices sl = locate_slices(total);
    if (iv.sample_bytes != sizeof(pos_t)) return fail(VLG_E_INTERNAL, "locate: sample width does not match the instantiation");
    constexpr bool kWide = sizeof(pos_t) == 8;
    return on_byte_walk<kWide>(iv, [&](auto walk) { return on_flag(shape(iv).text_order, [&](auto to) {
        // (in place: no words, no records -- the tail mode's parameters are empty)
        return launch(locate_kernel<tag_t<decltype(walk)>, ByteSampling<kWide, decltype(to)::value>, pos_t, false, kWide>, dim3(sl.blocks), stream, iv, d_io,
                      total, sl.per_wave, d_stats, nullptr, 0u, nullptr, 0ull, nullptr);
    }); });
}
template vlg_status launch_locate<uint32_t>(const IndexView&, uint32_t*, uint64_t, unsigned long long*, hipStream_t);
template vlg_status launch_locate<uint64_t>(const IndexView&, uint64_t*, uint64_t, unsigned long long*, hipStream_t);


size_t sweep_temp_bytes(uint64_t total, uint32_t sigma, hipStream_t stream)
{
    size_t tb = 0;
    rocprim::double_buffer<uint16_t> k(nullptr, nullptr);
    rocprim::double_buffer<uint64_t> v(nullptr, nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, tb, k, v, total, 0, bit_width64(sigma), stream);   // the sweep's own two buffers alternate
    return tb;
}

void launch_sweep_chunk_lists(const uint64_t* d_out_off, uint64_t n_pat, uint64_t t0, uint64_t t1, uint32_t* chunk_list, hipStream_t stream)
{
    const uint64_t chunks = (t1 - t0 + kSweepChunk - 1) / kSweepChunk;
    if (!chunks) return;
    hipLaunchKernelGGL(sweep_chunk_lists_kernel, dim3((uint32_t)((chunks + 255) / 256)), dim3(256), 0, stream, d_out_off, n_pat, t0, t1, chunk_list);
}

struct SweepSwitches { bool grouped_resolve, lookahead, resolve_stats; };      // the runtime switches of a sweep, read once per run
static bool env_is(const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; }

// What the sweep and K3u share while they run: the val / key pair as it stands, the partition that swaps it, and the host hook.
struct SweepState {
    SweepScratch buf;                                   // val[0] / key[0]: the elements as they stand
    hipStream_t stream; LaunchTimer* timer;
    const std::function<vlg_status()>* hook;            // null once it has run
    template <typename pos_t> explicit SweepState(const SweepJob<pos_t>& job) : buf(job.scratch), stream(job.stream), timer(job.timer), hook(job.while_first_step) {}
    // the stable partition of val[0] / key[0] [0, count) by symbol; the sorted side becomes val[0] / key[0]
    vlg_status partition(uint64_t count, unsigned key_bits)
    {
        size_t tb = buf.temp_bytes;
        rocprim::double_buffer<uint16_t> dk(buf.key[0], buf.key[1]);
        rocprim::double_buffer<uint64_t> dv(buf.val[0], buf.val[1]);
        const auto sort = [&]() -> vlg_status { VLG_HIP_TRY(rocprim::radix_sort_pairs(buf.temp, tb, dk, dv, count, 0, key_bits, stream)); return VLG_OK; };
        if (vlg_status s = timed(timer, 1, kSweepScratchPerElem * count, sort)) return s;      // key + element read once and written once
        buf.key[0] = dk.current(); buf.key[1] = dk.alternate();
        buf.val[0] = dv.current(); buf.val[1] = dv.alternate();
        return VLG_OK;
    }
    // the host work to do while the first step runs: where it is first due, and never again
    vlg_status hook_once() { const auto* due = hook; hook = nullptr; return due ? (*due)() : VLG_OK; }
};

// The sweep's driver: rounds, partitions, records and the stragglers' slices for ANY index that can launch the three kernels of
// SweepKernels (kernels.hpp) -- the byte index below, the integer-alphabet index in int_index.hpp.
template <typename pos_t, bool kWide>
struct SweepRun : SweepState {
    static constexpr uint32_t kShift = kWide ? 33 : 32;
    const SweepKernels& K; const SweepJob<pos_t>& job;
    const SweepSwitches sw{!env_is("VLG_RESOLVE_GROUPED", '0'), !env_is("VLG_SWEEP_LOOKAHEAD", '0'), env_is("VLG_RESOLVE_STATS", '1')};
    // bits of the keys 0..sigma (sigma = finished, sorts last), and of 0..sigma - 1 where no finished element is sorted
    const unsigned bits = bit_width64(K.sigma), live_bits = std::max(1u, bit_width64(K.sigma ? K.sigma - 1 : 0));
    bool front_valid = K.front != nullptr && sw.grouped_resolve;       // front[] holds what the grouped resolve reads
    // the sweep [t0, t1) under way: `alive` elements still walk, in val[0] / key[0] [0, alive), after `step` rounds
    uint64_t t0 = 0, t1 = 0, alive = 0; uint32_t step = 0; bool fused_first = false;
    SweepRun(const SweepKernels& K, const SweepJob<pos_t>& job) : SweepState(job), K(K), job(job) {}
    pos_t* out() const { return job.d_out + t0; }
    vlg_status run()
    {
        if (vlg_status s = check()) return s;
        if (vlg_status s = build_member()) return s;
        for (t0 = 0; t0 < job.total; t0 += sweep_batch_max<kWide>()) {
            t1 = std::min(job.total, t0 + sweep_batch_max<kWide>());
            if (vlg_status s = seed()) return s;
            while (alive > job.tail_threshold && step < 0xFFFFFFu)
                if (vlg_status s = round(fused_first && step == 0)) return s;
            if (vlg_status s = stragglers()) return s;
        }
        if (vlg_status s = hook_once()) return s;
        return job.member ? resolve() : VLG_OK;
    }
    vlg_status check()
    {
        if (K.n > (1ull << kShift)) return fail(VLG_E_UNSUPPORTED, "sorted sweep: text too long for the packed position");
        if (sizeof(pos_t) == 4 && K.n > (1ull << 32) + 1) return fail(VLG_E_INTERNAL, "sorted sweep: positions do not fit 32 bits");
        if (K.sigma >= 0xFFFFu) return fail(VLG_E_INTERNAL, "sorted sweep: alphabet too large for the 16-bit partition key");
        if (job.member && job.total > 0xFFFFFF00ull) return fail(VLG_E_INTERNAL, "member bit-vector: slots need 32 bits");
        return VLG_OK;
    }
    vlg_status build_member()
    {
        if (!job.member) return VLG_OK;
        const auto build = [&] { return launch(member_build_kernel, launch_grid(member_blocks(K.n), 16384), stream, job.d_l, job.d_out_off, job.n_member_lists, member_blocks(K.n), job.member); };
        if (vlg_status s = timed(timer, 0, 0, build)) return s;
        // more than one sweep: an element may stop at an element of a LATER sweep, whose record must read "still walking" until then
        if (job.total > sweep_batch_max<kWide>()) VLG_HIP_TRY(hipMemsetAsync(job.rec, 0xFF, job.total * 8, stream));
        return VLG_OK;
    }
    // a sweep too short for a single round hands its words to the stragglers' kernel; rounds start with the fused first round, which makes them itself
    vlg_status seed()
    {
        alive = t1 - t0; step = 0;
        fused_first = alive > job.tail_threshold;
        if (fused_first) return VLG_OK;
        front_valid = false;                   // (front[] is written by the fused first round only)
        if (job.member) VLG_HIP_TRY(hipMemsetAsync(job.rec + t0, 0xFF, alive * 8, stream));     // "still walking" (the first-round kernel writes it itself)
        return launch(sweep_init_kernel<kShift>, launch_grid((alive + 7) / 8, 32768), stream, job.d_l, job.d_out_off, job.n_lists, t0, t1, buf.val[0]);
    }
    vlg_status round(bool first)
    {
        const bool compact = first && job.h_round != nullptr;        // round 0 leaves its survivors alone, densely (sweep_kernels.hpp: commit_turn)
        VLG_HIP_TRY(hipMemsetAsync(buf.control, 0, sweep_control_bytes(alive, compact), stream));
        if (vlg_status ks = timed(timer, 0, 0, [&] {
                return first ? K.first(t0, t1, buf.val[0], buf.key[0], out(), buf.control, job.member, job.rec, sw.lookahead, buf.chunk_list(), compact)      // round 0 makes the elements' words itself
                             : K.step(buf.val[0], buf.key[0], alive, step, out(), buf.control, job.member, job.rec, t0, sw.lookahead && fused_first && step == 1);
            })) return ks;
        // not compacting: the partition carries the finished elements (key = sigma) into its last bucket, and runs before `done` is known
        if (!compact) if (vlg_status ps = partition(alive, bits)) return ps;
        unsigned long long done_here[2] = {0, 0};
        unsigned long long* done = compact ? job.h_round : done_here;
        VLG_HIP_TRY(hipMemcpyAsync(done, buf.control, compact ? 16 : 8, hipMemcpyDeviceToHost, stream));
        if (vlg_status hs = hook_once()) return hs;
        VLG_HIP_TRY(hipStreamSynchronize(stream));
        if (compact && done[kSweepStalled]) return fail(VLG_E_INTERNAL, "sweep compaction stalled");
        if (done[kSweepDone] > alive) return fail(VLG_E_INTERNAL, "locate sweep: more elements finished than were walking");
        alive -= done[kSweepDone];
        // compacting: the round has left its survivors, and nothing else, in val[0] / key[0] [0, alive); the next round follows the
        // partition without another round trip (the stragglers' kernel takes its elements in any order: no partition for it)
        if (compact && alive > job.tail_threshold) if (vlg_status ps = partition(alive, live_bits)) return ps;
        ++step;
        if (step > 1u << 20) return fail(VLG_E_INTERNAL, "locate sweep did not converge");
        return VLG_OK;
    }
    vlg_status stragglers()
    {
        if (!alive) return VLG_OK;
        const LocateSlices sl = locate_slices(alive);
        return timed(timer, 0, 0, [&] { return K.tail(out(), alive, sl.per_wave, buf.val[0], step, job.member ? job.rec : nullptr, t0, job.member, sl.blocks); });
    }
    // every element has a record now; jump pointers until all of them are positions
    vlg_status resolve()
    {
        const bool diag = sw.resolve_stats;
        for (uint32_t pass = 0;; ++pass) {
            VLG_HIP_TRY(hipMemsetAsync(buf.control, 0, diag ? 32 : 8, stream));
            if (vlg_status ks = timed(timer, 2, pass == 0 ? job.total * (8ull + sizeof(pos_t)) : 0, [&] {     // every record read, every position written
                if (pass == 0 && front_valid && !diag)
                    return launch(trail_resolve_grouped_kernel<pos_t, kWide>, dim3((uint32_t)std::min<uint64_t>((job.total + kGroupChunk - 1) / kGroupChunk, 1u << 20)), stream,
                                  job.rec, job.total, job.d_out, K.front, buf.control);
                return launch(trail_resolve_kernel<pos_t, kWide>, dim3((uint32_t)std::min<uint64_t>((job.total + kResolveChunk - 1) / kResolveChunk, 65536)), stream, job.rec,
                              job.total, job.d_out, buf.control, pass, diag);
            })) return ks;
            unsigned long long open = 0;
            VLG_HIP_TRY(hipMemcpyAsync(&open, buf.control, 8, hipMemcpyDeviceToHost, stream));
            VLG_HIP_TRY(hipStreamSynchronize(stream));
            if (diag) if (vlg_status s = trace_resolve(pass)) return s;
            if (!open) break;
            if (pass > 64) return fail(VLG_E_INTERNAL, "trail records did not resolve");
        }
        return VLG_OK;
    }
    // VLG_RESOLVE_STATS=1: what the pass's kernel counted behind the counter
    vlg_status trace_resolve(uint32_t pass)
    {
        unsigned long long c[4] = {0, 0, 0, 0};
        VLG_HIP_TRY(hipMemcpy(c, buf.control, 32, hipMemcpyDeviceToHost));
        fprintf(stderr, "[vlg resolve] round %u: %llu records, %llu pointers, %llu hops, %llu distinct lines (per wave-wide hop), %llu still open\n", pass,
                (unsigned long long)job.total, c[3], c[1], c[2], c[0]);
        return VLG_OK;
    }
};
template <typename pos_t, bool kWide>
vlg_status run_locate_sweep(const SweepKernels& K, const SweepJob<pos_t>& job) { return SweepRun<pos_t, kWide>(K, job).run(); }
template vlg_status run_locate_sweep<uint32_t, false>(const SweepKernels&, const SweepJob<uint32_t>&);

// the byte index (IndexView: Huffman-shaped tree, plain or rrr bit-vectors, either sampling) in the sweep
template <typename pos_t, bool kWide>
vlg_status launch_locate_sweep(const IndexView& iv, const SweepJob<pos_t>& job)
{
    if (iv.sample_bytes != (kWide ? 8u : 4u)) return fail(VLG_E_INTERNAL, "sorted sweep: sample width does not match the instantiation");
    const bool text_order = shape(iv).text_order;
    if (iv.dens == 1 && !text_order && job.total) {
        using sample_t = typename std::conditional<kWide, uint64_t, uint32_t>::type;
        return sweep_dense_copy(job, [&] {
            return launch(sa_dense_copy_kernel<pos_t, sample_t>, launch_grid((job.total + 7) / 8, 32768), job.stream, reinterpret_cast<const sample_t*>(iv.samples), job.d_l,
                          job.d_out_off, job.n_lists, job.total, job.d_out);
        });
    }
    return on_byte_walk<kWide>(iv, [&](auto walk) { return on_flag(text_order, [&](auto to) {
        return run_locate_sweep<pos_t, kWide>(bind_sweep<tag_t<decltype(walk)>, ByteSampling<kWide, decltype(to)::value>, pos_t, kWide>(iv, job, job.rec ? job.front : nullptr), job);
    }); });
}
// K3u (above): the whole suffix array into sa_full (n words of 32 bits), then the SA intervals of the lists into d_out.  Rounds are enqueued kUnsampleSync
// at a time: the count of walkers still on their way is read back only then (the kernels skip the ones that have arrived, which the partition keeps at the end).
constexpr uint32_t kUnsampleSync = 4;
template <bool kWide>
vlg_status launch_unsample(const IndexView& iv, const SweepJob<uint32_t>& job, uint32_t* sa_full, unsigned long long* h_done)
{
    SweepState st(job);
    const hipStream_t stream = job.stream;
    if (iv.sampling != kSamplingSaOrder || iv.dens < 2) return fail(VLG_E_INTERNAL, "unsampling needs SA-order samples of density >= 2");
    if (iv.sample_bytes != (kWide ? 8u : 4u)) return fail(VLG_E_INTERNAL, "unsampling: sample width does not match the instantiation");
    if (iv.n > (1ull << 32) + 1 || (!kWide && iv.n > (1ull << 32))) return fail(VLG_E_UNSUPPORTED, "unsampling: text too long for 32-bit positions");
    if (iv.sigma >= 0x7FFFu) return fail(VLG_E_INTERNAL, "unsampling: alphabet too large for the key");
    const unsigned bits = bit_width64(iv.sigma);            // keys 0 .. sigma - 1, dead = all ones in these bits too (sorts last)
    uint64_t alive = iv.n_samples;
    // one round of the walkers val[0] / key[0] [0, alive) as they stand when it is called; the first one makes their words
    const auto step_round = [&](bool first) {
        return timed(st.timer, 0, 0, [&] { return on_bv(iv.bv_kind, [&](auto bv) { return on_flag(first, [&](auto f) {
            return launch(unsample_step_kernel<tag_t<decltype(bv)>, kWide, decltype(f)::value>, launch_grid(alive, 8192), stream, iv, st.buf.val[0], st.buf.key[0], alive,
                          sa_full, job.d_stats, st.buf.control);
        }); }); });
    };
    VLG_HIP_TRY(hipMemsetAsync(st.buf.control, 0, 8, stream));
    uint32_t round = 0;
    while (alive > job.tail_threshold) {
        for (uint32_t r = 0; r < kUnsampleSync; ++r, ++round) {
            if (vlg_status ks = step_round(round == 0)) return ks;
            if (vlg_status ps = st.partition(alive, bits)) return ps;
            if (vlg_status hs = st.hook_once()) return hs;
        }
        VLG_HIP_TRY(hipMemcpyAsync(h_done, st.buf.control, 8, hipMemcpyDeviceToHost, stream));
        VLG_HIP_TRY(hipStreamSynchronize(stream));
        if (*h_done > iv.n_samples) return fail(VLG_E_INTERNAL, "unsampling: more walkers arrived than were started");
        alive = iv.n_samples - *h_done;
        if (round > (1u << 20)) return fail(VLG_E_INTERNAL, "unsampling did not converge");
    }
    if (round == 0 && iv.n_samples) {
        // too few walkers for a single sorted round: round 0 still makes their words (and writes the samples themselves)
        if (vlg_status ks = step_round(true)) return ks;
        ++round;
    }
    if (vlg_status hs = st.hook_once()) return hs;
    if (alive || round == 1) {
        // (after an unsorted round 0 the dead are anywhere: the tail looks at all of them)
        const uint64_t span = round == 1 ? iv.n_samples : alive;
        const LocateSlices sl = locate_slices(span, 64 * 4);
        const vlg_status ks = timed(st.timer, 0, 0, [&] { return on_bv(iv.bv_kind, [&](auto bv) {
            return launch(unsample_tail_kernel<tag_t<decltype(bv)>, kWide>, dim3(sl.blocks), stream, iv, st.buf.val[0], st.buf.key[0], span, sl.per_wave, sa_full, job.d_stats);
        }); });
        if (ks) return ks;
    }
    if (!job.total) return VLG_OK;
    return timed(st.timer, 0, 0, [&] { return launch_sa_dense_copy(sa_full, job.d_l, job.d_out_off, job.n_lists, job.total, job.d_out, stream); });
}
template vlg_status launch_unsample<false>(const IndexView&, const SweepJob<uint32_t>&, uint32_t*, unsigned long long*);
template vlg_status launch_unsample<true>(const IndexView&, const SweepJob<uint32_t>&, uint32_t*, unsigned long long*);

// the copy on its own, for the integer index (int_index.hpp: an SA-order index of density 1 keeps the suffix array as its samples)
vlg_status launch_sa_dense_copy(const uint32_t* sa, const uint64_t* d_l, const uint64_t* d_out_off, uint64_t n_pat, uint64_t total, uint32_t* d_out,
                                hipStream_t stream)
{
    if (!total) return VLG_OK;
    return launch(sa_dense_copy_kernel<uint32_t, uint32_t>, launch_grid((total + 7) / 8, 32768), stream, sa, d_l, d_out_off, n_pat, total, d_out);
}

template vlg_status launch_locate_sweep<uint32_t, false>(const IndexView&, const SweepJob<uint32_t>&);
template vlg_status launch_locate_sweep<uint32_t, true>(const IndexView&, const SweepJob<uint32_t>&);        // n = 2^32 + 1 (BASELINE config 4): 33-bit SA indices, 32-bit text positions
template vlg_status launch_locate_sweep<uint64_t, true>(const IndexView&, const SweepJob<uint64_t>&);

template <typename T>
vlg_status launch_narrow(const uint64_t* d_in, T* d_out, uint64_t count, hipStream_t stream)
{
    if (!count) return VLG_OK;
    return launch(narrow_kernel<T>, launch_grid(count), stream, d_in, d_out, count);
}
template vlg_status launch_narrow<uint32_t>(const uint64_t*, uint32_t*, uint64_t, hipStream_t);
template <typename T>
vlg_status launch_widen(const T* d_in, uint64_t* d_out, uint64_t count, hipStream_t stream)
{
    if (!count) return VLG_OK;
    return launch(widen_kernel<T>, launch_grid(count), stream, d_in, d_out, count);
}
template vlg_status launch_widen<uint32_t>(const uint32_t*, uint64_t*, uint64_t, hipStream_t);

// the build-time constants of this translation unit (vlg_build_constants)
KernelConstants kernel_constants()
{
    return KernelConstants{VLG_RESOLVE_HOPS, VLG_RESOLVE_CHUNK, VLG_GROUP_CHUNK, VLG_STAGE_LISTS, VLG_SWEEP_PAIRS, VLG_SWEEP_CHUNK};
}

}  // namespace vlg

extern "C" vlg_status vlg_wt_rank_batch(const vlg_index* idx, const uint64_t* d_i, const uint8_t* d_c, uint64_t* d_out, uint64_t count,
                                        void* stream)
{
    if (!idx || (count && (!d_i || !d_c || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (idx->is_int) return fail(VLG_E_INVALID, "integer-alphabet index: use vlg_int_rank_batch");
    if (!count) return VLG_OK;
    return on_bv(idx->view.bv_kind, [&](auto bv) {
        return launch(wt_rank_kernel<tag_t<decltype(bv)>>, launch_grid(count, 8192), (hipStream_t)stream, idx->view, d_i, d_c, d_out, count);
    });
}

extern "C" vlg_status vlg_backward_search_batch(const vlg_index* idx, const uint8_t* d_blob, const uint64_t* d_off, uint64_t n_patterns,
                                                uint64_t* d_l, uint64_t* d_r, void* stream)
{
    if (!idx || (n_patterns && (!d_off || !d_l || !d_r))) return fail(VLG_E_INVALID, "null argument");
    // (an integer-alphabet index takes patterns of little-endian uint32_t symbols, offsets in bytes)
    if (idx->is_int) return launch_int_backward_search(idx->iview, d_blob, d_off, n_patterns, d_l, d_r, nullptr, (hipStream_t)stream);
    return launch_backward_search(idx->view, d_blob, d_off, n_patterns, d_l, d_r, nullptr, (hipStream_t)stream);
}

namespace {
// The 32-bit path of vlg_sa_batch and vlg_locate_batch: fill(tmp) puts `count` SA indices into a scratch buffer, they are located in
// place and widened into d_out, and the stream is synchronised before the buffer goes.
template <class Fill>
vlg_status locate_narrow(const vlg_index* idx, uint64_t count, uint64_t* d_out, hipStream_t st, const Fill& fill)
{
    DevBuf tmp_buf;
    VLG_HIP_TRY(tmp_buf.alloc(count * 4));
    uint32_t* tmp = tmp_buf.as<uint32_t>();
    vlg_status s = fill(tmp);
    if (!s) s = idx->is_int ? launch_int_locate(idx->iview, tmp, count, nullptr, st) : launch_locate<uint32_t>(idx->view, tmp, count, nullptr, st);
    if (!s) s = launch_widen<uint32_t>(tmp, d_out, count, st);
    const hipError_t e = hipStreamSynchronize(st);                // (before tmp goes)
    if (s) return s;
    VLG_HIP_TRY(e);
    return VLG_OK;
}
}  // namespace

extern "C" vlg_status vlg_sa_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!idx || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    hipStream_t st = (hipStream_t)stream;
    if (idx->hdr.sample_bytes == 8) {
        if (d_out != d_i) VLG_HIP_TRY(hipMemcpyAsync(d_out, d_i, count * 8, hipMemcpyDeviceToDevice, st));
        return launch_locate<uint64_t>(idx->view, d_out, count, nullptr, st);
    }
    return locate_narrow(idx, count, d_out, st, [&](uint32_t* tmp) { return launch_narrow<uint32_t>(d_i, tmp, count, st); });
}

extern "C" vlg_status vlg_locate_batch(const vlg_index* idx, const uint64_t* d_l, const uint64_t* d_r, const uint64_t* d_out_off,
                                       uint64_t n_patterns, uint64_t total, uint64_t* d_out, void* stream)
{
    (void)d_r;
    if (!idx || (n_patterns && (!d_l || !d_out_off)) || (total && !d_out)) return fail(VLG_E_INVALID, "null argument");
    if (!total) return VLG_OK;
    hipStream_t st = (hipStream_t)stream;
    if (idx->hdr.sample_bytes == 8) {
        if (vlg_status s = launch_expand<uint64_t>(d_l, d_out_off, n_patterns, total, d_out, nullptr, st)) return s;
        return launch_locate<uint64_t>(idx->view, d_out, total, nullptr, st);
    }
    return locate_narrow(idx, total, d_out, st, [&](uint32_t* tmp) { return launch_expand<uint32_t>(d_l, d_out_off, n_patterns, total, tmp, nullptr, st); });
}

namespace {
// ISA samples of an SA-order index into d_out: (n - 1) / inv_dens + 1 entries of isa_sample_bytes(n) bytes
vlg_status isa_samples_device(const vlg_index* idx, uint32_t inv_dens, void* d_out, hipStream_t st)
{
    const uint64_t n = idx->hdr.n;
    if (idx->hdr.sampling != kSamplingSaOrder) return fail(VLG_E_UNSUPPORTED, "ISA samples are computed from an SA-order index");
    const uint64_t count = (n - 1) / inv_dens + 1;
    const uint32_t w = isa_sample_bytes(n);
    VLG_HIP_TRY(hipMemsetAsync(d_out, 0, count * w, st));
    if (idx->is_int)                                               // the walk on the wavelet matrix (int_index.hpp), plain or rrr levels
        return launch_int_isa_samples(idx->iview, inv_dens, (uint32_t*)d_out, st);
    const IndexView& iv = idx->view;
    return on_bv(iv.bv_kind, [&](auto bv) { return on_isa_samples_shape(shape(iv).wide, w, [&](auto pos, auto out) {
        using out_t = tag_t<decltype(out)>;
        return launch(isa_samples_kernel<tag_t<decltype(bv)>, tag_t<decltype(pos)>, out_t>, launch_grid(iv.n_samples, 8192), st, iv, inv_dens, (out_t*)d_out);
    }); });
}
}  // namespace

extern "C" vlg_status vlg_index_isa_samples(const vlg_index* idx, uint32_t inv_dens, uint64_t* h_out, uint64_t count)
{
    if (!idx || !h_out || !inv_dens) return fail(VLG_E_INVALID, "null argument");
    const uint64_t n = idx->hdr.n;
    if (count != (n - 1) / inv_dens + 1) return fail(VLG_E_INVALID, "ISA sample count must be (n-1)/inv_dens + 1");
    if (idx->hdr.sampling != kSamplingSaOrder) return fail(VLG_E_UNSUPPORTED, "ISA samples are computed from an SA-order index");
    const uint32_t w = isa_sample_bytes(n);
    DevBuf out_buf;
    VLG_HIP_TRY(out_buf.alloc(count * (8 + w)));                      // the samples as the device keeps them, then widened
    uint64_t* d_out = out_buf.as<uint64_t>();
    void* d_smp = d_out + count;
    vlg_status s = isa_samples_device(idx, inv_dens, d_smp, nullptr);
    if (!s) s = w == 8 ? (hipMemcpyAsync(d_out, d_smp, count * 8, hipMemcpyDeviceToDevice, nullptr) == hipSuccess ? VLG_OK : VLG_E_NO_DEVICE)
                       : launch_widen<uint32_t>((const uint32_t*)d_smp, d_out, count, nullptr);
    hipError_t e = s ? hipSuccess : hipMemcpy(h_out, d_out, count * 8, hipMemcpyDeviceToHost);
    if (s) return s == VLG_E_NO_DEVICE ? fail(s, "ISA samples: device copy failed") : s;
    VLG_HIP_TRY(e);
    return VLG_OK;
}

// ---- text access: sdsl::extract, csa.text[i], csa.isa[i] (extract.hpp) ----------------------------------------------------------------
// (struct vlg_text_access: common.hpp)
extern "C" vlg_status vlg_text_access_create(const vlg_index* idx, uint32_t inv_dens, void* stream, vlg_text_access** out)
{
    if (!idx || !out) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    if (idx->hdr.sampling != kSamplingSaOrder)
        return fail(VLG_E_UNSUPPORTED, "text access needs an SA-order index (a text-order index derives its ISA through the marks)");
    const uint32_t d = inv_dens ? inv_dens : 64;
    hipStream_t st = (hipStream_t)stream;
    vlg_text_access* t = new (std::nothrow) vlg_text_access;
    if (!t) return fail(VLG_E_OOM, "text access handle");
    t->idx = idx;
    t->d = d;
    t->isa_bytes = isa_sample_bytes(idx->hdr.n);
    const uint64_t count = (idx->hdr.n - 1) / d + 1;
    vlg_status s = VLG_OK;
    if (hipMalloc(&t->d_isa, count * t->isa_bytes) != hipSuccess) { t->d_isa = nullptr; s = fail(VLG_E_OOM, "text access: ISA samples"); }
    if (!s) s = isa_samples_device(idx, d, t->d_isa, st);
    if (!s && !idx->is_int) {
        if (hipMalloc((void**)&t->d_c2c, 256) != hipSuccess) { t->d_c2c = nullptr; s = fail(VLG_E_OOM, "text access: comp2char"); }
        else if (hipMemsetAsync(t->d_c2c, 0, 256, st) != hipSuccess) s = fail(VLG_E_NO_DEVICE, "text access: comp2char");
        else hipLaunchKernelGGL(comp2char_kernel, dim3(1), dim3(256), 0, st, idx->view.char2comp, t->d_c2c);
    }
    if (!s) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) s = fail(VLG_E_NO_DEVICE, std::string("text access: ") + hipGetErrorString(e));
    }
    if (s) { vlg_text_access_destroy(t); return s; }
    *out = t;
    return VLG_OK;
}

extern "C" void vlg_text_access_destroy(vlg_text_access* t)
{
    if (!t) return;
    if (t->d_isa) (void)hipFree(t->d_isa);
    if (t->d_c2c) (void)hipFree(t->d_c2c);
    delete t;
}

extern "C" vlg_status vlg_extract_batch(const vlg_text_access* t, const uint64_t* d_begin, const uint64_t* d_end, const uint64_t* d_out_off,
                                        uint64_t n_ranges, uint64_t total, void* d_out, void* stream)
{
    if (!t || (n_ranges && (!d_begin || !d_end || !d_out_off || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!n_ranges) return VLG_OK;
    const vlg_index* idx = t->idx;
    hipStream_t st = (hipStream_t)stream;
    // scratch: [0, n_ranges] segment counts scanned in place, then the bad-range counter
    size_t tb = 0;
    uint64_t* seg = nullptr;
    VLG_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, seg, seg, (uint64_t)0, n_ranges + 1, rocprim::plus<uint64_t>(), st));
    const size_t seg_bytes = align_up((n_ranges + 1) * 8 + 8, 256);
    DevBuf seg_buf;
    VLG_HIP_TRY(seg_buf.alloc(seg_bytes + tb));
    seg = seg_buf.as<uint64_t>();
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(seg + n_ranges + 1);
    void* temp = reinterpret_cast<uint8_t*>(seg) + seg_bytes;
    uint64_t h[2] = {0, 0};                                        // bad ranges, segments
    hipError_t e = hipMemsetAsync(d_bad, 0, 8, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(extract_check_kernel, launch_grid(n_ranges + 1, 4096), dim3(256), 0, st, d_begin, d_end, d_out_off, n_ranges, idx->hdr.n,
                           total, t->d, seg, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(temp, tb, seg, seg, (uint64_t)0, n_ranges + 1, rocprim::plus<uint64_t>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[0], d_bad, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[1], seg + n_ranges, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    vlg_status s = VLG_OK;
    if (e != hipSuccess) s = fail(VLG_E_NO_DEVICE, std::string("extract: ") + hipGetErrorString(e));
    else if (h[0]) s = fail(VLG_E_INVALID, std::to_string(h[0]) + " extract range(s) with begin > end, end >= n, or output beyond total");
    if (!s) {
        const ExtractJob job{d_begin, d_end, d_out_off, seg, n_ranges, h[1], idx->hdr.n, t->d};
        const IndexView& iv = idx->view;
        if (idx->is_int) s = launch_int_extract(idx->iview, job, (const uint32_t*)t->d_isa, (uint32_t*)d_out, st);
        else s = on_bv(iv.bv_kind, [&](auto bv) { return on_text_access_shape(shape(iv).wide, t->isa_bytes, [&](auto wide, auto isa) {
            using isa_t = tag_t<decltype(isa)>;
            return launch(extract_kernel<tag_t<decltype(bv)>, decltype(wide)::value, isa_t>, launch_grid(h[1], 8192), st, iv, job, (const isa_t*)t->d_isa, t->d_c2c, (uint8_t*)d_out);
        }); });
        e = hipStreamSynchronize(st);                              // the scratch is freed on return
        if (!s && e != hipSuccess) s = fail(VLG_E_NO_DEVICE, std::string("extract: ") + hipGetErrorString(e));
    }
    return s;
}

extern "C" vlg_status vlg_isa_batch(const vlg_text_access* t, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!t || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    const vlg_index* idx = t->idx;
    hipStream_t st = (hipStream_t)stream;
    DevBuf bad_buf;
    VLG_HIP_TRY(bad_buf.alloc(8));
    unsigned long long* d_bad = bad_buf.as<unsigned long long>();
    unsigned long long h_bad = 0;
    vlg_status s = VLG_OK;
    hipError_t e = hipMemsetAsync(d_bad, 0, 8, st);
    if (e == hipSuccess) {
        if (idx->is_int) s = launch_int_isa(idx->iview, t->d, (const uint32_t*)t->d_isa, d_i, d_out, count, d_bad, st);
        else s = on_bv(idx->view.bv_kind, [&](auto bv) { return on_text_access_shape(shape(idx->view).wide, t->isa_bytes, [&](auto wide, auto isa) {
            using isa_t = tag_t<decltype(isa)>;
            return launch(isa_kernel<tag_t<decltype(bv)>, decltype(wide)::value, isa_t>, launch_grid(count, 8192), st, idx->view, t->d, (const isa_t*)t->d_isa, d_i, d_out, count, d_bad);
        }); });
    }
    if (e == hipSuccess && !s) e = hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (s) return s;
    if (e != hipSuccess) return fail(VLG_E_NO_DEVICE, std::string("isa: ") + hipGetErrorString(e));
    if (h_bad) return fail(VLG_E_INVALID, std::to_string(h_bad) + " ISA position(s) >= n");
    return VLG_OK;
}

// ---- select (select.hpp): select_support_mcl / select_support_rrr on a bit-vector, wt_pc::select / wt_int::select, csa.psi, csa.lf, csa.bwt --
struct vlg_select_support {
    int kind = 0;                                                  // kSelPlainBv, kSelRrrBv, kSelIndex
    const vlg_bitvector* bv = nullptr;
    const vlg_rrr_bitvector* rrr = nullptr;
    const vlg_index* idx = nullptr;
    SelView view{};
    void* d_mem = nullptr;                                         // nodes, leaf_up, the hint pass's lists, hints: one allocation
    uint64_t bytes = 0;
};

namespace {

constexpr int kSelPlainBv = 0, kSelRrrBv = 1, kSelIndex = 2;

template <class Counts>
__global__ void __launch_bounds__(256) select_hints_kernel(Counts src, const SelNode* __restrict__ nodes, const uint32_t* __restrict__ list,
                                                           const uint64_t* __restrict__ first, uint32_t n_list, uint32_t shift, uint32_t* __restrict__ hints)
{
    select_build_hints(src, nodes, list, first, n_list, shift, hints);
}

// K1's view of a stand-alone bit-vector, as the plain policy reads an index
struct BitsView {
    const Block* blocks;
};

template <int kBit>
__global__ void __launch_bounds__(256) bit_select_kernel(BitsView bv, SelView sv, const uint64_t* __restrict__ k, uint64_t* __restrict__ out, uint64_t count)
{
    const PlainBV::Shared sh{};
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x)
        out[j] = bit_select<PlainBV>(bv, sh, sv, (uint32_t)kBit, k[j]);
}

// select_support_rrr on K6's layout: the header search of the rrr policy, the classes of the super-block, then the block decoded bit
// by bit as K6 numbers it (rrr_select63_seq), the binomial table in LDS as in rrr_rank_kernel
template <int kBit>
__global__ void __launch_bounds__(256) rrr_bit_select_kernel(const uint4* __restrict__ hdr, const uint64_t* __restrict__ stream, const uint64_t* __restrict__ binom,
                                                             SelView sv, const uint64_t* __restrict__ k_in, uint64_t* __restrict__ out, uint64_t count)
{
    __shared__ RrrLds s;
    stage_rrr_lds(s, binom);
    constexpr uint32_t bit = (uint32_t)kBit;
    const SelNode nd = sv.nodes[0];
    const uint64_t have = bit ? nd.ones : nd.size - nd.ones;
    const uint32_t* hints = sv.hints + (bit ? nd.h1 : nd.h0);
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = k_in[q];
        if (k == 0 || k > have) { out[q] = nd.size; continue; }
        const uint32_t sb = select_superblock(hints, sv.shift, kRrrBlock * kRrrSuper, bit, k, [&](uint32_t x) { return hdr[2 * (uint64_t)x].x; });
        const uint4 h0 = hdr[2 * (uint64_t)sb], h1 = hdr[2 * (uint64_t)sb + 1];
        uint32_t kk = (uint32_t)(k - (bit ? (uint64_t)h0.x : (uint64_t)sb * (kRrrBlock * kRrrSuper) - h0.x));
        uint64_t ptr = h0.y;
        const uint64_t c0 = (uint64_t)h0.z | ((uint64_t)h0.w << 32), c1 = (uint64_t)h1.x | ((uint64_t)h1.y << 32),
                       c2 = (uint64_t)h1.z | ((uint64_t)h1.w << 32);
        uint32_t blk = 0, cls = rrr_class(c0, c1, c2, 0);
        for (; blk < kRrrSuper - 1; ++blk) {
            const uint32_t n_here = bit ? cls : kRrrBlock - cls;
            if (kk <= n_here) break;
            kk -= n_here;
            ptr += s.space[cls];
            cls = rrr_class(c0, c1, c2, blk + 1);
        }
        const uint32_t len = s.space[cls];
        const uint64_t nr = rrr_stream_bits(stream, ptr, len);
        out[q] = (uint64_t)sb * (kRrrBlock * kRrrSuper) + blk * kRrrBlock + rrr_select63_seq(&s.binom[0][0], cls, nr, bit, kk);
    }
}

// wt_pc::select(k, c) for text bytes c (kPsi = false), or csa.psi[i] = select(i - C[F[i]] + 1, F[i]) (kPsi = true: `arg` holds i)
template <class BV, bool kPsi>
__global__ void __launch_bounds__(256) wt_select_kernel(IndexView iv, SelView sv, const uint64_t* __restrict__ arg, const uint8_t* __restrict__ sym,
                                                        uint64_t* __restrict__ out, uint64_t count)
{
    __shared__ uint64_t sC[257];
    __shared__ typename BV::Shared sh;
    for (uint32_t i = threadIdx.x; i <= iv.sigma; i += blockDim.x) sC[i] = iv.C[i];
    BV::stage(sh, iv);
    __syncthreads();
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = arg[j];
        if (kPsi) {
            if (a >= iv.n) { out[j] = ~0ull; continue; }
            const uint32_t c = first_column(sC, iv.sigma, a);
            out[j] = byte_select<BV>(iv, sh, sv, c, a - sC[c] + 1);
        } else {
            const uint8_t ch = sym[j];
            const uint32_t c = iv.char2comp[ch];
            const bool present = ch == 0 || c != 0;                // wt_pc.hpp:418-420
            out[j] = (present && a >= 1 && a <= sC[c + 1] - sC[c]) ? byte_select<BV>(iv, sh, sv, c, a) : iv.n;
        }
    }
}

// csa.lf[i] and csa.bwt[i]: one LF step of lf_walk.hpp per lane; either output may be null
template <class BV, bool kWide>
__global__ void __launch_bounds__(256) lf_bwt_kernel(IndexView iv, const uint64_t* __restrict__ in, uint64_t* __restrict__ out_lf, uint8_t* __restrict__ out_bwt,
                                                     uint64_t count)
{
    __shared__ WalkLds<BV> s;
    __shared__ uint8_t c2c[256];
    c2c[threadIdx.x] = 0;
    __syncthreads();
    { const uint32_t ch = threadIdx.x, c = iv.char2comp[ch]; if (ch == 0 || c != 0) c2c[c] = (uint8_t)ch; }      // comp2char (256 threads)
    stage_walk(s, iv);
    const ByteWalk<BV, kWide> walk{iv, s, c2c};
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = in[j];
        uint32_t c = 0;
        const uint64_t r = i < iv.n ? walk.lf(i, c) : ~0ull;
        if (out_lf) out_lf[j] = r;
        if (out_bwt) out_bwt[j] = i < iv.n ? walk.sym(c) : (uint8_t)0;
    }
}

// the hint pass of select_support_finish over one source of counts
template <class Counts>
auto select_hints_pass(const Counts& src, uint32_t shift, hipStream_t st)
{
    return [=](const SelNode* nd, const uint32_t* list, const uint64_t* first, uint32_t n_list, uint32_t* hints, dim3 grid) {
        return launch(select_hints_kernel<Counts>, grid, st, src, nd, list, first, n_list, shift, hints);
    };
}

bool select_sample_shift(uint32_t sample, uint32_t& shift)
{
    const uint32_t s = sample ? sample : kSelectSampleDefault;
    if (s < kSelectSampleMin || s > kSelectSampleMax || (s & (s - 1))) return false;
    shift = 31u - (uint32_t)__builtin_clz(s);
    return true;
}

// Lay the handle out, upload its tables and run the hint pass.  nodes: every SelNode with size, ones, base, nb, up set (nb = 0: no
// bit-vector, a leaf); hint offsets are assigned here.  run(nodes, list, first, n_list, hints, grid) launches the pass for the source's
// layout (select_hints_pass).
template <class Run>
vlg_status select_support_finish(vlg_select_support* s, std::vector<SelNode>& nodes, const std::vector<uint32_t>& leaf_up, uint32_t shift, hipStream_t st,
                                 const Run& run)
{
    std::vector<uint32_t> list;
    std::vector<uint64_t> first(1, 0);
    uint64_t n_hints = 0;
    for (uint32_t v = 0; v < nodes.size(); ++v) {
        if (!nodes[v].nb) continue;
        nodes[v].h1 = n_hints; n_hints += select_hint_count(nodes[v].ones, shift);
        nodes[v].h0 = n_hints; n_hints += select_hint_count(nodes[v].size - nodes[v].ones, shift);
        list.push_back(v);
        first.push_back(first.back() + nodes[v].nb);
    }
    const uint64_t off_nodes = 0, off_leaf = align_up(off_nodes + std::max<size_t>(nodes.size(), 1) * sizeof(SelNode), 256),
                   off_list = align_up(off_leaf + std::max<size_t>(leaf_up.size(), 1) * 4, 256), off_first = align_up(off_list + std::max<size_t>(list.size(), 1) * 4, 256),
                   off_hints = align_up(off_first + first.size() * 8, 256);
    s->bytes = align_up(off_hints + std::max<uint64_t>(n_hints, 1) * 4, 256);
    if (hipMalloc(&s->d_mem, s->bytes) != hipSuccess) { s->d_mem = nullptr; return fail(VLG_E_OOM, "select support: " + std::to_string(s->bytes) + " bytes"); }
    uint8_t* b = reinterpret_cast<uint8_t*>(s->d_mem);
    s->view.nodes = reinterpret_cast<const SelNode*>(b + off_nodes);
    s->view.leaf_up = reinterpret_cast<const uint32_t*>(b + off_leaf);
    s->view.hints = reinterpret_cast<const uint32_t*>(b + off_hints);
    s->view.shift = shift;
    s->view.n_nodes = (uint32_t)nodes.size();
    if (!nodes.empty()) VLG_HIP_TRY(hipMemcpyAsync(b + off_nodes, nodes.data(), nodes.size() * sizeof(SelNode), hipMemcpyHostToDevice, st));
    if (!leaf_up.empty()) VLG_HIP_TRY(hipMemcpyAsync(b + off_leaf, leaf_up.data(), leaf_up.size() * 4, hipMemcpyHostToDevice, st));
    if (!list.empty()) VLG_HIP_TRY(hipMemcpyAsync(b + off_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
    VLG_HIP_TRY(hipMemcpyAsync(b + off_first, first.data(), first.size() * 8, hipMemcpyHostToDevice, st));
    VLG_HIP_TRY(hipMemsetAsync(b + off_hints, 0, std::max<uint64_t>(n_hints, 1) * 4, st));
    if (!list.empty()) {
        if (vlg_status r = run(s->view.nodes, reinterpret_cast<const uint32_t*>(b + off_list), reinterpret_cast<const uint64_t*>(b + off_first), (uint32_t)list.size(),
                               reinterpret_cast<uint32_t*>(b + off_hints), launch_grid(first.back(), 8192))) return r;
    }
    VLG_HIP_TRY(hipStreamSynchronize(st));                         // (the host tables are read until here)
    return VLG_OK;
}

vlg_status select_create_checks(const void* src, uint32_t sample, vlg_select_support** out, uint32_t& shift)
{
    if (!src || !out) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    if (!select_sample_shift(sample, shift))
        return fail(VLG_E_INVALID, "select support: sample must be 0 (the default, 512) or a power of two in [64, 65536]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available");
    return VLG_OK;
}

using SelectPtr = Building<vlg_select_support, vlg_select_support_destroy>;

}  // namespace

extern "C" vlg_status vlg_bitvector_select_create(const vlg_bitvector* bv, uint32_t sample, void* stream, vlg_select_support** out)
{
    uint32_t shift = 0;
    if (vlg_status st = select_create_checks(bv, sample, out, shift)) return st;
    SelectPtr s(new vlg_select_support());
    s->kind = kSelPlainBv;
    s->bv = bv;
    // ones of the whole vector: the count before the last block + its popcount (bv_pack_kernel leaves the bits past nbits zero).  A
    // blocking read of 32 bytes: the source was synchronised when it was created; everything after it runs on `stream`.
    uint64_t ones = 0;
    {
        Block last;
        VLG_HIP_TRY(hipMemcpy(&last, bv->d_blocks + (bv->n_blocks - 1), sizeof(Block), hipMemcpyDeviceToHost));
        ones = last.cnt;
        for (uint32_t w = 0; w < 7; ++w) ones += (uint32_t)__builtin_popcount(last.w[w]);
    }
    std::vector<SelNode> nodes(1, SelNode{bv->nbits, ones, 0, 0, 0, (uint32_t)bv->n_blocks, kSelNoParent, 0});
    hipStream_t st = (hipStream_t)stream;
    if (vlg_status r = select_support_finish(s.get(), nodes, {}, shift, st, select_hints_pass(PlainCounts{bv->d_blocks}, shift, st))) return r;
    *out = s.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_rrr_bitvector_select_create(const vlg_rrr_bitvector* bv, uint32_t sample, void* stream, vlg_select_support** out)
{
    uint32_t shift = 0;
    if (vlg_status st = select_create_checks(bv, sample, out, shift)) return st;
    SelectPtr s(new vlg_select_support());
    s->kind = kSelRrrBv;
    s->rrr = bv;
    // ones before the last super-block + its 32 classes (blocks past nbits are class 0); a blocking read of 32 bytes, as above
    uint64_t ones = 0;
    {
        uint32_t H[8];
        VLG_HIP_TRY(hipMemcpy(H, bv->d_hdr + 2 * (bv->n_sb - 1), 32, hipMemcpyDeviceToHost));
        ones = H[0];
        const uint64_t c[3] = {(uint64_t)H[2] | ((uint64_t)H[3] << 32), (uint64_t)H[4] | ((uint64_t)H[5] << 32), (uint64_t)H[6] | ((uint64_t)H[7] << 32)};
        for (uint32_t j = 0; j < 32; ++j) {
            const uint32_t bit = 6 * j, w = bit >> 6, o = bit & 63;
            uint64_t v = c[w] >> o;
            if (o > 58) v |= c[w + 1] << (64 - o);
            ones += v & 63;
        }
    }
    std::vector<SelNode> nodes(1, SelNode{bv->nbits, ones, 0, 0, 0, (uint32_t)bv->n_sb, kSelNoParent, 0});
    hipStream_t st = (hipStream_t)stream;
    if (vlg_status r = select_support_finish(s.get(), nodes, {}, shift, st, select_hints_pass(RrrCounts{bv->d_hdr}, shift, st))) return r;
    *out = s.release();
    return VLG_OK;
}

extern "C" vlg_status vlg_index_select_create(const vlg_index* idx, uint32_t sample, void* stream, vlg_select_support** out)
{
    uint32_t shift = 0;
    if (vlg_status st = select_create_checks(idx, sample, out, shift)) return st;
    SelectPtr s(new vlg_select_support());
    s->kind = kSelIndex;
    s->idx = idx;
    std::vector<SelNode> nodes;
    std::vector<uint32_t> leaf_up;
    const uint64_t n = idx->hdr.n;
    bool rrr;
    if (idx->is_int) {                                             // one node per level of the matrix: n bits, n - Z[l] ones
        const IntView& v = idx->iview;
        rrr = shape(v).rrr;
        uint64_t Z[kMaxIntLevels] = {0};
        if (v.n_levels) VLG_HIP_TRY(hipMemcpy(Z, v.Z, v.n_levels * 8, hipMemcpyDeviceToHost));
        for (uint32_t l = 0; l < v.n_levels; ++l) {
            if (Z[l] > n) return fail(VLG_E_INVALID, "select support: a level has more zeros than symbols");
            nodes.push_back(SelNode{n, n - Z[l], 0, 0, (uint32_t)(l * v.stride), (uint32_t)(n / (rrr ? kRrrSuperBits : kBlockBits) + 1), kSelNoParent, 0});
        }
    } else {                                                       // the tree as the kernels walk it; sizes from the symbol counts
        const IndexView& v = idx->view;
        rrr = shape(v).rrr;
        const uint32_t nn = v.n_nodes, sigma = v.sigma;
        std::vector<DNode> dn(std::max<uint32_t>(nn, 1));
        std::vector<uint64_t> Cc(sigma + 1, 0);
        if (nn) VLG_HIP_TRY(hipMemcpy(dn.data(), v.nodes, nn * sizeof(DNode), hipMemcpyDeviceToHost));
        VLG_HIP_TRY(hipMemcpy(Cc.data(), v.C, (sigma + 1) * 8, hipMemcpyDeviceToHost));
        leaf_up.assign(std::max<uint32_t>(sigma, 1), kSelNoParent);
        if (sigma > 1) {
            nodes.assign(nn, SelNode{0, 0, 0, 0, 0, 0, kSelNoParent, 0});
            std::vector<uint8_t> inner(nn, 0);
            inner[0] = 1;
            for (uint32_t p = 0; p < nn; ++p) {                    // top-down: who is inner, and the way up
                if (!inner[p]) continue;
                for (uint32_t b = 0; b < 2; ++b) {
                    const uint32_t ch = dn[p].child[b];
                    if (ch & kLeafFlag) { if ((ch & ~kLeafFlag) >= sigma) return fail(VLG_E_INVALID, "select support: leaf symbol out of range"); leaf_up[ch & ~kLeafFlag] = 2 * p + b; }
                    else if (ch <= p || ch >= nn) return fail(VLG_E_INVALID, "select support: node table is not in BFS order");
                    else { inner[ch] = 1; nodes[ch].up = 2 * p + b; }
                }
            }
            for (uint32_t p = nn; p-- > 0;) {                      // bottom-up: sizes
                if (!inner[p]) continue;
                uint64_t cnt[2];
                for (uint32_t b = 0; b < 2; ++b) {
                    const uint32_t ch = dn[p].child[b];
                    cnt[b] = (ch & kLeafFlag) ? Cc[(ch & ~kLeafFlag) + 1] - Cc[ch & ~kLeafFlag] : nodes[ch].size;
                }
                nodes[p].size = cnt[0] + cnt[1];
                nodes[p].ones = cnt[1];
                nodes[p].base = dn[p].base;
                nodes[p].nb = (uint32_t)(nodes[p].size / (rrr ? kRrrSuperBits : kBlockBits) + 1);
            }
            if (nodes[0].size != n) return fail(VLG_E_INVALID, "select support: the tree does not hold n symbols");
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const auto finish = [&](const auto& src) { return select_support_finish(s.get(), nodes, leaf_up, shift, st, select_hints_pass(src, shift, st)); };
    if (vlg_status r = rrr ? finish(RrrCounts{idx->is_int ? idx->iview.rrr_hdr : idx->view.rrr_hdr}) : finish(PlainCounts{idx->is_int ? idx->iview.blocks : idx->view.blocks}))
        return r;
    *out = s.release();
    return VLG_OK;
}

extern "C" uint64_t vlg_select_support_hbm_bytes(const vlg_select_support* s) { return s ? s->bytes : 0; }

extern "C" void vlg_select_support_destroy(vlg_select_support* s)
{
    if (!s) return;
    if (s->d_mem) (void)hipFree(s->d_mem);
    delete s;
}

extern "C" vlg_status vlg_bit_select_batch(const vlg_select_support* s, int bit, const uint64_t* d_k, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!s || (count && (!d_k || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (bit != 0 && bit != 1) return fail(VLG_E_INVALID, "bit select: bit must be 0 or 1");
    if (s->kind == kSelIndex) return fail(VLG_E_INVALID, "bit select: the support was made from an index (use vlg_wt_select_batch / vlg_int_select_batch)");
    if (!count) return VLG_OK;
    hipStream_t st = (hipStream_t)stream;
    return on_flag(bit != 0, [&](auto one) {
        constexpr int kBit = decltype(one)::value ? 1 : 0;
        if (s->kind == kSelPlainBv) return launch(bit_select_kernel<kBit>, launch_grid(count, 8192), st, BitsView{s->bv->d_blocks}, s->view, d_k, d_out, count);
        const vlg_rrr_bitvector* r = s->rrr;
        return launch(rrr_bit_select_kernel<kBit>, launch_grid(count, 2048), st, r->d_hdr, r->d_stream, r->d_binom, s->view, d_k, d_out, count);
    });
}

extern "C" vlg_status vlg_wt_select_batch(const vlg_select_support* s, const uint64_t* d_k, const uint8_t* d_c, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!s || (count && (!d_k || !d_c || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (s->kind != kSelIndex) return fail(VLG_E_INVALID, "wt select: the support was made from a bit-vector (use vlg_bit_select_batch)");
    if (s->idx->is_int) return fail(VLG_E_INVALID, "integer-alphabet index: use vlg_int_select_batch");
    if (!count) return VLG_OK;
    return on_bv(s->idx->view.bv_kind, [&](auto bv) {
        return launch(wt_select_kernel<tag_t<decltype(bv)>, false>, launch_grid(count, 8192), (hipStream_t)stream, s->idx->view, s->view, d_k, d_c, d_out, count);
    });
}

extern "C" vlg_status vlg_int_select_batch(const vlg_select_support* s, const uint64_t* d_k, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!s || (count && (!d_k || !d_sym || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (s->kind != kSelIndex) return fail(VLG_E_INVALID, "int select: the support was made from a bit-vector (use vlg_bit_select_batch)");
    if (!s->idx->is_int) return fail(VLG_E_INVALID, "byte-alphabet index: use vlg_wt_select_batch");
    if (!count) return VLG_OK;
    return launch_int_select(s->idx->iview, s->view, d_k, d_sym, d_out, count, (hipStream_t)stream);
}

extern "C" vlg_status vlg_psi_batch(const vlg_select_support* s, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!s || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (s->kind != kSelIndex) return fail(VLG_E_INVALID, "psi: the support was made from a bit-vector");
    if (!count) return VLG_OK;
    if (s->idx->is_int) return launch_int_select(s->idx->iview, s->view, d_i, nullptr, d_out, count, (hipStream_t)stream);
    return on_bv(s->idx->view.bv_kind, [&](auto bv) {
        return launch(wt_select_kernel<tag_t<decltype(bv)>, true>, launch_grid(count, 8192), (hipStream_t)stream, s->idx->view, s->view, d_i, nullptr, d_out, count);
    });
}

namespace {
vlg_status lf_bwt_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_lf, void* d_bwt, uint64_t count, hipStream_t st)
{
    if (idx->is_int) return launch_int_lf_bwt(idx->iview, d_i, d_lf, (uint32_t*)d_bwt, count, st);
    const IndexView& iv = idx->view;
    return on_bv(iv.bv_kind, [&](auto bv) { return on_flag(shape(iv).wide, [&](auto wide) {
        return launch(lf_bwt_kernel<tag_t<decltype(bv)>, decltype(wide)::value>, launch_grid(count, 8192), st, iv, d_i, d_lf, (uint8_t*)d_bwt, count);
    }); });
}
}  // namespace

extern "C" vlg_status vlg_lf_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream)
{
    if (!idx || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    return lf_bwt_batch(idx, d_i, d_out, nullptr, count, (hipStream_t)stream);
}

extern "C" vlg_status vlg_bwt_batch(const vlg_index* idx, const uint64_t* d_i, void* d_out, uint64_t count, void* stream)
{
    if (!idx || (count && (!d_i || !d_out))) return fail(VLG_E_INVALID, "null argument");
    if (!count) return VLG_OK;
    return lf_bwt_batch(idx, d_i, nullptr, d_out, count, (hipStream_t)stream);
}

namespace {
// LF through the quad walk, for tests: what QuadWalk::lf returns, reads and counts for every SA index of a batch
template <bool kWide>
__global__ void __launch_bounds__(256) quad_lf_kernel(IndexView iv, const uint64_t* __restrict__ in, uint64_t* __restrict__ out_lf, uint8_t* __restrict__ out_comp,
                                                      uint32_t* __restrict__ out_levels, uint64_t count)
{
    __shared__ QuadLds s;
    QuadWalk<kWide>::stage(s, iv);
    const QuadWalk<kWide> walk{iv, s};
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = in[j];
        uint32_t c = 0, n_lv = 0;
        const uint64_t r = i < iv.n ? walk.lf(i, c, n_lv) : ~0ull;
        if (out_lf) out_lf[j] = r;
        if (out_comp) out_comp[j] = (uint8_t)c;
        if (out_levels) out_levels[j] = n_lv;
    }
}
}  // namespace

extern "C" vlg_status vlg_quad_lf_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_lf, uint8_t* d_comp, uint32_t* d_levels, uint64_t count)
{
    if (!idx || (count && !d_i)) return fail(VLG_E_INVALID, "null argument");
    if (idx->is_int || !idx->view.qblocks) return fail(VLG_E_UNSUPPORTED, "the index has no quad image");
    if (!count) return VLG_OK;
    const IndexView& iv = idx->view;
    const vlg_status s = on_flag(shape(iv).wide, [&](auto wide) {
        return launch(quad_lf_kernel<decltype(wide)::value>, launch_grid(count, 8192), (hipStream_t) nullptr, iv, d_i, d_lf, d_comp, d_levels, count);
    });
    if (s) return s;
    VLG_HIP_TRY(hipStreamSynchronize(nullptr));
    return VLG_OK;
}

extern "C" vlg_status vlg_index_quad_image(const vlg_index* idx, uint64_t* bytes, uint32_t* n_nodes, double* build_s)
{
    if (!idx) return fail(VLG_E_INVALID, "null argument");
    const bool have = !idx->is_int && idx->view.qblocks;
    if (bytes) *bytes = have ? idx->quad.cap : 0;
    if (n_nodes) *n_nodes = have ? idx->view.n_qnodes : 0;
    if (build_s) *build_s = have ? idx->quad_build_s : 0.0;
    return VLG_OK;
}
