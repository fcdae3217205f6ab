// Shared declarations of the MI355X VLG library (device layout, error plumbing).
//
// HBM layout of the index ("blob": ONE contiguous device allocation, 256-byte aligned sections):
//
//   [BlobHeader][blocks][nodes][C][paths][char2comp][samples][reference-layout nodes]
//
// blocks : the Huffman-shaped wavelet tree of the BWT, level-contiguous like the reference
//          (BFS node order, include/sdsl/wt_helper.hpp:170-206) but re-cut into 256-bit
//          super-blocks  { 7 x u32 data = 224 bits, u32 cnt }.  Every inner node starts on a
//          block boundary and owns size/224 + 1 blocks; cnt = number of 1s of THIS NODE before the
//          block (node-relative, so bv_pos_rank(v) of wt_pc.hpp:364 is folded away and the count
//          fits 32 bits for n <= 2^32).  One rank = one aligned 32-byte read.
// nodes  : DNode per tree node {first block, child[0], child[1]}; a child word with bit 31 set is a
//          leaf and carries the alphabet rank (comp) of its symbol in the low bits.
// C      : u64[sigma+1] cumulative counts (lib/csa_alphabet_strategy.cpp:25-55)
// paths  : u64[256] m_path of wt_helper.hpp:219-240 (code bits, first edge in bit 0; length in 56..63)
// samples: SA[0], SA[d], SA[2d], ... as u32 (n <= 2^32) or u64 (sa_order_sa_sampling, the default); or, for
//          text_order_sa_sampling (csa_sampling_strategy.hpp:127-246), SA[i] / d of the SA indices i with SA[i] % d == 0 in
//          ascending i, plus [marked]: super-blocks {224 marks, ones before} over the SA indices -- is_sampled(i) and the rank
//          that addresses the sample come out of ONE 32-byte read.
//
// Beside the blob, in an allocation of its own (vlg_index::quad): the quad image of a plain byte index -- [QNode x 256][QuadBlock ...],
// the tree two levels per 32-byte read for the locate walks (quad_code.hpp has the layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include "../../include/vlg_hip.h"

namespace vlg {

constexpr uint32_t kBlockBits = 224;
constexpr uint32_t kLeafFlag = 0x80000000u;
constexpr uint64_t kBlobMagic = 0x32424C4756ULL;  // "VGLB2" (2: rrr offsets numbered by halves, rrr_code.hpp)
constexpr uint32_t kMaxNodes = 512;

struct __attribute__((aligned(16))) DNode {
    uint32_t base;      // first 32-byte block of the node (inner nodes only)
    uint32_t child[2];  // node id, or kLeafFlag | comp
    uint32_t size_lo;   // node size in bits (low 32 bits; informational)
};

struct __attribute__((aligned(32))) Block {
    uint32_t w[7];
    uint32_t cnt;
};

struct BlobHeader {
    uint64_t magic;
    uint64_t total_bytes;
    uint64_t n;
    uint64_t wt_bits;
    uint64_t n_blocks;
    uint64_t n_samples;
    uint32_t sigma;
    uint32_t dens;
    uint32_t n_nodes;
    uint32_t max_code_len;
    uint32_t sample_bytes;
    uint32_t sampling;            // 0 = SA order (SA[0], SA[d], ...: _sa_order_sampling), 1 = text order (_text_order_sampling: a marked
                                  // bit-vector over SA indices + SA / d of the marked ones)
    uint64_t off_blocks, off_nodes, off_C, off_paths, off_c2c, off_samples, off_refnodes;
    uint64_t bv_kind;             // 0 = plain 256-bit super-blocks, 1 = rrr-63 (headers + offset stream as K6, block code of rrr_code.hpp)
    uint64_t off_rrr_hdr, off_rrr_stream, off_binom, n_rrr_sb, rrr_stream_words;
    uint64_t off_marked;          // text-order sampling: n / 224 + 1 super-blocks {224 marks, ones before} over the SA indices
};

// What kernels receive (by value).
struct IndexView {
    const Block* blocks;
    const DNode* nodes;
    const uint64_t* C;
    const uint64_t* paths;
    const uint8_t* char2comp;
    const void* samples;
    uint64_t n;
    uint64_t n_samples;
    uint32_t n_nodes;
    uint32_t sigma;
    uint32_t dens;
    uint32_t sample_bytes;
    // rrr-63 variant of the wavelet-tree bit-vectors (bv_kind == 1): DNode.base counts 32-byte headers
    uint32_t bv_kind;
    uint32_t sampling;                    // kSamplingSaOrder / kSamplingTextOrder
    const Block* marked;                  // text-order sampling: marks over the SA indices (samples = SA / dens of the marked ones)
    const uint4* rrr_hdr;
    const uint64_t* rrr_stream;
    const struct RrrTables* rrr_tables;   // rrr_code.hpp
    // the 4-ary image of the tree (quad_code.hpp; null = none: rrr bit-vectors, sigma = 1, a digit count beyond 32 bits).  It is not part
    // of the blob: every index derives its own from `blocks` when it is made (index.hip: derive_quad_image)
    const struct QuadBlock* qblocks;
    const struct QNode* qnodes;
    uint32_t n_qnodes;
};

// ---- FM-index of an integer text (int_index.hpp): its own blob, recognised by its magic -------------------------------------
constexpr uint64_t kIntBlobMagic = 0x3149474C56ULL;   // "VLGI1"
constexpr uint32_t kMaxIntLevels = 32;
struct IntHeader {
    uint64_t magic, total_bytes;                      // (the first two words as in BlobHeader: what export / attach look at)
    uint64_t n, sigma, n_samples, nb;                 // nb = super-blocks per level
    uint32_t levels, dens;
    uint64_t off_levels, off_Z, off_D, off_C, off_c2c, off_samples;
    // rrr-63 levels (vlg_index_compress of an integer index; all zero in a plain one -- the header is followed by zeros up to 256 bytes,
    // so blobs written before these fields existed read as plain): the layout of the byte index's rrr variant, one "node" per level
    uint64_t bv_kind, n_sb /* super-blocks of 32 x 63 bits per level */, rrr_words, off_rrr_hdr, off_rrr_stream, off_binom;
    // SA sampling (vlg_index_resample of an integer index; zero in blobs written before these fields existed: SA order): kSamplingSaOrder
    // keeps SA[0], SA[dens], ...; kSamplingTextOrder keeps SA[i] / dens of the marked i (SA[i] % dens == 0) in ascending i, and the marks
    // at off_marked as the byte index keeps them (n / 224 + 1 super-blocks {224 marks, ones before} over the SA indices)
    uint64_t sampling, off_marked;
};
static_assert(sizeof(IntHeader) <= 256, "the integer header is zero-padded to 256 bytes");
struct IntView {
    const Block* blocks;                              // plain: [n_levels][nb] wavelet matrix of the BWT over compact symbols
    const uint4* rrr_hdr;                             // rrr-63: [n_levels][n_sb] headers, the offset stream and the block code's tables
    const uint64_t* rrr_stream;                       //         (the members the bit-vector policies of device_rank.hpp read)
    const struct RrrTables* rrr_tables;
    uint64_t stride;                                  // super-blocks per level: nb (plain) or n_sb (rrr)
    uint32_t bv_kind, sampling;                       // kBvPlain / kBvRrr63; kSamplingSaOrder / kSamplingTextOrder
    const uint64_t* Z;                                // zeros per level
    const uint64_t* D;                                // C[c] - first position of c in the last arrangement
    const uint64_t* C;                                // [sigma + 1]
    const uint32_t* comp2char;                        // [sigma] ascending
    const uint32_t* samples;                          // SA[0], SA[dens], ... (SA order) or SA[i] / dens of the marked i (text order)
    uint64_t n, nb, sigma, n_samples;
    uint32_t n_levels, dens;
    const Block* marked;                              // text order: the marks over the SA indices (null in SA order)
};

constexpr uint32_t kBvPlain = 0, kBvRrr63 = 1;
constexpr uint32_t kSamplingSaOrder = 0, kSamplingTextOrder = 1;
constexpr uint32_t kRrrBlockBits = 63, kRrrBlocksPerSuper = 32, kRrrSuperBits = 63 * 32;

void set_error(const std::string& msg);
vlg_status fail(vlg_status st, const std::string& msg);
void release_cached_device_memory();      // result buffers parked for reuse (search.hip) go back to the driver

#define VLG_HIP_TRY(expr)                                                                        \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return ::vlg::fail(_e == hipErrorOutOfMemory ? VLG_E_OOM : VLG_E_NO_DEVICE,          \
                               std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

// Device scratch that frees itself: whatever a builder or an export allocates and does not hand to an index.  release() frees now
// (a builder lets its big arrays go as soon as no later stage reads them), take() hands the allocation to the object that owns it
// from then on.  An empty request still allocates (256 bytes), so that a buffer of an empty text is a pointer like any other.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 256);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void* take() { void* q = p; p = nullptr; cap = 0; return q; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
// rocPRIM's two calls -- call(nullptr, bytes) asks for the scratch size, call(scratch, bytes) runs -- around a scratch buffer that
// grows when a call wants more than it holds: a DevBuf, or any buffer with p, cap and alloc(bytes) (result_passes.hpp: CachedBuf)
template <class Buf, class Call>
hipError_t with_scratch(Buf& scratch, Call&& call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess && (!scratch.p || bytes > scratch.cap)) e = scratch.alloc(bytes);
    return e == hipSuccess ? call(scratch.p, bytes) : e;
}
// blocks of 256 threads for n items of a grid-stride kernel, at most `cap` and at least one
inline dim3 launch_grid(uint64_t n, uint32_t cap = 16384) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, cap))); }

// Host memory the batch path copies from / into.  Pageable vectors there are pinned by the runtime on the fly, and
// freeing them afterwards (munmap) makes the driver evict and restore the process's GPU queues: tens of ms in which the
// next kernel does not start.  These vectors live in pinned blocks owned by the workspace instead: handed out bump-style
// while a batch runs, recycled at the next batch, never unmapped in between.
struct HostPool {
    struct Blk { uint8_t* p; size_t cap; bool pinned; };
    std::vector<Blk> blocks;
    size_t cur = 0, off = 0;
    void* take(size_t bytes);              // 64-byte aligned; pageable blocks (kept just as long) when pinned memory cannot be had
    void reset() { cur = 0; off = 0; }
    void release();                        // back to the driver (workspace destruction)
};
HostPool*& host_pool_slot();               // pool of the batch this thread is running (nullptr outside a batch)
struct HostPoolScope {
    HostPool* prev;
    explicit HostPoolScope(HostPool* p) : prev(host_pool_slot()) { host_pool_slot() = p; p->reset(); }
    ~HostPoolScope() { host_pool_slot() = prev; }
};
template <class T>
struct StageAlloc {
    using value_type = T;
    StageAlloc() = default;
    template <class U> StageAlloc(const StageAlloc<U>&) {}
    T* allocate(size_t n)
    {
        HostPool* hp = host_pool_slot();
        void* p = hp ? hp->take(n * sizeof(T)) : nullptr;
        if (!p) throw std::bad_alloc();
        return (T*)p;
    }
    void deallocate(T*, size_t) noexcept {}
    template <class U> bool operator==(const StageAlloc<U>&) const { return true; }
    template <class U> bool operator!=(const StageAlloc<U>&) const { return false; }
};
template <class T> using svec = std::vector<T, StageAlloc<T>>;   // a vector whose storage is staged for device copies
// ... and one whose resize(n) leaves the new elements as they are (arrays that a device copy fills completely)
template <class T>
struct StageAllocRaw : StageAlloc<T> {
    using value_type = T;
    StageAllocRaw() = default;
    template <class U> StageAllocRaw(const StageAllocRaw<U>&) {}
    template <class U> struct rebind { using other = StageAllocRaw<U>; };
    template <class U> void construct(U*) noexcept {}
    template <class U, class... Args> void construct(U* p, Args&&... args) { ::new ((void*)p) U(std::forward<Args>(args)...); }
};
template <class T> using rvec = std::vector<T, StageAllocRaw<T>>;

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
inline uint32_t bit_width64(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

// bit_vector_il<512> of the paper's index tree (include/sdsl/bit_vector_il.hpp:113-150): sizes of a tree of n values and L levels
struct IlShape {
    uint64_t bits, data_words, superblocks, block_num, rank_samples;
};
inline IlShape il_shape(uint64_t n, uint32_t levels)
{
    IlShape s;
    s.bits = n * levels;
    s.data_words = (s.bits + 64) / 64;
    s.superblocks = (s.bits + 512) / 512;
    s.block_num = s.data_words + s.superblocks + 1;
    const uint64_t top = 1ull << (bit_width64(s.superblocks) - 1);                 // 1 << bits::hi(superblocks)
    s.rank_samples = s.block_num > 1024 * 64 ? (top < 1024 ? top : 1024) : 0;
    return s;
}
// m_rank_samples (init_rank_samples, bit_vector_il.hpp:87-104): count words of the superblocks met in the BFS order of a bisection
inline void il_rank_samples(const uint64_t* data, uint64_t superblocks, uint64_t count, uint64_t* out)
{
    std::vector<uint64_t> lbs{0}, rbs{superblocks};
    uint64_t idx = 0;
    for (size_t q = 0; q < lbs.size() && idx < count; ++q) {
        const uint64_t lb = lbs[q], rb = rbs[q], mid = lb + (rb - lb) / 2;
        out[idx++] = data[mid * 9];
        lbs.push_back(lb); rbs.push_back(mid);
        lbs.push_back(mid + 1); rbs.push_back(rb);
    }
}

// Host-side description of the tree, shared by from_parts and the device builder.
struct HostTree {
    uint32_t n_nodes = 0;
    uint32_t sigma = 0;
    uint32_t max_code_len = 0;
    std::vector<vlg_wt_node> nodes;     // reference layout
    std::vector<uint64_t> node_size;    // bits per inner node (0 for leaves)
    std::vector<uint32_t> node_depth;
    std::vector<uint64_t> paths;        // [256]
    std::vector<uint16_t> c_to_leaf;    // [256]
    std::vector<DNode> dnodes;          // device layout
    uint64_t wt_bits = 0;
    uint64_t n_blocks = 0;
    uint8_t char2comp[256];
    std::vector<uint64_t> C;            // [sigma+1]
};

// Huffman shape + BFS layout from symbol counts (restates wt_huff.hpp:91-117, wt_helper.hpp:170-241).
vlg_status tree_from_counts(const uint64_t counts[256], HostTree& t);
// Adopt reference nodes (from a loaded index).
vlg_status tree_from_nodes(const vlg_wt_node* nodes, uint32_t n_nodes, uint64_t bv_bits, const uint8_t* char2comp,
                           const uint64_t* C, uint32_t sigma, HostTree& t);

}  // namespace vlg

struct vlg_index {
    void* d_blob = nullptr;
    bool owns_blob = true;
    vlg::BlobHeader hdr;
    vlg::IndexView view;
    vlg::HostTree tree;   // host copy (node table, C, ...) for export and planning
    bool is_int = false;  // integer-alphabet FM-index (int_index.hpp): ihdr / iview are valid, hdr carries the generic fields only
    vlg::IntHeader ihdr;
    vlg::IntView iview;
    vlg::DevBuf quad;     // the quad image view.qnodes / view.qblocks point into (an allocation of its own, freed with the index)
    double quad_build_s = 0;
};

// Text access (kernels.hip: vlg_text_access_create, vlg_extract_batch, vlg_isa_batch; search.hip reads idx for the match texts)
struct vlg_text_access {
    const vlg_index* idx = nullptr;
    uint32_t d = 0;
    uint32_t isa_bytes = 0;                                        // isa_sample_bytes(n)
    void* d_isa = nullptr;                                         // ISA[0], ISA[d], ... ((n - 1) / d + 1 entries)
    uint8_t* d_c2c = nullptr;                                      // byte index: comp2char[256]
};

namespace vlg {
// an object under construction: its destroy function takes it, with what it owns by then, unless release() hands it to the caller
template <class T, void (*Destroy)(T*)> struct DestroyWith { void operator()(T* p) const { Destroy(p); } };
template <class T, void (*Destroy)(T*)> using Building = std::unique_ptr<T, DestroyWith<T, Destroy>>;
// (an index frees d_blob only where owns_blob is set: a fresh one holds no blob, and whoever points d_blob at memory of the caller's
// clears owns_blob in the same place -- the attach functions -- so a failure after that never frees the caller's blob)
using IndexPtr = Building<vlg_index, vlg_index_destroy>;
// the paper's index on disk (wtsa_sdsl.hpp): m_text packed to `width` bits (in: 0 = the index's own width; out: the width used), and
// bit_vector_il<512>::m_data of the tree, both converted on the device and copied to the host
vlg_status wtsa_text_words(const vlg_wtsa* idx, uint32_t& width, std::vector<uint64_t>& words);
vlg_status wtsa_il_words(const vlg_wtsa* idx, std::vector<uint64_t>& words);
vlg_status derive_quad_image(vlg_index* idx, hipStream_t stream);                 // index.hip: what every maker of a plain byte index ends with
vlg_status attach_int_blob(const void* d_blob, uint64_t bytes, vlg_index* idx);   // int_index.hpp
void layout_int_blob(IntHeader& h);                                               // int_index.hpp: offsets and total_bytes from the sizes
}
