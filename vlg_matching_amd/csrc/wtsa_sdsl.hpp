// The paper's index on disk (vlg_hip.h: vlg_wtsa_from_parts, vlg_wtsa_il_device; the file itself is read and written by
// sdsl_format.cpp): the device side of vlg_index<alphabet_tag, wt_int<bit_vector_il<>, rank_support_il<>>>.
//   vlg_index::serialize           include/sdsl/vlg_index.hpp:181-198    m_text, then m_wt
//   wt_int::serialize              include/sdsl/wt_int.hpp:708-732       size, sigma, tree, (empty supports), max_level
//   bit_vector_il<512>             include/sdsl/bit_vector_il.hpp:113-150 m_data: a cumulative count word before every 8 data words
//                                                                          (data word i at i + i / 8 + 1), the total ones last
// Internal to search.hip's translation unit; included exactly once, behind wtsa.hpp (whose view, block layout and count pass it uses).
//
// The device tree keeps level l as its own run of 32-byte Blocks {7 x u32 data, u32 ones before the block inside the level}; the file
// keeps the levels back to back as ONE bit-vector of S = n * L bits.  Bit g of the file's tree is bit g - l * n of level l = g / n.
// Both directions run one lane per output word and compute every read position from n and L alone -- never from a value read from
// the file -- so a damaged file is caught by a check, not by a fault.  Bit positions reach n * L ~ 3.3e10 on a 1 GiB text: 64-bit.
//   save  one pass: one lane per data word assembles 64 tree bits (one level, or the end of one and the start of the next -- more when
//         n < 64).  A count word is the number of ones before its superblock, which the device tree already knows: the ones of the
//         levels before (L + 1 prefix sums made with the tree) plus one rank inside the level -- so the first lane of every 8 writes it, and no
//         scan over the popcounts of the data words is needed.
//   load  one lane per Block gathers its 224 bits from the data words, the per-block popcounts go through the build's own count pass
//         (exclusive scan + wtsa_counts_kernel); then one lane per superblock checks its count word against the same rank.
#pragma once

namespace {

__device__ __forceinline__ uint64_t il_index(uint64_t i) { return i + i / 8 + 1; }     // data word i in m_data

// bits [bit, bit + cnt) of one level (cnt <= 64, bit + cnt <= n) from its Blocks
__device__ __forceinline__ uint64_t wtsa_level_bits(const Block* __restrict__ lb, uint64_t bit, uint32_t cnt)
{
    uint64_t v = 0;
    for (uint32_t got = 0; got < cnt;) {
        const uint64_t blk = bit / kBlockBits;
        const uint32_t r = (uint32_t)(bit - blk * kBlockBits), wi = r >> 5, sh = r & 31;
        const uint32_t take = min(32u - sh, cnt - got);
        const uint64_t piece = (uint64_t)(lb[blk].w[wi] >> sh) & ((1ull << take) - 1);
        v |= piece << got;
        got += take;
        bit += take;
    }
    return v;
}

// tree bits [g, g + 64) of the level concatenation (g = lvl * n + off), 0 past S = n * L
__device__ __forceinline__ uint64_t wtsa_tree_word(const WtsaView& w, uint64_t lvl, uint64_t off)
{
    const uint64_t n = w.n_vals;
    uint64_t v = 0;
    for (uint32_t got = 0; got < 64 && lvl < w.levels; ++lvl, off = 0) {
        const uint64_t left = n - off;
        const uint32_t take = left < 64 - got ? (uint32_t)left : 64 - got;
        v |= wtsa_level_bits(w.blocks + lvl * w.nb, off, take) << got;
        got += take;
    }
    return v;
}

// ones of the tree before bit g = lvl * n + off: the levels before it (prefix[lvl]) and the rank inside its level, read off the device
// tree's own counts -- so every count word of m_data is ONE rank, and no pass over the data words is needed to scan their popcounts
__device__ __forceinline__ uint64_t wtsa_ones_before(const WtsaView& w, const uint64_t* __restrict__ prefix, uint64_t lvl, uint64_t off)
{
    if (lvl >= w.levels) return prefix[w.levels];
    return prefix[lvl] + (off ? node_rank1(w.blocks, (uint32_t)(lvl * w.nb), off) : 0);
}

// prefix[l] = ones of the levels before l (prefix[L] = all of them); one lane
__global__ void wtsa_level_prefix_kernel(WtsaView w, uint64_t* __restrict__ prefix)
{
    if (blockIdx.x || threadIdx.x) return;
    uint64_t acc = 0;
    for (uint32_t l = 0; l < w.levels; ++l) {
        prefix[l] = acc;
        acc += node_rank1(w.blocks, (uint32_t)(l * w.nb), w.n_vals);
    }
    prefix[w.levels] = acc;
}

// save: one lane per data word of m_data; the first lane of every 8 also writes its superblock's count word, the last one the final word
__global__ void __launch_bounds__(256) wtsa_il_fill_kernel(WtsaView w, const uint64_t* __restrict__ prefix, uint64_t data_words,
                                                           uint64_t superblocks, uint64_t* __restrict__ img)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < data_words; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = i * 64, lvl = g / w.n_vals, off = g - lvl * w.n_vals;
        img[il_index(i)] = wtsa_tree_word(w, lvl, off);
        if ((i & 7) == 0) img[9 * (i >> 3)] = wtsa_ones_before(w, prefix, lvl, off);
        if (i + 1 == data_words) img[data_words + superblocks] = prefix[w.levels];
    }
}

// load, once the device tree is complete: every count word and the final word must be the ones before them (flag bit 1), and the bits
// of the last data word past S must be 0 (flag bit 0) -- with that the count words are the running popcount of the file's data words
__global__ void __launch_bounds__(256) wtsa_il_check_kernel(WtsaView w, const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ img,
                                                            uint64_t data_words, uint64_t superblocks, unsigned* __restrict__ flag)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < superblocks; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = k * 512, lvl = g / w.n_vals, off = g - lvl * w.n_vals;
        if (img[9 * k] != wtsa_ones_before(w, prefix, lvl, off)) atomicOr(flag, 2u);
        if (k == 0) {
            if (img[data_words + superblocks] != prefix[w.levels]) atomicOr(flag, 2u);
            const uint64_t S = w.n_vals * w.levels, last = (data_words - 1) * 64;     // the one data word that reaches past S
            if (img[il_index(data_words - 1)] >> (S - last)) atomicOr(flag, 1u);    // (S - last < 64: data_words = S / 64 + 1)
        }
    }
}

// load: one lane per Block of the device tree gathers its 224 bits from the data words; pops[level * (nb + 1) + b] = its ones
__global__ void __launch_bounds__(256) wtsa_il_gather_kernel(const uint64_t* __restrict__ img, uint64_t n, uint32_t levels, uint64_t nb,
                                                             Block* __restrict__ blocks, uint32_t* __restrict__ pops)
{
    const uint64_t total = (uint64_t)levels * nb;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t lvl = t / nb, b = t - lvl * nb;
        Block B;
        uint32_t pop = 0;
#pragma unroll
        for (uint32_t wi = 0; wi < 7; ++wi) {
            const uint64_t bit = b * kBlockBits + 32ull * wi;
            uint32_t word = 0;
            if (bit < n) {
                const uint32_t cnt = n - bit < 32 ? (uint32_t)(n - bit) : 32u;
                const uint64_t g = lvl * n + bit, di = g >> 6;
                const uint32_t o = (uint32_t)(g & 63);
                uint64_t v = img[il_index(di)] >> o;
                if (o + cnt > 64) v |= img[il_index(di + 1)] << (64 - o);            // (g + cnt - 1 < S: a data word of the file)
                word = (uint32_t)(v & ((1ull << cnt) - 1));
            }
            B.w[wi] = word;
            pop += (uint32_t)__popc(word);
        }
        B.cnt = 0;
        blocks[t] = B;
        pops[lvl * (nb + 1) + b] = pop;
    }
}

// the last entry of every level's scanned counts: the ones of the level
__global__ void wtsa_level_ones_kernel(const uint32_t* __restrict__ pops, uint32_t levels, uint64_t nb, uint64_t* __restrict__ out)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < levels) out[l] = pops[(uint64_t)l * (nb + 1) + nb];
}

// byte text: flag bit 0 on a 0 byte
__global__ void wtsa_zero_byte_kernel(const uint8_t* __restrict__ t, uint64_t n, unsigned* __restrict__ flag)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (t[i] == 0) atomicOr(flag, 1u);
}

// int_vector<0> of width w -> uint32_t; flag bit 0 on a value >= 2^32
__global__ void wtsa_unpack_kernel(const uint64_t* __restrict__ words, uint64_t count, uint32_t width, uint32_t* __restrict__ out,
                                   unsigned* __restrict__ flag)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t bit = i * width, wd = bit >> 6;
        const uint32_t o = (uint32_t)(bit & 63);
        uint64_t v = words[wd] >> o;
        if (o + width > 64) v |= words[wd + 1] << (64 - o);
        if (width < 64) v &= (1ull << width) - 1;
        if (v >> 32) atomicOr(flag, 1u);
        out[i] = (uint32_t)v;
    }
}

// uint32_t -> int_vector<0> of width w: one lane per output word (the symbols were checked to fit)
__global__ void wtsa_pack_kernel(const uint32_t* __restrict__ syms, uint64_t count, uint32_t width, uint64_t* __restrict__ words, uint64_t n_words)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_words; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t lo = t * 64, hi = lo + 64;
        uint64_t word = 0;
        for (uint64_t i = lo / width; i < count && i * width < hi; ++i) {
            const uint64_t v = syms[i], bit = i * width;
            word |= bit >= lo ? v << (bit - lo) : v >> (lo - bit);
        }
        words[t] = word;
    }
}

__global__ void wtsa_max_kernel(const uint32_t* __restrict__ syms, uint64_t count, unsigned* __restrict__ out)
{
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) m = max(m, syms[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_down(m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// x->d_level_prefix, once the device tree is complete (vlg_wtsa_build, vlg_wtsa_from_parts)
vlg_status wtsa_level_prefix(vlg_wtsa* x)
{
    DevBuf d_prefix;
    VLG_HIP_TRY(d_prefix.alloc(((uint64_t)x->levels + 1) * 8));
    x->d_level_prefix = static_cast<uint64_t*>(d_prefix.take());
    hipLaunchKernelGGL(wtsa_level_prefix_kernel, dim3(1), dim3(64), 0, nullptr, wtsa_view(x), x->d_level_prefix);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

vlg_status wtsa_il_device_impl(const vlg_wtsa* x, uint64_t* d_words, hipStream_t st)
{
    const IlShape s = il_shape(x->n_vals, x->levels);
    hipLaunchKernelGGL(wtsa_il_fill_kernel, launch_grid(s.data_words, 1u << 20), dim3(256), 0, st, wtsa_view(x), (const uint64_t*)x->d_level_prefix,
                       s.data_words, s.superblocks, d_words);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;                                                  // asynchronous on `st`
}

}  // namespace

extern "C" vlg_status vlg_wtsa_il_device(const vlg_wtsa* x, uint64_t* d_words, uint64_t n_words, void* stream)
{
    if (!x || !d_words) return fail(VLG_E_INVALID, "null argument");
    if (n_words < il_shape(x->n_vals, x->levels).block_num) return fail(VLG_E_INVALID, "d_words holds fewer than block_num words");
    return wtsa_il_device_impl(x, d_words, (hipStream_t)stream);
}

vlg_status vlg::wtsa_il_words(const vlg_wtsa* x, std::vector<uint64_t>& words)
{
    const IlShape s = il_shape(x->n_vals, x->levels);
    DevBuf d;
    VLG_HIP_TRY(d.alloc(s.block_num * 8));
    if (vlg_status r = wtsa_il_device_impl(x, d.as<uint64_t>(), nullptr)) return r;
    try { words.resize(s.block_num); }
    catch (const std::bad_alloc&) { return fail(VLG_E_OOM, "out of host memory for the tree image"); }
    VLG_HIP_TRY(hipMemcpy(words.data(), d.p, s.block_num * 8, hipMemcpyDeviceToHost));   // (on the null stream, after the fill)
    return VLG_OK;
}

vlg_status vlg::wtsa_text_words(const vlg_wtsa* x, uint32_t& width, std::vector<uint64_t>& words)
{
    const uint64_t count = x->n_text;
    if (x->sym_bytes == 1) {
        if (width != 0 && width != 8) return fail(VLG_E_INVALID, "a byte index stores its text as int_vector<8>: text_width must be 0 or 8");
        width = 8;
        try { words.assign((count + 7) / 8, 0); }
        catch (const std::bad_alloc&) { return fail(VLG_E_OOM, "out of host memory for the text"); }
        if (count) VLG_HIP_TRY(hipMemcpy(words.data(), x->d_text, count, hipMemcpyDeviceToHost));
        return VLG_OK;
    }
    if (width > 64) return fail(VLG_E_INVALID, "text_width must be 0..64");
    DevBuf d_max, d;
    VLG_HIP_TRY(d_max.alloc(4));
    unsigned mx = 0;
    VLG_HIP_TRY(hipMemset(d_max.p, 0, 4));
    if (count) {
        hipLaunchKernelGGL(wtsa_max_kernel, launch_grid(count, 4096), dim3(256), 0, nullptr, (const uint32_t*)x->d_text, count, d_max.as<unsigned>());
        VLG_HIP_TRY(hipGetLastError());
    }
    VLG_HIP_TRY(hipMemcpy(&mx, d_max.p, 4, hipMemcpyDeviceToHost));
    const uint32_t need = std::max(1u, bit_width64(mx));
    if (!width) width = x->file_width ? x->file_width : need;
    if (width < need)
        return fail(VLG_E_INVALID, "symbol " + std::to_string(mx) + " does not fit a text width of " + std::to_string(width) + " bits");
    const uint64_t n_words = (count * width + 63) / 64;
    try { words.assign(n_words, 0); }
    catch (const std::bad_alloc&) { return fail(VLG_E_OOM, "out of host memory for the text"); }
    if (!n_words) return VLG_OK;
    VLG_HIP_TRY(d.alloc(n_words * 8));
    hipLaunchKernelGGL(wtsa_pack_kernel, launch_grid(n_words, 8192), dim3(256), 0, nullptr, (const uint32_t*)x->d_text, count, width, d.as<uint64_t>(), n_words);
    VLG_HIP_TRY(hipGetLastError());
    VLG_HIP_TRY(hipMemcpy(words.data(), d.p, n_words * 8, hipMemcpyDeviceToHost));
    return VLG_OK;
}

extern "C" vlg_status vlg_wtsa_from_parts(const vlg_wtsa_parts* p, vlg_wtsa** out)
{
    if (!p || !out) return fail(VLG_E_INVALID, "null argument");
    *out = nullptr;
    // ---- the sizes, on the host: everything the kernels read is at a position computed from n and L -------------------------------
    if (p->symbol_bytes != 1 && p->symbol_bytes != 4) return fail(VLG_E_INVALID, "symbol_bytes must be 1 or 4");
    const uint64_t n = p->n;
    if (n == 0) return fail(VLG_E_INVALID, "n = 0: the tree holds at least the sentinel's suffix");
    if (n > 0xFFFFFFF0ull) return fail(VLG_E_UNSUPPORTED, "more than 2^32 - 16 suffixes: the device tree counts in 32 bits");
    const uint32_t L = bit_width64(std::max<uint64_t>(n - 1, 1));
    if (p->levels != L) return fail(VLG_E_INVALID, "levels " + std::to_string(p->levels) + " != hi(max(n - 1, 1)) + 1 = " + std::to_string(L));
    if (p->text_count != n - 1) return fail(VLG_E_INVALID, "the text does not hold n - 1 symbols");
    const uint32_t w = p->text_width;
    if (p->symbol_bytes == 1 ? w != 8 : (w < 1 || w > 64)) return fail(VLG_E_INVALID, "text width " + std::to_string(w) + " does not fit the alphabet");
    const IlShape s = il_shape(n, L);
    if (p->data_words != s.block_num) return fail(VLG_E_INVALID, "m_data does not hold block_num words");
    if (p->n_rank_samples != s.rank_samples) return fail(VLG_E_INVALID, "wrong number of rank samples");
    if (!p->data || (p->text_count && !p->text_words) || (s.rank_samples && !p->rank_samples)) return fail(VLG_E_INVALID, "null part");
    if (s.rank_samples) {
        std::vector<uint64_t> want(s.rank_samples);
        il_rank_samples(p->data, s.superblocks, s.rank_samples, want.data());
        if (memcmp(want.data(), p->rank_samples, s.rank_samples * 8)) return fail(VLG_E_INVALID, "the rank samples are not the count words they copy");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VLG_E_NO_DEVICE, "no HIP device available (the VLG library has no CPU fallback)");
    release_cached_device_memory();
    WtsaPtr x(new vlg_wtsa());
    x->n_text = n - 1; x->n_vals = n; x->sym_bytes = p->symbol_bytes; x->levels = L;
    x->nb = n / kBlockBits + 1;
    x->file_width = p->symbol_bytes == 4 ? w : 0;
    DevBuf d_flag_buf, d_text, d_words, d_img, d_blocks, d_pops_buf, d_tmp, d_ones;
    auto run = [&]() -> vlg_status {                                 // (host vectors in here: std::bad_alloc becomes a status below)
        const uint64_t count = n - 1, nb = x->nb;
        VLG_HIP_TRY(d_flag_buf.alloc(16));
        unsigned* d_flag = d_flag_buf.as<unsigned>();
        VLG_HIP_TRY(hipMemset(d_flag, 0, 16));
        // ---- text ----------------------------------------------------------------------------------------------------------------------
        VLG_HIP_TRY(d_text.alloc(count * x->sym_bytes));
        x->d_text = d_text.take();
        if (x->sym_bytes == 1) {
            if (count) {
                VLG_HIP_TRY(hipMemcpy(x->d_text, p->text_words, count, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(wtsa_zero_byte_kernel, launch_grid(count, 8192), dim3(256), 0, nullptr, (const uint8_t*)x->d_text, count, d_flag);
                VLG_HIP_TRY(hipGetLastError());
            }
        } else if (count) {
            const uint64_t nw = (count * w + 63) / 64;
            VLG_HIP_TRY(d_words.alloc(nw * 8));
            VLG_HIP_TRY(hipMemcpy(d_words.p, p->text_words, nw * 8, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(wtsa_unpack_kernel, launch_grid(count, 8192), dim3(256), 0, nullptr, d_words.as<uint64_t>(), count, w, (uint32_t*)x->d_text, d_flag + 1);
            VLG_HIP_TRY(hipGetLastError());
        }
        // ---- the tree ------------------------------------------------------------------------------------------------------------------
        VLG_HIP_TRY(d_img.alloc(s.block_num * 8));
        VLG_HIP_TRY(hipMemcpy(d_img.p, p->data, s.block_num * 8, hipMemcpyHostToDevice));
        VLG_HIP_TRY(d_blocks.alloc((uint64_t)L * nb * sizeof(Block)));
        x->d_blocks = static_cast<Block*>(d_blocks.take());
        VLG_HIP_TRY(d_pops_buf.alloc((uint64_t)L * (nb + 1) * 4));
        uint32_t* d_pops = d_pops_buf.as<uint32_t>();
        VLG_HIP_TRY(hipMemset(d_pops, 0, (uint64_t)L * (nb + 1) * 4));
        hipLaunchKernelGGL(wtsa_il_gather_kernel, launch_grid((uint64_t)L * nb), dim3(256), 0, nullptr, d_img.as<uint64_t>(), n, L, nb,
                           x->d_blocks, d_pops);
        VLG_HIP_TRY(hipGetLastError());
        for (uint32_t lvl = 0; lvl < L; ++lvl)
            if (vlg_status r = wtsa_level_counts(x->d_blocks + (uint64_t)lvl * nb, nb, d_pops + (uint64_t)lvl * (nb + 1), d_tmp)) return r;
        VLG_HIP_TRY(d_ones.alloc((uint64_t)L * 8));
        hipLaunchKernelGGL(wtsa_level_ones_kernel, dim3(1), dim3(64), 0, nullptr, d_pops, L, nb, d_ones.as<uint64_t>());
        VLG_HIP_TRY(hipGetLastError());
        // the count words against the tree just built
        if (vlg_status r = wtsa_level_prefix(x.get())) return r;
        hipLaunchKernelGGL(wtsa_il_check_kernel, launch_grid(s.superblocks), dim3(256), 0, nullptr, wtsa_view(x.get()), (const uint64_t*)x->d_level_prefix,
                           d_img.as<uint64_t>(), s.data_words, s.superblocks, d_flag + 2);
        VLG_HIP_TRY(hipGetLastError());
        std::vector<uint64_t> ones(L);
        unsigned flags[4] = {0, 0, 0, 0};
        VLG_HIP_TRY(hipMemcpy(ones.data(), d_ones.p, (uint64_t)L * 8, hipMemcpyDeviceToHost));
        VLG_HIP_TRY(hipMemcpy(flags, d_flag, 16, hipMemcpyDeviceToHost));
        // ---- the checks --------------------------------------------------------------------------------------------------------------
        if (flags[0]) return fail(VLG_E_ZERO_BYTE, "the byte text holds a 0 byte (construct.hpp:36-45)");
        if (flags[1]) return fail(VLG_E_UNSUPPORTED, "a symbol >= 2^32: the device index holds uint32_t symbols");
        if (flags[2] & 1) return fail(VLG_E_INVALID, "bits past n * max_level are set in the tree");
        if (flags[2] & 2) return fail(VLG_E_INVALID, "a cumulative count word of the tree is not the running popcount");
        for (uint32_t lvl = 0; lvl < L; ++lvl) {
            const uint32_t b = L - 1 - lvl;                          // values v in [0, n) with bit b set
            const uint64_t period = 1ull << (b + 1), half = 1ull << b, rem = n % period;
            const uint64_t want = (n / period) * half + (rem > half ? rem - half : 0);
            if (ones[lvl] != want)
                return fail(VLG_E_INVALID, "level " + std::to_string(lvl) + " holds " + std::to_string(ones[lvl]) + " ones, a suffix array's tree " +
                                               std::to_string(want));
        }
        return VLG_OK;
    };
    vlg_status st;
    try { st = run(); }
    catch (const std::bad_alloc&) { st = fail(VLG_E_OOM, "out of host memory"); }
    if (st) return st;
    *out = x.release();
    return VLG_OK;
}
