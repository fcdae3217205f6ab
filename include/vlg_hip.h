/* include/vlg_hip.h -- C-ABI of the MI355X-native variable-length-gap (VLG) matcher.
 *
 * This is the drop-in boundary for the FM-index VLG hot path of olydis/vlg_matching
 * (an sdsl-lite fork).  The reference has no FFI: the path sits behind C++ template concepts
 * (SURVEY.md 8b).  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference root); INTEGRATION.md shows the C++ adapter a reference
 * maintainer would add to route `index_*::search` / `sdsl::locate` through it.
 *
 * Conventions
 *   - plain C, no exceptions: every call returns a vlg_status; vlg_last_error() gives the text.
 *   - "h_" arguments are host pointers, "d_" arguments are device (HBM) pointers of the current
 *     HIP device; the caller owns every buffer it passes in.
 *   - positions/counts are uint64_t at the boundary, like sdsl's size_type; all arithmetic is
 *     unsigned integer / bit manipulation (no floating point anywhere on the path).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - a vlg_index is immutable after creation; batched calls on different streams may share it.
 *     A vlg_workspace / vlg_result belongs to one caller thread at a time.
 *   - there is no CPU fallback: without a usable HIP device every compute call fails with
 *     VLG_E_NO_DEVICE.
 */
#ifndef VLG_HIP_H
#define VLG_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    VLG_OK = 0,
    VLG_E_INVALID = 1,       /* bad argument                                                   */
    VLG_E_NO_DEVICE = 2,     /* no HIP device / HIP runtime error                              */
    VLG_E_OOM = 3,           /* device or host allocation failed                               */
    VLG_E_PARSE = 4,         /* gap syntax: the reference throws std::runtime_error
                                (include/sdsl/vlg_index.hpp:92-99)                             */
    VLG_E_ZERO_BYTE = 5,     /* text contains a 0 byte: std::logic_error in the reference
                                (include/sdsl/construct.hpp:36-45)                             */
    VLG_E_UNSUPPORTED = 6,   /* e.g. text longer than this build handles                       */
    VLG_E_WORKSPACE = 7,     /* one query needs more workspace than the configured cap          */
    VLG_E_INTERNAL = 8
} vlg_status;

typedef struct vlg_index vlg_index;          /* FM-index resident in HBM                       */
typedef struct vlg_bitvector vlg_bitvector;  /* stand-alone rank-enabled bit-vector in HBM     */
typedef struct vlg_queries vlg_queries;      /* a parsed query batch resident in HBM           */
typedef struct vlg_result vlg_result;        /* results of one vlg_search_batch, in HBM        */
typedef struct vlg_workspace vlg_workspace;  /* scratch HBM + stream + per-kernel statistics   */

const char* vlg_last_error(void);            /* thread-local text of the last failure          */
const char* vlg_version(void);
vlg_status vlg_device_count(int* n);
vlg_status vlg_set_device(int ordinal);

/* ------------------------------------------------------------------------------------------
 * Index parts in the REFERENCE's own layout (host memory) -- what a loaded
 * sdsl::csa_wt<wt_huff<>,32,64> exposes (include/sdsl/csa_wt.hpp:120-152):
 *   wavelet_tree.bv (wt_pc.hpp:185), the _byte_tree nodes (wt_helper.hpp:73-131, BFS order),
 *   char2comp / C (csa_wt.hpp:139-142), sa_sample (csa_wt.hpp:150; csa_sampling_strategy.hpp:85-111).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t bv_pos;        /* inner node: first bit of the node in wavelet_tree.bv             */
    uint64_t bv_pos_rank;   /* inner node: rank1(bv_pos); leaf: the symbol                      */
    uint16_t parent;        /* 0xFFFF for the root                                             */
    uint16_t child[2];      /* 0xFFFF,0xFFFF for a leaf                                        */
} vlg_wt_node;

typedef struct {
    uint64_t n;                   /* csa.size() = |text| + 1 (sentinel)                         */
    uint32_t sigma;               /* csa.sigma                                                 */
    uint32_t sa_sample_dens;      /* t_dens, 32 in the reference default (csa_wt.hpp:61)        */
    const uint8_t* char2comp;     /* [256]                                                     */
    const uint64_t* C;            /* [sigma+1]                                                 */
    const uint64_t* bv_words;     /* ceil(bv_bits/64) words, bit i = word[i>>6] >> (i&63)      */
    uint64_t bv_bits;
    const vlg_wt_node* nodes;     /* [n_nodes], node 0 = root                                  */
    uint32_t n_nodes;             /* 2*sigma-1                                                 */
    const uint64_t* sa_samples;   /* [ceil(n/dens)] unpacked: SA[0], SA[dens], ...              */
    uint64_t n_samples;
} vlg_index_parts;

typedef struct {
    uint64_t n;                   /* text length + 1                                           */
    uint32_t sigma;
    uint32_t sa_sample_dens;
    uint32_t n_nodes;
    uint32_t max_code_len;        /* deepest leaf of the Huffman-shaped tree                    */
    uint64_t wt_bits;             /* sum of node sizes = n * (mean code length)                 */
    uint64_t n_blocks;            /* 32-byte super-blocks in HBM                               */
    uint64_t n_samples;
    uint64_t hbm_bytes;           /* total device bytes of the index                           */
    uint32_t pos_bytes;           /* 4 (n <= 2^32) or 8: width of SA samples / SA indices; text positions inside the
                                     kernels are 32-bit up to n = 2^32 + 1 whatever this says     */
    uint32_t bv_kind;             /* VLG_BV_PLAIN or VLG_BV_RRR63                               */
    uint32_t sampling;            /* VLG_SAMPLING_SA_ORDER or VLG_SAMPLING_TEXT_ORDER           */
    uint32_t reserved;
} vlg_index_info;

/* Build on the device from raw text (no 0 byte; the sentinel is appended like
 * sdsl::construct, include/sdsl/construct.hpp:47-52,112-159): suffix sort, BWT, Huffman-shaped
 * wavelet tree (wt_pc.hpp:197-248), SA sampling -- all in HBM.  Replaces
 * `index_*(collection&)` (benchmark/gapped-matching/include/index_sasearch.hpp:23-31) and
 * `construct(idx, file, num_bytes)` (include/sdsl/vlg_index.hpp:375-392). */
vlg_status vlg_index_build(const uint8_t* h_text, uint64_t n_text, uint32_t sa_sample_dens, vlg_index** out);
/* Same, text already in HBM.  Synchronises `stream`: the index is complete on return. */
vlg_status vlg_index_build_device(const uint8_t* d_text, uint64_t n_text, uint32_t sa_sample_dens,
                                  void* stream, vlg_index** out);
/* Adopt an index built by the reference (host arrays in its layout) -- replaces
 * `idx.load(istream)` (index_sasearch.hpp:41-45; csa_wt.hpp:395-407).
 * Limits: n <= 2^36, and no wavelet-tree node may hold 2^32 or more 1-bits (the super-block counts are 32-bit and
 * node-relative): always true for n <= 2^32, otherwise checked against the symbol counts -> VLG_E_UNSUPPORTED. */
vlg_status vlg_index_from_parts(const vlg_index_parts* h_parts, vlg_index** out);
/* Export to the reference layout (two-phase: pass NULL buffers in `out` to get sizes only). -- replaces
 * `idx.serialize(ostream)` (index_sasearch.hpp:33-39).  Buffers in `out` are caller-allocated host arrays. */
typedef struct {
    uint8_t* char2comp;           /* [256]                                                     */
    uint64_t* C;                  /* [257]                                                     */
    uint64_t* bv_words;           /* [ceil(bv_bits/64)]                                        */
    vlg_wt_node* nodes;           /* [n_nodes]                                                 */
    uint64_t* sa_samples;         /* [n_samples]                                               */
} vlg_index_parts_out;
vlg_status vlg_index_export_parts(const vlg_index* idx, vlg_index_parts* sizes, vlg_index_parts_out* out);
/* A second index over the same text whose wavelet-tree bit-vectors are H0-compressed -- csa_wt<wt_huff<rrr_vector<63>>>
 * (BASELINE config 5; include/sdsl/rrr_vector.hpp).  Every search entry point accepts it and returns identical results.
 * Blocks of 63 bits are stored as a 6-bit class and an offset of ceil(log2 C(63,k)) bits -- the sizes of rrr_vector<63>; the
 * offset numbers the blocks of a class by halves (csrc/rrr_code.hpp) instead of bit by bit, so that a rank decodes in a fixed
 * short sequence of table lookups.  The device image is this library's own (blob magic "VGLB2"); a stock
 * csa_wt<wt_huff<rrr_vector<63>>> file is read by vlg_index_load_sdsl_kind, which decodes its blocks and ends here.  `src` must be
 * a plain index.  An integer-alphabet index (vlg_index_build_int) is compressed the same way, level by level of its wavelet matrix:
 * csa_wt<wt_int<rrr_vector<63>>, ., ., ., ., int_alphabet<>> (test/csa_int_test.cpp:32); vlg_index_info then says
 * VLG_BV_INT_MATRIX_RRR63. */
#define VLG_BV_PLAIN 0
#define VLG_BV_RRR63 1
#define VLG_BV_INT_MATRIX 2          /* integer-alphabet index (vlg_index_build_int): bv_kind of vlg_index_info */
#define VLG_BV_INT_MATRIX_RRR63 3    /* ... with rrr-63 levels (vlg_index_compress of one) */
vlg_status vlg_index_compress(const vlg_index* src, int bv_kind, vlg_index** out);
/* The other SA sampling strategy of the reference, and other densities: a second index over the same BWT whose SA samples are
 *   VLG_SAMPLING_SA_ORDER    SA[0], SA[d], SA[2d], ...                   sa_order_sa_sampling, csa_wt's default
 *                            (include/sdsl/csa_sampling_strategy.hpp:64-112)
 *   VLG_SAMPLING_TEXT_ORDER  the SA values that are multiples of d, found through a marked bit-vector over the SA indices:
 *                            is_sampled(i) = marked[i], csa[i] = samples[rank_marked(i)] * d   text_order_sa_sampling (:127-246) --
 *                            the locate indexes of benchmark/indexing_locate/index.config:9-12; a walk takes SA[i] % d LF steps
 * Every search entry point accepts it and returns identical results.  `src` must be SA-order sampled (plain or rrr); the new index keeps
 * its samples as wide as the source does (8 bytes when SA indices need 33 bits: n > 2^32, or VLG_FORCE_POS64);
 * VLG_SAMPLING_SA_ORDER with d = 1 (also vlg_index_build* with sa_sample_dens = 1, any n) keeps the whole suffix array in HBM
 * (csa_wt<wt_huff<>, 1, .>: 4 B per text character up to 4 GiB of text, 8 B beyond): csa[i] is one read (csa_wt.hpp:335-348 with
 * zero LF steps), vlg_search_batch's locate stage becomes a coalesced copy of the SA intervals and keeps no trail table;
 * for a text-order index vlg_index_export_parts' sa_samples receives the condensed values SA / d, vlg_index_export_marked the
 * marks (bit i = h_words[i >> 6] >> (i & 63), ceil(n / 64) words).
 * An integer-alphabet index (vlg_index_build_int, plain or compressed) is resampled under the same rules and statuses --
 * csa_wt<wt_int<>, d, ., text_order_sa_sampling<>, ., int_alphabet<>> (test/csa_int_test.cpp:34), or SA order at another density; its
 * samples stay 4 bytes wide, its suffix array is expanded on the device by LF walks on the wavelet matrix, and at SA order d = 1 its
 * locate stage is the same copy of SA intervals whatever the alphabet size.  A text-order integer index is not compressed
 * (VLG_E_INVALID: compress first, then resample); vlg_index_export_marked gives its marks, vlg_index_info reports its sampling.
 * vlg_index_export_marked refuses an SA-order index of either alphabet (VLG_E_INVALID). */
#define VLG_SAMPLING_SA_ORDER 0
#define VLG_SAMPLING_TEXT_ORDER 1
vlg_status vlg_index_resample(const vlg_index* src, int sampling, uint32_t sa_sample_dens, vlg_index** out);
vlg_status vlg_index_export_marked(const vlg_index* idx, uint64_t* h_words);
vlg_status vlg_index_get_info(const vlg_index* idx, vlg_index_info* info);

/* FM-index of an INTEGER text -- csa_wt<wt_int<>, dens, ., sa_order_sa_sampling, ., int_alphabet<>>, the csa the reference builds for
 * vlg_index<int_alphabet_tag> (include/sdsl/vlg_index.hpp:383-384) and its word-level experiments: int_alphabet
 * (include/sdsl/csa_alphabet_strategy.hpp:394-470), BWT in a level-wise tree (wt_int.hpp; here a wavelet matrix over the compact
 * symbols: one super-block read per level), LF / csa[i] / backward_search as for bytes.  h_text: n_symbols uint32_t, none of them 0
 * (VLG_E_ZERO_BYTE: construct.hpp:36-45); n_symbols < 2^32 / 5.  The handle is a vlg_index: vlg_search_batch (with a batch parsed
 * by vlg_queries_parse_int), vlg_queries_intervals / _occurrences, vlg_backward_search_batch (patterns = little-endian uint32_t
 * symbols), vlg_sa_batch, vlg_locate_batch, blob export / attach / broadcast take it; the byte-only entry points refuse it.
 * vlg_index_compress (rrr-63 levels), vlg_index_resample (text-order sampling, other densities, the resident suffix array at d = 1),
 * vlg_index_export_marked and vlg_index_isa_samples take it too, under the byte index's rules. */
vlg_status vlg_index_build_int(const uint32_t* h_text, uint64_t n_symbols, uint32_t sa_sample_dens, vlg_index** out);
/* 64-bit symbols.  gapped_pattern_query<int_alphabet_tag> reads uint64_t tokens (vlg_index.hpp:57-69) and int_vector<64> texts hold
 * 64-bit symbols; the device indexes (vlg_index_build_int, vlg_wtsa_build_int) hold uint32_t.  A symbol map carries the sorted
 * distinct symbols of a 64-bit text and sends a symbol to its rank + 1: dense, order-preserving, never 0 -- so the suffix order, every
 * SA interval and every result of the mapped text are those of the original.  vlg_symbol_map_apply maps a text (or any symbols:
 * one that does not occur in the map's text becomes sigma + 1, which occurs nowhere in the mapped text), the mapped text goes to
 * vlg_index_build_int / vlg_wtsa_build_int, and vlg_queries_parse_int_mapped parses a batch as vlg_queries_parse_int does -- tokens
 * of any 64-bit value -- through the same map.  Host only (no GPU needed for the map itself). */
typedef struct vlg_symbol_map vlg_symbol_map;
vlg_status vlg_symbol_map_create(const uint64_t* h_text, uint64_t n_symbols, vlg_symbol_map** out);
uint64_t vlg_symbol_map_sigma(const vlg_symbol_map* map);
vlg_status vlg_symbol_map_symbols(const vlg_symbol_map* map, uint64_t* h_out /* [sigma] ascending */);
vlg_status vlg_symbol_map_apply(const vlg_symbol_map* map, const uint64_t* h_in, uint64_t n, uint32_t* h_out);
void vlg_symbol_map_destroy(vlg_symbol_map* map);
/* int_alphabet of such an index: *sigma symbols (comp 0 = the sentinel), h_C[sigma + 1], h_comp2char[sigma]; null buffers: sigma only */
vlg_status vlg_index_export_int_alphabet(const vlg_index* idx, uint64_t* sigma, uint64_t* h_C, uint64_t* h_comp2char);
/* wt_int::rank(i, c) (include/sdsl/wt_int.hpp:370-395) on its BWT: out[j] = #d_sym[j] in BWT[0, d_i[j]).  Asynchronous on `stream`. */
vlg_status vlg_int_rank_batch(const vlg_index* idx, const uint64_t* d_i, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, void* stream);
void vlg_index_destroy(vlg_index* idx);

/* Suffix array of text + sentinel on the device (what sdsl::construct_sa computes, include/sdsl/construct_sa.hpp:145-170): d_sa
 * receives n_text + 1 entries, d_sa[0] = n_text.  The same prefix-doubling sorter the index builder uses; n_text < 2^32 - 1.
 * Synchronises `stream`. */
vlg_status vlg_suffix_array_device(const uint8_t* d_text, uint64_t n_text, uint32_t* d_sa, void* stream);
/* ISA samples as csa_wt keeps them (include/sdsl/csa_sampling_strategy.hpp:626-642): h_out[j] = the SA index i with SA[i] = j * inv_dens,
 * count = (n-1)/inv_dens + 1.  Computed from the index alone by walking LF from every SA sample: the byte index on its wavelet tree, the
 * integer-alphabet index (plain or rrr) on its wavelet matrix.  The index must be SA-order sampled (a text-order one: VLG_E_UNSUPPORTED). */
vlg_status vlg_index_isa_samples(const vlg_index* idx, uint32_t inv_dens, uint64_t* h_out, uint64_t count);
/* Store the index in the reference's on-disk format of csa_wt<wt_huff<>,32,64> (csa_wt.hpp:374-393) so that stock sdsl
 * can load_from_file() it: wavelet tree with rank_support_v and both select_support_mcl, SA samples, ISA samples (density
 * 64), byte_alphabet.  The index must be a plain one with SA sample density 32.  An integer-alphabet index is stored as
 * csa_wt<wt_int<>, d, 64, ., ., int_alphabet<>> instead (vlg_index_save_sdsl_int below). */
vlg_status vlg_index_save_sdsl(const vlg_index* idx, const char* path);
/* Load an index stored by stock sdsl: the file written by `store_to_file(csa, file)` / `csa.serialize(out)` for
 * csa_wt<wt_huff<>, t_dens, t_inv_dens> with the default sampling strategies and byte_alphabet
 * (include/sdsl/csa_wt.hpp:374-393; member formats: wt_pc.hpp:638-652, int_vector.hpp:584-600, rank_support_v.hpp:134-148,
 * select_support_mcl.hpp:424-494, wt_helper.hpp:112-131,275-301, lib/csa_alphabet_strategy.cpp:103-121).
 * t_dens is a template parameter of the reference type and is not stored: pass it (0 = 32, the reference default).
 * vlg_sdsl_file_* parse on the host only (no GPU needed); vlg_index_load_sdsl = open + parts + vlg_index_from_parts. */
typedef struct vlg_sdsl_file vlg_sdsl_file;
vlg_status vlg_sdsl_file_open(const char* path, uint32_t sa_sample_dens, vlg_sdsl_file** out);
vlg_status vlg_sdsl_file_parts(const vlg_sdsl_file* f, vlg_index_parts* parts);   /* pointers stay valid until close */
void vlg_sdsl_file_close(vlg_sdsl_file* f);
vlg_status vlg_index_load_sdsl(const char* path, uint32_t sa_sample_dens, vlg_index** out);
/* The same for the file of csa_wt<wt_huff<rrr_vector<63>>, t_dens, t_inv_dens> (bv_kind = VLG_BV_RRR63; the index type of
 * benchmark/indexing_count/index.config:10 and BASELINE config 5): the wavelet tree's bit-vector is an rrr_vector<63>
 * (include/sdsl/rrr_vector.hpp:349-372: size, block classes, offsets, pointer and rank samples, inversion bits; its rank / select
 * supports store nothing).  Every block is decoded on the host (rrr_helper.hpp:304-375) and the index is kept rrr-coded on the
 * device in this library's block numbering (vlg_index_compress): same sizes, same answers.  VLG_BV_PLAIN = vlg_index_load_sdsl. */
vlg_status vlg_sdsl_file_open_kind(const char* path, uint32_t sa_sample_dens, int bv_kind, vlg_sdsl_file** out);
vlg_status vlg_index_load_sdsl_kind(const char* path, uint32_t sa_sample_dens, int bv_kind, vlg_index** out);

/* Integer-alphabet indexes on disk: the file of csa_wt<wt_int<>, t_dens, t_inv_dens, sa_order_sa_sampling<>, isa_sampling<>,
 * int_alphabet<>> (test/csa_int_test.cpp:29-33), written by `store_to_file(csa, file)` (csa_wt.hpp:374-393):
 *   wt_int        size, sigma (distinct values), tree (int_vector<1> of size * max_level bits), rank_support_v<1>,
 *                 select_support_mcl<1>, select_support_mcl<0>, u32 max_level = hi(max(largest symbol, 1)) + 1   (wt_int.hpp:708-732)
 *   SA samples    int_vector<> of width hi(n)+1: SA[0], SA[d], ...;  ISA samples: the same width, (n-1)/t_inv_dens + 1 of them
 *   int_alphabet  m_char (sd_vector<> over largest symbol + 1 bits, EMPTY when the symbols are exactly 0..sigma-1), its rank / select
 *                 supports (sd: nothing stored), m_C (int_vector<> of width hi(n)+1, sigma + 1 entries), u64 m_sigma
 *                 (csa_alphabet_strategy.hpp:470-590; sd_vector.hpp:192-230, 404-416, 538-541, 643-646)
 * The reference's wt_int<> keeps the BWT over the ORIGINAL symbols, level l (of max_level) being the arrangement stably sorted by the
 * symbols' top l bits, one node per prefix (wt_int.hpp:182-262); the device index keeps a wavelet matrix over the compact symbols.
 * Saving and loading convert between the two on the device, one level step at a time (csrc/int_index.hpp).
 *
 * vlg_index_save_sdsl(idx, path) on an integer index (plain or rrr, SA order, any density d) writes the plain type above with
 * t_inv_dens = 64; vlg_index_save_sdsl_int chooses t_inv_dens (0 = 64).  A text-order integer index: VLG_E_UNSUPPORTED (resample it to
 * SA order first); a byte index given to vlg_index_save_sdsl_int: VLG_E_INVALID.
 * vlg_index_load_sdsl_int reads such a file: bv_kind VLG_BV_PLAIN for wt_int<>, VLG_BV_RRR63 for wt_int<rrr_vector<63>> (its blocks
 * decoded on the host, the index then compressed by vlg_index_compress).  t_dens is not stored: pass it (0 = 32).  The ISA samples'
 * count is checked against n, their values are not used.  Malformed files (truncated, trailing bytes, a sample count other than
 * ceil(n / t_dens), wt size != C[sigma], max_level inconsistent with the largest symbol, C not increasing, a tree inconsistent with C)
 * give VLG_E_INVALID; a symbol >= 2^32 gives VLG_E_UNSUPPORTED (the device index holds uint32_t symbols: INTEGRATION.md, symbol map).
 * A loaded index is byte for byte the one vlg_index_build_int makes of the same text.
 * vlg_sdsl_int_file_* parse on the host only (no GPU needed); vlg_index_load_sdsl_int = open + parts + vlg_index_from_int_parts. */
typedef struct {
    uint64_t n;                   /* csa.size() = |text| + 1                                                                  */
    uint64_t sigma;               /* distinct symbols, the sentinel 0 included                                                */
    uint32_t max_level;           /* levels of the reference's wt_int<>: hi(max(largest symbol, 1)) + 1                       */
    uint32_t sa_sample_dens;
    const uint64_t* comp2char;    /* [sigma] ascending, comp2char[0] = 0                                                      */
    const uint64_t* C;            /* [sigma + 1]                                                                              */
    const uint64_t* tree_words;   /* wt_int::tree: level l = bits [l * n, (l + 1) * n), bit i = word[i >> 6] >> (i & 63)      */
    uint64_t tree_bits;           /* n * max_level                                                                            */
    const uint64_t* sa_samples;   /* [n_samples] unpacked: SA[0], SA[dens], ...                                               */
    uint64_t n_samples;
} vlg_int_index_parts;
typedef struct vlg_sdsl_int_file vlg_sdsl_int_file;
vlg_status vlg_sdsl_int_file_open(const char* path, uint32_t sa_sample_dens, int bv_kind, vlg_sdsl_int_file** out);
vlg_status vlg_sdsl_int_file_parts(const vlg_sdsl_int_file* f, vlg_int_index_parts* parts);   /* pointers stay valid until close */
void vlg_sdsl_int_file_close(vlg_sdsl_int_file* f);
vlg_status vlg_index_from_int_parts(const vlg_int_index_parts* h_parts, vlg_index** out);
vlg_status vlg_index_load_sdsl_int(const char* path, uint32_t sa_sample_dens, int bv_kind, vlg_index** out);
vlg_status vlg_index_save_sdsl_int(const vlg_index* idx, const char* path, uint32_t isa_inv_dens);
/* wt_int::tree of an integer index (plain or rrr), converted on the device (two-phase: a null h_words gives *max_level only):
 * h_words receives ceil(n * max_level / 64) words in the layout of vlg_int_index_parts.tree_words. */
vlg_status vlg_index_export_int_tree(const vlg_index* idx, uint32_t* max_level, uint64_t* h_words);

/* One contiguous device image of the read-only index, for replication across the GPUs of a node
 * (SURVEY.md 8e): the owner exports it into caller-provided HBM, the caller moves it with RCCL
 * (ncclBroadcast, or torch.distributed.broadcast on a uint8 tensor), every other rank attaches.
 * The attached index borrows the blob: keep it alive until vlg_index_destroy. */
vlg_status vlg_index_blob_bytes(const vlg_index* idx, uint64_t* bytes);
/* Synchronises `stream`: the image is complete on return. */
vlg_status vlg_index_blob_export(const vlg_index* idx, void* d_blob, uint64_t bytes, void* stream);
vlg_status vlg_index_attach_blob(const void* d_blob, uint64_t bytes, vlg_index** out);
/* The same for ONE process that drives several GPUs of a node (the C++ host's `gm_search_gpu -g N`): a copy of the index in the
 * HBM of `device`, moved by a peer copy over xGMI; the new handle owns its memory.  Calls on it must run with `device`
 * current (vlg_set_device is per host thread). */
vlg_status vlg_index_replicate(const vlg_index* src, int device, vlg_index** out);

/* ------------------------------------------------------------------------------------------
 * X1: RCCL (one process per GPU over xGMI; SURVEY.md 8b "broadcast(handle, ncclComm)", 8e).  An ncclComm_t crosses this ABI as
 * void*.  The caller may bring its own communicator (created with the RCCL its process holds: the library binds RCCL at run time
 * and calls the one already loaded, else librccl.so.1), or make one here: rank 0 calls vlg_comm_unique_id, the host hands the 128
 * bytes to every rank (a pipe, a file, MPI ...), every rank calls vlg_comm_create with its device current.
 * ---------------------------------------------------------------------------------------- */
const char* vlg_comm_library(void);                               /* path of the RCCL that was bound ("" = none)  */
typedef struct { char bytes[128]; } vlg_comm_id;                  /* ncclUniqueId                                */
vlg_status vlg_comm_unique_id(vlg_comm_id* out);                  /* ncclGetUniqueId                             */
vlg_status vlg_comm_create(const vlg_comm_id* id, int n_ranks, int rank, void** nccl_comm);   /* ncclCommInitRank */
vlg_status vlg_comm_info(void* nccl_comm, int* n_ranks, int* rank);
void vlg_comm_destroy(void* nccl_comm);
/* The read-only index of rank `root` in every rank's HBM: one ncclBroadcast of its contiguous image (size first), received
 * straight into the allocation the new index owns -- `idx.load(istream)` on every rank (gm_search.cpp:68-80) replaced by one load
 * + one collective.  Root: pass the index, *out (optional) receives the same handle; other ranks: pass NULL, *out receives a new
 * index to destroy.  Collective: every rank of the communicator calls it. */
vlg_status vlg_index_broadcast(const vlg_index* idx_or_null, void* nccl_comm, int root, void* stream, vlg_index** out);
/* Sum over the ranks, in place, modulo 2^64 -- num_results / checksum (gm_search.cpp:110-114) / located occurrences of a sharded
 * batch.  Host values in, host values out. */
vlg_status vlg_comm_allreduce_sum_u64(void* nccl_comm, uint64_t* h_vals, uint32_t count, void* stream);
/* All-gather of device buffers of different sizes: rank r contributes h_counts[r] elements of elem_bytes (d_send); every rank
 * ends with all of them in rank order in d_recv.  The exchange step of the list-sharded locate (vlg_workspace option "comm"). */
vlg_status vlg_comm_allgatherv(void* nccl_comm, const void* d_send, const uint64_t* h_counts, uint32_t elem_bytes, void* d_recv,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * K1: batched bit-rank.  rank_support_v<1,1>::rank / rank_support_v5<1,1>::rank
 * (include/sdsl/rank_support_v.hpp:114-124, rank_support_v5.hpp:116-134) on a plain bit_vector,
 * re-laid out as 256-bit super-blocks {32-bit count, 224 data bits}.
 * out[j] = number of 1 bits in bv[0, idx[j]),  0 <= idx[j] <= nbits.
 * ---------------------------------------------------------------------------------------- */
vlg_status vlg_bitvector_create(const uint64_t* h_words, uint64_t nbits, vlg_bitvector** out);
/* Asynchronous on `stream`. */
vlg_status vlg_bitvector_rank_batch(const vlg_bitvector* bv, const uint64_t* d_idx, uint64_t* d_out,
                                    uint64_t count, void* stream);
uint64_t vlg_bitvector_hbm_bytes(const vlg_bitvector* bv);
void vlg_bitvector_destroy(vlg_bitvector* bv);

/* ------------------------------------------------------------------------------------------
 * K6: the same batched rank on an H0-compressed bit-vector: rrr_vector<63> + rank_support_rrr<1,63>
 * (include/sdsl/rrr_vector.hpp:145-237, 444-480; block coding include/sdsl/rrr_helper.hpp:304-320, 411-460).
 * One 32-byte header per 32 blocks of 63 bits {ones before, offset position, 32 x 6-bit classes} + offset stream;
 * blocks are decoded on the fly against the binomial table staged in LDS.  Results equal vlg_bitvector_rank_batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct vlg_rrr_bitvector vlg_rrr_bitvector;
vlg_status vlg_rrr_bitvector_create(const uint64_t* h_words, uint64_t nbits, vlg_rrr_bitvector** out);
/* Asynchronous on `stream`. */
vlg_status vlg_rrr_bitvector_rank_batch(const vlg_rrr_bitvector* bv, const uint64_t* d_idx, uint64_t* d_out,
                                        uint64_t count, void* stream);
uint64_t vlg_rrr_bitvector_hbm_bytes(const vlg_rrr_bitvector* bv);
void vlg_rrr_bitvector_destroy(vlg_rrr_bitvector* bv);

/* ------------------------------------------------------------------------------------------
 * K2 / K3 primitives on the index (device-resident arguments).
 * ---------------------------------------------------------------------------------------- */
/* wt_pc::rank(i, c) (include/sdsl/wt_pc.hpp:350-373): out[j] = #c[j] in BWT[0, i[j]).  Asynchronous on `stream`. */
vlg_status vlg_wt_rank_batch(const vlg_index* idx, const uint64_t* d_i, const uint8_t* d_c, uint64_t* d_out,
                             uint64_t count, void* stream);
/* backward_search(csa, 0, n-1, pat.begin(), pat.end(), l, r)
 * (include/sdsl/suffix_array_algorithm.hpp:305-326): pattern p = d_blob[d_off[p], d_off[p+1]).
 * d_l/d_r receive the interval exactly as the reference leaves it; occurrences = r+1-l.  Asynchronous on `stream`. */
vlg_status vlg_backward_search_batch(const vlg_index* idx, const uint8_t* d_blob, const uint64_t* d_off,
                                     uint64_t n_patterns, uint64_t* d_l, uint64_t* d_r, void* stream);
/* csa[i] (include/sdsl/csa_wt.hpp:335-348) for arbitrary SA indices: out[j] = SA[d_i[j]].  Synchronises `stream` when the index keeps
 * 4-byte samples (vlg_index_info.pos_bytes = 4: the SA indices walk in a narrow temporary that is freed on return); with 8-byte
 * samples the walk runs in d_out and the call returns while it does. */
vlg_status vlg_sa_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream);
/* locate (include/sdsl/suffix_array_algorithm.hpp:604-619): for pattern p the occurrences
 * csa[l[p]..r[p]] are written, in SA order (unsorted, like the reference), to
 * d_out[d_out_off[p] ...]; d_out_off = exclusive prefix sum of (r+1-l), n_patterns+1 entries.  Synchronises `stream` under the
 * same condition as vlg_sa_batch. */
vlg_status vlg_locate_batch(const vlg_index* idx, const uint64_t* d_l, const uint64_t* d_r,
                            const uint64_t* d_out_off, uint64_t n_patterns, uint64_t total,
                            uint64_t* d_out, void* stream);

/* Text access: the index keeps no text, but a self-index can give it back.  A vlg_text_access holds, in HBM, the ISA samples of one
 * index -- isa_sample of csa_wt (m_isa_sample, t_inv_dens: include/sdsl/csa_wt.hpp:145-151; csa_sampling_strategy.hpp:626-642):
 * ISA[0], ISA[d], ISA[2d], ..., 4 bytes each when n < 2^32, else 8 -- computed on the device like vlg_index_isa_samples.  It does not
 * change idx, which must outlive it.  SA-order indexes only (byte or integer, plain or rrr, any SA density including 1); a text-order
 * index gives VLG_E_UNSUPPORTED (the reference derives its ISA through the marks, which needs a select structure).
 * inv_dens = 0 means 64, the reference's t_inv_dens default.  Creation walks n LF steps in all and synchronises `stream`. */
typedef struct vlg_text_access vlg_text_access;
vlg_status vlg_text_access_create(const vlg_index* idx, uint32_t inv_dens, void* stream, vlg_text_access** out);
void vlg_text_access_destroy(vlg_text_access* t);
/* sdsl::extract(csa, begin, end) (include/sdsl/suffix_array_algorithm.hpp:645-745, the lf_tag specialisation; csa.text[i] --
 * text_of_csa, suffix_array_helper.hpp:641 -- is the range [i, i]) for every range r: inclusive ends, begin[r] <= end[r] < n (n = |text| + 1: position n - 1 is the sentinel and extracts
 * as 0).  Range r is written to d_out from d_out_off[r] on (the exclusive prefix sum of the lengths end - begin + 1; every range must
 * end within `total` elements).  d_out holds uint8_t for a byte index, uint32_t ORIGINAL symbols (comp2char applied) for an integer
 * one.  Each range is cut at the multiples of d and one lane walks each piece backward from an ISA sample: at most d LF steps per
 * lane, however long the range.  The ranges are checked on the device first: any bad range gives VLG_E_INVALID and nothing is
 * written.  Synchronises `stream`. */
vlg_status vlg_extract_batch(const vlg_text_access* t, const uint64_t* d_begin, const uint64_t* d_end, const uint64_t* d_out_off,
                             uint64_t n_ranges, uint64_t total, void* d_out, void* stream);
/* csa.isa[i] (include/sdsl/csa_wt.hpp:149; isa_of_csa_wt::operator[], suffix_array_helper.hpp:500-514, from
 * isa_sample.sample_qeq, csa_sampling_strategy.hpp:650-663): d_out[j] = ISA[d_i[j]], fewer than d LF steps from the next sample.  A position >= n gives VLG_E_INVALID (d_out is then undefined).  Synchronises `stream`. */
vlg_status vlg_isa_batch(const vlg_text_access* t, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream);

/* Select.  A vlg_select_support holds, in HBM, what select needs beside a bit-vector or an index: select hints, `sample` ones (and
 * zeros) apart -- the super-block that holds every sample-th one (zero) of every wavelet-tree node (byte index), of every
 * wavelet-matrix level (integer index) or of the bit-vector; sample = 0 means 512, otherwise a power of two in [64, 65536]
 * (VLG_E_INVALID for anything else).  At 512 the hints take 1/16 of the bytes of the plain bit-vectors they serve.  It replaces
 * select_support_mcl<1> and <0> (include/sdsl/select_support_mcl.hpp:347-400), select_support_rrr<1> and <0>
 * (include/sdsl/rrr_vector.hpp:638-700) and the select structures inside wt_pc / wt_int.  The handle does not change its source,
 * which must outlive it; an index of any kind is taken (byte or integer alphabet, plain or rrr-63, SA-order or text-order sampling,
 * built, loaded or attached).  Creation first reads the source's totals with blocking copies (the last block or header of a
 * bit-vector; the node table, C or Z of an index: a few KiB), then uploads its tables and runs one pass over the super-block counts
 * on `stream`.  Synchronises `stream`: the support is complete on return. */
typedef struct vlg_select_support vlg_select_support;
vlg_status vlg_bitvector_select_create(const vlg_bitvector* bv, uint32_t sample, void* stream, vlg_select_support** out);
vlg_status vlg_rrr_bitvector_select_create(const vlg_rrr_bitvector* bv, uint32_t sample, void* stream, vlg_select_support** out);
vlg_status vlg_index_select_create(const vlg_index* idx, uint32_t sample, void* stream, vlg_select_support** out);
uint64_t vlg_select_support_hbm_bytes(const vlg_select_support* s);
void vlg_select_support_destroy(vlg_select_support* s);
/* select_support_mcl<bit>::select(k) (select_support_mcl.hpp:347-400; select_support_rrr<bit>::select, rrr_vector.hpp:638-700):
 * d_out[j] = position of the d_k[j]-th `bit` (k = 1 .. number of them) of the bit-vector the support was made from; k = 0 or a k
 * larger than that number gives nbits.  A support made from an index gives VLG_E_INVALID.  Asynchronous on `stream`. */
vlg_status vlg_bit_select_batch(const vlg_select_support* s, int bit, const uint64_t* d_k, uint64_t* d_out, uint64_t count, void* stream);
/* wt_pc::select(k, c) (include/sdsl/wt_pc.hpp:415-442) on the BWT of a byte index: d_out[j] = SA index of the d_k[j]-th occurrence of the
 * text byte d_c[j] in the BWT (c = 0: the sentinel).  k = 0, a k larger than the number of occurrences, or a byte that does not occur
 * gives n (wt_pc.hpp:418-420).  A support made from a bit-vector or from an integer index gives VLG_E_INVALID.  Asynchronous on `stream`. */
vlg_status vlg_wt_select_batch(const vlg_select_support* s, const uint64_t* d_k, const uint8_t* d_c, uint64_t* d_out, uint64_t count, void* stream);
/* wt_int::select(k, c) (include/sdsl/wt_int.hpp:442-480) on the BWT of an integer index; symbols as vlg_int_rank_batch takes them (the
 * original symbols, 0 = the sentinel).  The same refusals: n for k = 0, k too large, an absent symbol or one above the largest.
 * Asynchronous on `stream`. */
vlg_status vlg_int_select_batch(const vlg_select_support* s, const uint64_t* d_k, const uint32_t* d_sym, uint64_t* d_out, uint64_t count, void* stream);
/* csa.psi[i] (psi_of_csa_wt::operator[], include/sdsl/suffix_array_helper.hpp:322-332) = wt.select(i - C[comp(F[i])] + 1, F[i]), byte and
 * integer indexes: d_out[j] = ISA[(SA[d_i[j]] + 1) mod n].  An i >= n gives ~0.  Asynchronous on `stream`. */
vlg_status vlg_psi_batch(const vlg_select_support* s, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream);
/* csa.lf[i] (lf_of_csa_wt::operator[], suffix_array_helper.hpp:336-349) and csa.bwt[i] (bwt_of_csa_wt::operator[], :425-429): the LF step
 * of the locate kernels, byte and integer indexes, no support needed.  lf: d_out[j] = ISA[(SA[d_i[j]] - 1) mod n], ~0 for i >= n.
 * bwt: d_out holds uint8_t (byte index, comp2char applied) or uint32_t original symbols (integer index), as vlg_extract_batch
 * writes them; the sentinel and an i >= n give 0.  Both calls are asynchronous on `stream`. */
vlg_status vlg_lf_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream);
vlg_status vlg_bwt_batch(const vlg_index* idx, const uint64_t* d_i, void* d_out, uint64_t count, void* stream);
/* The quad image of a byte index with plain bit-vectors: the wavelet tree two levels per 32-byte read, derived on the device when the
 * index is made and kept beside the blob in an allocation of its own (it is not part of the blob, of the exported parts or of a saved
 * file: whoever attaches a blob derives its own).  The locate kernels walk LF on it (workspace option "quad_walk").  rrr and integer
 * indexes, sigma = 1 and a tree in which a digit count would not fit 32 bits have none: bytes = 0, n_nodes = 0.  Its bytes are part of
 * vlg_index_info.hbm_bytes.  Any of the three outputs may be null. */
vlg_status vlg_index_quad_image(const vlg_index* idx, uint64_t* bytes, uint32_t* n_nodes, double* build_s);
/* For tests: the LF step of vlg_lf_batch taken through the quad image.  d_lf[j] = LF(d_i[j]) (~0 for i >= n), d_comp[j] = the compact
 * symbol read on the way, d_levels[j] = the binary tree levels the step accounts for (the symbol's code length); any output may be
 * null.  VLG_E_UNSUPPORTED for an index without an image.  Runs on the null stream and returns when the results are there. */
vlg_status vlg_quad_lf_batch(const vlg_index* idx, const uint64_t* d_i, uint64_t* d_lf, uint8_t* d_comp, uint32_t* d_levels, uint64_t count);

/* ------------------------------------------------------------------------------------------
 * Query batches.  Parsing mirrors the reference's two dialects:
 *   VLG_DIALECT_LIBRARY   gapped_pattern_query(const std::string&)   include/sdsl/vlg_index.hpp:54-105
 *   VLG_DIALECT_BENCHMARK gapped_pattern(const std::string&, true) + index_sasearch's gap mapping
 *                         benchmark/gapped-matching/include/utils.hpp:25-70, index_sasearch.hpp:68-69,113
 * ---------------------------------------------------------------------------------------- */
#define VLG_DIALECT_LIBRARY 0
#define VLG_DIALECT_BENCHMARK 1
#define VLG_MAX_SUBPATTERNS 64

/* Host-only view of one parsed query (no device involved): sub-pattern i = re[sub_off[i], sub_off[i]+sub_len[i]);
 * lo/hi[i] (i >= 1) = start-to-start distance bounds between sub-patterns i-1 and i; end_len = length added to the
 * last position for the non-overlap rule.  Returns VLG_E_PARSE / VLG_E_INVALID like vlg_queries_parse. */
typedef struct {
    uint32_t k;
    uint32_t reserved;
    uint64_t sub_off[VLG_MAX_SUBPATTERNS], sub_len[VLG_MAX_SUBPATTERNS];
    uint64_t lo[VLG_MAX_SUBPATTERNS], hi[VLG_MAX_SUBPATTERNS];
    uint64_t end_len;
} vlg_parsed_query;
vlg_status vlg_parse_query(const char* h_regexp, uint64_t len, int dialect, vlg_parsed_query* out);

/* Parse `n_queries` regexps (concatenated in h_text; query q = h_text[h_off[q], h_off[q+1])) and upload.
 * h_status (optional, n_queries ints) receives VLG_OK / VLG_E_PARSE / VLG_E_INVALID per query; an
 * unparsable query stays in the batch as an always-empty query (the reference driver skips such
 * lines, utils.hpp:94-99).  Returns VLG_E_PARSE if any query failed and h_status is NULL. */
vlg_status vlg_queries_parse(const char* h_text, const uint64_t* h_off, uint64_t n_queries, int dialect,
                             int* h_status, vlg_queries** out);
/* Already-parsed form: sub-pattern bytes + per-gap start-to-start bounds (lo,hi) + non-overlap length.
 * Query q has sub-patterns [h_qsub[q], h_qsub[q+1]); sub-pattern s = h_blob[h_suboff[s], h_suboff[s+1]);
 * h_lo/h_hi are indexed by sub-pattern (entry of a query's first sub-pattern is ignored).
 * Accepted: at most VLG_MAX_SUBPATTERNS non-empty sub-patterns per query, lo <= hi < 2^63 for every gap (lo may be smaller than
 * the previous sub-pattern's length, down to 0: two sub-patterns at the same position), and 1 <= end_len < 2^63 for every query
 * with a sub-pattern -- after a match the search restarts at its last position + end_len, and with 0 it would not advance.
 * Anything else is VLG_E_INVALID, decided on the host before a device is asked for. */
vlg_status vlg_queries_create(const uint8_t* h_blob, const uint64_t* h_suboff, const uint64_t* h_qsub,
                              const uint64_t* h_lo, const uint64_t* h_hi, const uint64_t* h_end_len,
                              uint64_t n_queries, vlg_queries** out);
/* sdsl::count(csa, sub-pattern) (include/sdsl/suffix_array_algorithm.hpp:516-529) for every sub-pattern of the batch: one
 * backward-search pass, h_occ[s] = r + 1 - l (vlg_queries_subpatterns(q) entries, in batch order).  What SURVEY.md 8(e) shards
 * a batch by: the sum over a query's sub-patterns estimates its locate + join work.  Synchronises `stream`. */
vlg_status vlg_queries_occurrences(const vlg_index* idx, const vlg_queries* q, uint64_t* h_occ, void* stream);
/* The same pass, returning the SA interval [l, r] of every sub-pattern as backward_search leaves it (r + 1 - l occurrences;
 * suffix_array_algorithm.hpp:305-326).  Equal intervals are the same occurrence list: a host that shards a batch can keep the
 * queries that share their longest list on one GPU, so that the list is located once (vlg_matching_amd.dist.shard_by_affinity).
 * Synchronises `stream`. */
vlg_status vlg_queries_intervals(const vlg_index* idx, const vlg_queries* q, uint64_t* h_l, uint64_t* h_r, void* stream);
uint64_t vlg_queries_count(const vlg_queries* q);
uint64_t vlg_queries_subpatterns(const vlg_queries* q);
/* h_k[q] = number of sub-patterns of query q (0 for a query that failed to parse). */
vlg_status vlg_queries_k(const vlg_queries* q, uint32_t* h_k);
/* Text windows of a batch: query j is answered on [h_begin[j], h_end[j]) and its matches are exactly those of the same query on the
 * stand-alone text T[begin, end), with begin added to every position -- what a caller with a document collection asks for: one batch
 * entry per (query, document) pair, every distinct occurrence list still located once.  An occurrence of a sub-pattern of m symbols
 * (m = (suboff[s + 1] - suboff[s]) / symbol bytes) counts only if it lies wholly inside: begin <= v and v + m <= end.  h_begin / h_end
 * are host arrays of vlg_queries_count(q) entries, copied; a NULL h_begin means all zeros, a NULL h_end "to the end of the text"; both
 * NULL removes the windows and the batch is what it was.  The batch does not know the text: an end beyond it is clamped at search time,
 * a begin beyond it is an empty window.  begin[j] > end[j] gives VLG_E_INVALID and the batch keeps its previous windows; a window shorter
 * than a sub-pattern, or begin == end, makes an empty query and is no error.  Host only: no device, no stream.
 *   vlg_search_batch honours the windows (byte and integer indexes, plain or rrr, either sampling, any density); gaps, end_len, "tuples"
 *     and every other workspace option keep their meaning, the checksum is the sum over what is returned.  A collective search
 *     (vlg_workspace_set_comm / _set_exchange* with more than one rank) of a windowed batch gives VLG_E_UNSUPPORTED before any launch.
 *   vlg_queries_occurrences, vlg_queries_intervals and vlg_wtsa_ranges ignore them: they answer per sub-pattern.
 *   vlg_wtsa_search_batch and vlg_wtsa_search_window_batch refuse a batch that carries windows with VLG_E_INVALID: that path takes its
 *     windows as arrays.
 * A batch must not be changed (windows included) while a search on it runs.
 * get: *has_windows = 1 when the batch carries windows; h_begin / h_end (either may be NULL) receive them as they were set (a NULL
 * h_begin reads as zeros, a NULL h_end as UINT64_MAX; a batch without windows gives 0 and UINT64_MAX). */
vlg_status vlg_queries_set_windows(vlg_queries* q, const uint64_t* h_begin, const uint64_t* h_end);
vlg_status vlg_queries_get_windows(const vlg_queries* q, int* has_windows, uint64_t* h_begin, uint64_t* h_end);

/* Documents: the indexed text as a collection -- proteins, contigs, lines, files laid end to end -- and searches whose matches never
 * cross a document boundary.  A vlg_documents is a device-resident handle beside the index, like vlg_text_access and
 * vlg_select_support: it holds the starts b_0 = 0 < b_1 < ... < b_{d-1} < n_text of the d documents and the sentinel b_d = n_text
 * (8 bytes each, and one fence per 64 of them, laid out as the fences of the occurrence lists are); document j is [b_j, b_{j+1}).
 *   vlg_documents_create: h_starts is a host array of n_docs starts, copied.  Checked on the host before a device is asked for: NULL
 *     starts, n_docs == 0, h_starts[0] != 0, starts that do not strictly ascend, a start >= n_text (so n_text == 0 too) and
 *     n_docs >= 2^32 - 16 give VLG_E_INVALID; then VLG_E_NO_DEVICE without a device.  Returns when the starts are on the device.
 *   vlg_documents_locate_batch: doc[j] = the document of positions[j], offset[j] = positions[j] - its start -- what turns a hit into
 *     (protein, offset).  One lower-bound kernel.  positions, doc and offset (either output may be NULL) are DEVICE arrays of n
 *     entries, as for vlg_psi_batch.  A position >= n_text gets doc = UINT64_MAX and offset = UINT64_MAX.  Runs on the null stream and
 *     returns when the results are there (like vlg_quad_lf_batch; neither entry point takes a stream).
 * vlg_queries_set_documents(q, d) makes every later vlg_search_batch of the batch document-bounded; d == NULL removes the documents and
 * the batch is what it was.  Host only (no device, no stream), the contract of vlg_queries_set_windows; the handle is borrowed and must
 * outlive the searches.  Any batch takes documents: byte, integer, character classes, mismatch budgets.  A batch that carries windows
 * refuses documents and a batch that carries documents refuses windows: VLG_E_UNSUPPORTED, the batch left as it was.
 * Semantics.  An occurrence of a sub-pattern of m symbols at v lies inside a document iff doc(v) == doc(v + m - 1).  The matches of a
 * query are, for j ascending, the matches of the same query on the stand-alone text T[b_j, b_{j+1}) with b_j added to every position:
 * exactly the answer of a windowed batch with one entry (query, b_j, b_{j+1}) per document, concatenated -- counts, first positions,
 * tuples, n_matches and the checksum follow from it -- but with ONE batch entry per query and every distinct occurrence list located
 * and sorted once.  This holds in both dialects: a match in one document never delays the first match of the next (the restart key
 * end + end_len of the non-overlap rule is capped at the next boundary, which matters for the benchmark dialect's end_len = |s_0|).
 * With the single document [0, n_text) the result is bit-identical to that of the batch without documents.
 * How: the join's link and jump passes run instantiations that look the next boundary nb(x) of every list element up:
 * an element whose sub-pattern crosses nb(x) is infeasible, its gap window ends at min(x + hi, nb(x) - m') for a next sub-pattern of m'
 * symbols.  The window filter, sort, locate and gather are untouched (the filter keeps the uncapped windows: a superset).  A batch
 * without documents launches exactly the kernels it launched before.  The workspace option "fuse_jump" = 0 is honoured: the separate
 * jump pass applies the same restart cap.
 * Road by road:
 *   vlg_search_batch honours documents on byte and integer indexes (plain or rrr, either sampling) and on batches with classes or
 *     budgets.  n_text of the handle must be the index's text length (n - 1, without the sentinel): VLG_E_INVALID otherwise, at
 *     search time, before any launch.  A collective search (more than one rank) of such a batch: VLG_E_UNSUPPORTED before any launch.
 *   vlg_wtsa_search_batch and vlg_wtsa_search_window_batch refuse a batch with documents: VLG_E_UNSUPPORTED before any launch.
 *   vlg_join_batch joins caller-built lists and does not look at documents; vlg_queries_occurrences, vlg_queries_intervals and
 *     vlg_wtsa_ranges answer per sub-pattern and ignore them. */
typedef struct vlg_documents vlg_documents;
vlg_status vlg_documents_create(const uint64_t* h_starts, uint64_t n_docs, uint64_t n_text, vlg_documents** out);
void vlg_documents_destroy(vlg_documents* d);
uint64_t vlg_documents_count(const vlg_documents* d);
uint64_t vlg_documents_text_length(const vlg_documents* d);
vlg_status vlg_documents_locate_batch(const vlg_documents* d, const uint64_t* positions, uint64_t n, uint64_t* doc, uint64_t* offset);
vlg_status vlg_queries_set_documents(vlg_queries* q, const vlg_documents* d);
vlg_status vlg_queries_get_documents(const vlg_queries* q, const vlg_documents** out);
void vlg_queries_destroy(vlg_queries* q);

/* Document listing: which documents each query of a result matches, and how often -- reduced on the device, where the first positions
 * already lie sorted per query beside the document starts.  It replaces vlg_result_fetch of every first position (1.2 GB for a result
 * of the C3 size), a lower bound per position (on the host, or the positions uploaded again for vlg_documents_locate_batch) and a
 * run-length encoding on the host: what crosses PCIe is one (document, first match) pair per document hit instead of every match.
 * Semantics.  F_q = the first positions of query q's matches in the order vlg_result_fetch returns them, doc(x) = j with
 * b_j <= x < b_{j+1}.  The listing of q is the sequence of maximal runs of equal doc(F_q[i]), in order; a run gives
 *   doc          the document
 *   count        the length of the run
 *   first_match  the index of the run's first match in the result's match numbering, offsets[q] + i (offsets of vlg_result_fetch):
 *                what slices first positions or tuples per document
 * and df[q] is the number of runs: the documents q matches.  A match belongs to the document of its FIRST position; for a
 * document-bounded search with the same handle the whole match lies there and count is the number of matches q has on the stand-alone
 * document.  A run never continues across a query border, even when the neighbouring queries hit the same document.
 *   vlg_result_list_documents  what = VLG_DOCLIST_PAIRS: df and the pairs.  what = VLG_DOCLIST_DF: only df and the number of pairs (the
 *     pass that writes the pairs is skipped).  The listing stays on the device until fetched, and borrows neither r nor d once the call
 *     has returned.  Runs on the null stream and returns when the listing is there (like vlg_documents_locate_batch: no stream, no
 *     workspace; every search synchronises its stream before it returns its result).  A result without matches gives a listing of zero
 *     pairs and launches nothing.
 *     Accepted: every result of vlg_search_batch (byte or integer index, plain or rrr, classes, budgets, windows, documents or none,
 *     one chunk or several), of vlg_join_batch, of vlg_wtsa_search_batch and of vlg_wtsa_search_window_batch.
 *     Refused, nothing returned and *out untouched: a NULL argument or an unknown `what` (VLG_E_INVALID); a match whose first position
 *     is >= vlg_documents_text_length(d), i.e. documents of another text (VLG_E_INVALID); the result of a collective search that holds
 *     only part of the queries (vlg_result_owned_queries gives ranges: VLG_E_UNSUPPORTED).
 *   vlg_doc_listing_info   either output may be NULL.
 *   vlg_doc_listing_fetch  h_df[q], h_offsets (n_queries + 1, exclusive prefix sum of df: query q owns the pairs
 *     [h_offsets[q], h_offsets[q + 1])), and h_docs / h_counts / h_first_match of n_pairs entries each.  Any pointer may be NULL; one of
 *     the last three on a VLG_DOCLIST_DF listing gives VLG_E_INVALID.  Documents cross PCIe 4 bytes wide (n_docs < 2^32 - 16), counts
 *     are taken on the host from consecutive first_match values, closed by the query's end.
 * How: a head pass in the element-parallel shape of the join passes (matches dealt to waves in runs of VLG_DOCLIST_RUN,
 * 64 per step: documents through the fences, query borders carried along, one word of head bits per step), a scan of the per-run head
 * counts, and a pass in which every head writes its pair at its rank.  No search launches anything it did not launch before. */
typedef struct vlg_doc_listing vlg_doc_listing;
enum { VLG_DOCLIST_DF = 0, VLG_DOCLIST_PAIRS = 1 };
vlg_status vlg_result_list_documents(const vlg_result* r, const vlg_documents* d, int what, vlg_doc_listing** out);
vlg_status vlg_doc_listing_info(const vlg_doc_listing* l, uint64_t* n_queries, uint64_t* n_pairs);
vlg_status vlg_doc_listing_fetch(const vlg_doc_listing* l, uint64_t* h_df, uint64_t* h_offsets /* n_queries + 1 */,
                                 uint64_t* h_docs, uint64_t* h_counts, uint64_t* h_first_match /* n_pairs each */);
void vlg_doc_listing_destroy(vlg_doc_listing* l);

/* Match texts: what every match of a result matched, extracted on the device.  A class position accepts a set of bytes, a budgeted
 * sub-pattern matches some neighbour of itself, and a gap .{100,2000}? stands for whatever lies between the sub-patterns (for in-silico
 * PCR that stretch is the amplicon): the positions of a result no longer say what the text holds there.  The first positions and the
 * tuples, the document starts and a text access are all in HBM; this call composes them without a round trip through the host
 * (vlg_result_fetch of every tuple, ranges computed and uploaded again, vlg_extract_batch, download).
 * The rule.  The matches of a result are numbered as vlg_result_fetch returns them.  For match i of query q: p0 its first position, pl
 * the position of its last sub-pattern (its last tuple value; p0 when k(q) = 1), m_last the number of SYMBOLS of q's last sub-pattern.
 * The core of the match is [p0, ce), ce = pl + m_last.  The bounds [B0, B1) are [0, n_text) when docs is NULL, otherwise the document of
 * p0 (a match belongs to the document of its first position, as in the listing).  The extracted range is [b, e):
 *   b = p0 - min(flank_left, p0 - min(p0, B0))        e = ce + min(flank_right, max(B1, ce) - ce)
 * The core is never cut, the flanks stop at the text's or the document's ends, and a core that reaches over its document's end (a
 * result of a search without documents) keeps itself and gets no right flank.  A flank of UINT64_MAX means "to the bound".
 *   vlg_result_extract_matches  extracts the matches [match_begin, match_end) of the fetch numbering (match_end = UINT64_MAX: to the
 *     last match), so that a large result can be paged through; the offsets of vlg_result_fetch give the slice of one query.
 *     max_symbols, when not 0, caps the symbols of the slice: a slice with more is refused BEFORE the symbol buffer is allocated.  The
 *     texts stay on the device until fetched; the handle borrows none of r, q, t, docs once the call has returned.  Runs on the
 *     null stream and returns when the texts are there (the listing's contract: no stream, no workspace).  An empty slice or an empty
 *     result gives a handle with 0 matches and launches nothing.
 *     Accepted: every result of vlg_search_batch (byte or integer index, plain or rrr, classes, budgets, windows, documents or none, 4-
 *     or 8-byte positions, one chunk or several), of vlg_join_batch, of vlg_wtsa_search_batch and of vlg_wtsa_search_window_batch; q is
 *     the batch that was searched (for vlg_join_batch: a batch of the same shape whose last sub-patterns have the joined lengths), t a
 *     text access of an index of the same text.  A result without tuples (workspace option "tuples" = 0) is accepted iff every query
 *     with a match in the slice has k = 1.
 *     Refused, nothing left allocated and *out untouched.  VLG_E_INVALID: a NULL r, q, t or out; match_begin > match_end; match_end
 *     beyond the matches; a q whose number of queries, or the k of any query, differs from the result's; a byte batch with the text of
 *     an integer index or the reverse; docs whose text length is not that of t's index; a result without tuples and a k > 1 query with
 *     a match in the slice; any match whose core is none of the text (ce > n_text, a position behind the text: q, t or docs do not
 *     belong to this result -- the message says how many, from a counter on the device).  VLG_E_WORKSPACE: more symbols than a
 *     non-zero max_symbols (the message names both numbers).  VLG_E_UNSUPPORTED: the result of a collective search that holds only
 *     part of the queries, as the listing refuses it.
 *   vlg_match_texts_info   any output may be NULL.  symbol_bytes is 1 for a byte index and 4 for an integer one.
 *   vlg_match_texts_fetch  text i of the slice is h_symbols[h_offsets[i] .. h_offsets[i + 1]) -- uint8_t for a byte index, the ORIGINAL
 *     uint32_t symbols for an integer one, what vlg_extract_batch writes -- and h_begin[i] is b: a sub-pattern's offset inside its text
 *     is tuple value - b.  Any pointer may be NULL.
 * How: a span pass in the shape of the listing's head pass (runs of VLG_DOCLIST_RUN matches per wave, 64 per step; the
 * query of a lane from the carried offsets, the document of p0 through the fences) writes b, e - 1 and e - b; one scan of the lengths
 * gives the offsets; vlg_extract_batch walks the ranges.  No search launches anything it did not launch before. */
typedef struct vlg_match_texts vlg_match_texts;
vlg_status vlg_result_extract_matches(const vlg_result* r, const vlg_queries* q, const vlg_text_access* t,
                                      const vlg_documents* docs /* may be NULL */,
                                      uint64_t flank_left, uint64_t flank_right,
                                      uint64_t match_begin, uint64_t match_end /* UINT64_MAX: to the last match */,
                                      uint64_t max_symbols /* 0: no cap */, vlg_match_texts** out);
vlg_status vlg_match_texts_info(const vlg_match_texts* m, uint64_t* n_matches, uint64_t* n_symbols, uint32_t* symbol_bytes);
vlg_status vlg_match_texts_fetch(const vlg_match_texts* m, uint64_t* h_offsets /* n_matches + 1 */,
                                 uint64_t* h_begin /* n_matches: b of every match */, void* h_symbols);
void vlg_match_texts_destroy(vlg_match_texts* m);

/* Character classes: a position of a sub-pattern may accept a SET of bytes -- PROSITE motifs (C-x(2,4)-C-x(3)-[LIVMFYWC] is
 * "C.{2,4}?C.{3,3}?[LIVMFYWC]"), IUPAC codes (R = [AG]), case-insensitive words ([Tt]he).  Expanding such a query into one query per
 * member string gives other answers: the left-most, lazy, non-overlapping rule applies to the UNION of the alternatives' occurrences.
 * Syntax: the library dialect (s0.{a,b}?s1..., the same gap rules and errors) where, inside a sub-pattern and read left to right,
 *   [ ... ]   is ONE position that accepts the bytes listed: single bytes and ranges x-y (x > y: VLG_E_PARSE; a '-' right behind '[',
 *             '[^' or in front of ']' is itself); a leading ^ complements the set over the bytes 1..255; ".{" inside a class is two members
 *   \x        is the byte x, inside and outside a class (\[ \] \\ \. \- \^); a lone \ at the end is VLG_E_PARSE
 *   [], [^] and a class without its ] are VLG_E_PARSE.  The 0 byte is never a member: complements leave it out, a class that names it is
 *   VLG_E_INVALID (so is a complement that accepts nothing).  At most VLG_MAX_SUBPATTERNS sub-patterns, none empty (VLG_E_INVALID).
 * A sub-pattern's length m is its number of POSITIONS; lo / hi / end_len follow from m as the library dialect derives them from byte
 * lengths.  vlg_parse_query / vlg_queries_parse are not touched: '[' and '\' stay literal bytes there.
 *   vlg_parse_class_query  host only, no device.  `out` as for vlg_parse_query with sub_len in positions and sub_off = the first
 *     position of the sub-pattern in the mask array; h_masks (room for cap_positions positions, VLG_E_INVALID when too small; NULL only
 *     counts) receives 32 bytes per position, bit c (byte c / 8, bit c % 8) = byte c is accepted; *n_positions (optional) = positions.
 *   vlg_queries_parse_classes  the batch form, with the per-query status contract of vlg_queries_parse.
 *   vlg_queries_create_classes  the already-parsed form, as vlg_queries_create with mask rows for bytes (h_suboff counts positions) and
 *     the same validity rules; a position that accepts no byte, or several with the 0 byte among them, is VLG_E_INVALID.
 * A batch in which every position accepts exactly one byte HAS no classes: it is the batch vlg_queries_parse / vlg_queries_create make
 * of the same strings, and every entry point treats it so.
 * vlg_search_batch answers a batch with classes on a byte index (plain or rrr, either sampling, any density, n <= 2^32 + 1; a longer
 * text: VLG_E_UNSUPPORTED): every distinct sub-pattern is searched once -- one with a class by a backward search that branches over the
 * members the text has and keeps a frontier of pairwise disjoint SA intervals, one per member string that occurs -- its intervals are
 * located into ONE list, sorted, and the lists are joined as ever; "tuples", the window filter and the workspace cap keep their
 * meaning.  The frontier of a sub-pattern holds at most "class_intervals" intervals (vlg_workspace_set_option, default 1024, 1 .. 2^20)
 * at any step; one that would pass it makes the search return VLG_E_WORKSPACE, naming the query, the sub-pattern and the option, with
 * nothing written beyond the cap and nothing further launched (exactly that many is legal).
 * Summary of such a search: located_occurrences = sum of the distinct lists' lengths, logical_occurrences = sum of the list lengths of
 * the live queries, lf_steps / wt_levels_locate from the walks, wt_levels_bsearch over both backward searches, locate_mode =
 * VLG_LOCATE_WALKS (the lists are always located by random-access walks here); everything else as for any batch.
 * Out of scope, refused with VLG_E_UNSUPPORTED before any launch when the batch has classes: text windows (vlg_queries_set_windows),
 * collective searches, integer-alphabet indexes, vlg_queries_occurrences, vlg_queries_intervals, vlg_wtsa_ranges, vlg_wtsa_search_batch
 * and vlg_wtsa_search_window_batch.  The benchmark dialect has no class form. */
vlg_status vlg_parse_class_query(const char* h_regexp, uint64_t len, vlg_parsed_query* out, uint8_t* h_masks, uint64_t cap_positions,
                                 uint64_t* n_positions);
vlg_status vlg_queries_parse_classes(const char* h_text, const uint64_t* h_off, uint64_t n_queries, int* h_status, vlg_queries** out);
vlg_status vlg_queries_create_classes(const uint8_t* h_masks, const uint64_t* h_suboff, const uint64_t* h_qsub, const uint64_t* h_lo,
                                      const uint64_t* h_hi, const uint64_t* h_end_len, uint64_t n_queries, vlg_queries** out);
/* The SA intervals of every sub-pattern of a batch with classes, from a host copy the result of its vlg_search_batch keeps:
 * sub-pattern s (batch order) has the intervals [h_l[j], h_r[j]], h_ivoff[s] <= j < h_ivoff[s + 1], ascending by l and pairwise
 * disjoint (a literal sub-pattern has one, or none).  h_ivoff has vlg_queries_subpatterns(q) + 1 entries; h_l / h_r may be NULL to
 * fetch the offsets alone.  A result of any other search gives VLG_E_INVALID. */
vlg_status vlg_result_class_intervals(const vlg_result* r, uint64_t* h_ivoff, uint64_t* h_l, uint64_t* h_r);

/* Mismatch budgets: a sub-pattern may differ from the text in up to k of its positions (Hamming distance, substitutions only) -- primers
 * with one or two substitutions for in-silico PCR ("fwd.{100,2000}?rev"), motifs with a tolerated residue.  Expanding a sub-pattern into
 * its neighbours gives other answers, for the reason given for classes: the left-most, lazy, non-overlapping rule applies to the UNION
 * of the neighbours' occurrences.
 * A sub-pattern with the positions S_0 .. S_{m-1} (sets of bytes; one byte each when it is literal) and the budget k OCCURS AT v when
 * 0 <= v, v + m <= n and #{t : T[v + t] not in S_t} <= k.  m, and with it lo / hi / end_len, stay as parsed; the 0 byte is never
 * substituted in (the sentinel is not text); k >= m means "every position may differ" and behaves as k = m.  The matches of a query
 * are the left-most, lazy, non-overlapping ones over these occurrence lists; nothing else about a query changes.
 *   vlg_queries_set_mismatches  host only, no device, no stream (the contract of vlg_queries_set_windows).  h_k has
 *     vlg_queries_subpatterns(q) entries in batch order; NULL or all zeros removes the budgets, and the batch is what it was.  Any batch
 *     of bytes takes them: vlg_queries_parse, _create, _parse_classes, _create_classes.  The query syntax has no form for a budget.
 *   vlg_queries_get_mismatches  *has (optional) = 1 when a budget > 0 is set; h_k (optional) receives the budgets, zeros when none is set.
 * VLG_E_UNSUPPORTED, the batch left as it was and no device touched: an integer batch (vlg_queries_parse_int, _parse_int_mapped);
 * vlg_queries_set_mismatches on a batch that carries windows; vlg_queries_set_windows on a batch that carries budgets.
 * vlg_search_batch answers a batch with budgets on the road of a batch with classes (byte index, n <= 2^32 + 1): a distinct sub-pattern
 * is a content AND its effective budget min(k, m); one with budget 0 is searched as without budgets, one with a budget > 0 by a
 * backward search that branches over every byte the text has and carries the misses so far with each SA interval -- its frontier ends
 * as one interval per distinct string within the budget that occurs, ascending and disjoint, under the same "class_intervals" cap and
 * the same VLG_E_WORKSPACE.  The first k steps of such a search are unconstrained: sigma^k intervals at least are needed for them.
 * Summary and vlg_result_class_intervals as for a batch with classes (the latter for any result of this road, a batch of literal
 * sub-patterns with budgets included); the kernel-stat class "class_search" counts the budgeted searches too.
 * Out of scope, refused with VLG_E_UNSUPPORTED before any launch when the batch has budgets: insertions and deletions (there is no
 * form for them), collective searches, integer-alphabet indexes, vlg_queries_occurrences, vlg_queries_intervals, vlg_wtsa_ranges,
 * vlg_wtsa_search_batch and vlg_wtsa_search_window_batch. */
vlg_status vlg_queries_set_mismatches(vlg_queries* q, const uint8_t* h_k);
vlg_status vlg_queries_get_mismatches(const vlg_queries* q, int* has_mismatches, uint8_t* h_k);

/* ------------------------------------------------------------------------------------------
 * Workspace, fused search, results.
 * ---------------------------------------------------------------------------------------- */
/* max_hbm_bytes bounds the scratch used per chunk of queries (0 = default 8 GiB). */
vlg_status vlg_workspace_create(uint64_t max_hbm_bytes, void* stream, vlg_workspace** out);
void vlg_workspace_destroy(vlg_workspace* ws);

/* The whole hot path for a batch, everything resident in HBM:
 *   per sub-pattern backward_search -> locate -> sort ascending -> gap-bounded merge join
 * = `idx.search(pat)` for every pattern (benchmark/gapped-matching/src/gm_search.cpp:91-121,
 *   index_sasearch.hpp:58-118) and `sdsl::locate(idx, query)` (include/sdsl/vlg_index.hpp:395-401).
 * Matches are the left-most, lazy, non-overlapping tuples of SURVEY.md Appendix C, bit-exact.
 * Every search (this one, vlg_join_batch, vlg_wtsa_search_batch, vlg_wtsa_search_window_batch) runs on the stream its workspace was
 * created with and synchronises it before it returns: the result can be fetched at once. */
vlg_status vlg_search_batch(const vlg_index* idx, const vlg_queries* q, vlg_workspace* ws, vlg_result** out);

/* K4 stand-alone (std::sort of one occurrence list, benchmark/gapped-matching/include/index_sasearch.hpp:80): every list
 * d_pos[h_off[l], h_off[l + 1]) of 32-bit positions < 2^position_bits is sorted ascending in place by the per-list sort of the batch
 * path.  mode 1: as "list_sort" = 1 above, mode 2: as 2, mode 3: as 1 with "sort_one_pass" = 0.  n_clustered (may be null) receives the number of long lists whose
 * positions were too clustered for the window pass (they took the four full passes).  Synchronises `stream` before it returns. */
vlg_status vlg_sort_lists_u32(uint32_t* d_pos, const uint64_t* h_off, uint64_t n_lists, uint32_t position_bits, int mode,
                              uint64_t* n_clustered, void* stream);
/* K5 on its own: the gap-bounded merge join of benchmark/gapped-matching/include/index_sasearch.hpp:85-116 (semantics of
 * vlg_iterator, include/sdsl/vlg_index.hpp:227-291) over caller-provided occurrence lists in HBM.
 *   d_lists      all lists concatenated, u64 positions, every list ascending (what std::sort leaves, index_sasearch.hpp:80);
 *                a position may not exceed 2^63
 *   h_list_off   [n_lists+1] element offsets of the lists inside d_lists
 *   h_join_list  [n_joins+1] join j uses the lists [h_join_list[j], h_join_list[j+1]) as its sub-patterns 0..k-1 (a list may
 *                not be shared between joins here: pass it twice); k <= VLG_MAX_SUBPATTERNS
 *   h_lo, h_hi   [n_lists] start-to-start distance bounds between a list and the previous one of its join (the entry of a
 *                join's first list is ignored); lo <= hi < 2^63
 *   h_end_len    [n_joins] length added to the last position of a match for the non-overlap rule (|s_{k-1}| for the library,
 *                |s_0| for index_sasearch.hpp:113)
 * The result is read like a search result: counts / offsets / first positions / tuples per join.  A join with an empty list
 * has no match (vlg_index.hpp:315-316).  Uses the workspace's window filter and chunking like vlg_search_batch. */
vlg_status vlg_join_batch(const uint64_t* d_lists, const uint64_t* h_list_off, uint64_t n_lists, const uint64_t* h_join_list,
                          const uint64_t* h_lo, const uint64_t* h_hi, const uint64_t* h_end_len, uint64_t n_joins,
                          vlg_workspace* ws, vlg_result** out);

typedef struct {
    uint64_t n_queries;
    uint64_t n_matches;           /* = gm_search's num_results (gm_search.cpp:110-114)          */
    uint64_t checksum;            /* = gm_search's checksum: sum of first positions mod 2^64    */
    uint64_t n_tuple_values;      /* sum over matches of k(query)                              */
    uint64_t located_occurrences; /* occurrences materialised by locate (each distinct SA interval of the
                                     batch is located once and shared by the queries that use it)     */
    uint64_t lf_steps;            /* LF steps taken by locate (csa_wt.hpp:338-341)              */
    uint64_t wt_levels_locate;    /* 32-byte super-block reads in locate                       */
    uint64_t wt_levels_bsearch;   /* 32-byte super-block reads in backward search              */
    uint64_t n_chunks;
    uint64_t logical_occurrences; /* sum of the list lengths the joins consumed (what the reference
                                     would locate query by query)                                 */
    uint64_t join_slots;          /* list elements the join passes evaluated: the non-final lists of every live
                                     query, after the window filter                               */
    uint64_t locate_mode;         /* how the last super-chunk's occurrences were located: VLG_LOCATE_*  */
    uint64_t filter_stream_segments; /* lists the window filter compacted, by how their survivors were kept: activity bits   */
    uint64_t filter_bit_segments;    /* of streamed queries, activity bits of pivot-filtered queries, index ranges of       */
    uint64_t filter_range_segments;  /* pivot-filtered queries ("pivot_range_ratio")                                          */
    uint64_t filter_survivors;       /* elements the joins read of those lists (the same however the joins were cut into chunks) */
    uint64_t filter_overflows;       /* groups of filtered queries whose survivors did not fit the room behind the lists at once:
                                        their join chunks compacted their own lists                                            */
} vlg_result_summary;
/* A batch with text windows (vlg_queries_set_windows): the lists are located whole, so located_occurrences, lf_steps, wt_levels_* and
 * locate_mode are those of the same batch without windows; logical_occurrences is the sum of the CUT lengths of the live queries (the
 * list lengths the joins consumed), and everything else -- matches, checksum, chunks, join slots, the filter's counters -- follows
 * from the cut lists. */
/* csa[i] = iterated LF to a sampled index (csa_wt.hpp:335-348), organised per batch as
 *   WALKS     one walk per occurrence (few occurrences; integer alphabets; workspace option "sweep" = 0)
 *   SWEEP     all occurrences advance together in SA order, walks that meet share their LF steps ("trail" = 1)
 *   UNSAMPLE  a batch that locates a large part of all text positions ("unsample_pct" per cent; default 0, off): one walker per SA
 *             sample rebuilds the whole suffix array -- n LF steps whatever the batch, each SA index visited once -- and the
 *             lists are copied out of it; recomputed for every batch, nothing is kept
 *   COPY      an index that keeps every SA value (sa_sample_dens = 1): no LF step at all                               */
enum { VLG_LOCATE_NONE = 0, VLG_LOCATE_WALKS = 1, VLG_LOCATE_SWEEP = 2, VLG_LOCATE_UNSAMPLE = 3, VLG_LOCATE_COPY = 4 };

vlg_status vlg_result_summary_get(const vlg_result* r, vlg_result_summary* s);
/* Copy to host.  counts[q] = matches of query q; offsets = exclusive prefix sum (n_queries+1);
 * first_positions = gapped_search_result::positions of every query, concatenated (utils.hpp:73-80);
 * tuples = every sub-pattern position of every match (vlg_iterator::operator[], vlg_index.hpp:337-340),
 * query-major, k(q) values per match.  Any pointer may be NULL. */
vlg_status vlg_result_fetch(const vlg_result* r, uint64_t* h_counts, uint64_t* h_offsets,
                            uint64_t* h_first_positions, uint64_t* h_tuples);
/* The same positions as 32-bit values, for callers that keep them that way: results of a text whose positions fit 32 bits
 * (vlg_index_info.n <= 2^32 + 1) are held 4 bytes wide in HBM and cross PCIe that way -- vlg_result_fetch widens them on the
 * host (threads, pinned staging blocks), this entry point copies them as they are.  VLG_E_INVALID when the result's positions
 * are 64 bits wide (larger texts, VLG_FORCE_POS64=1, vlg_wtsa_* results).  Either pointer may be NULL. */
vlg_status vlg_result_fetch32(const vlg_result* r, uint32_t* h_first_positions, uint32_t* h_tuples);
void vlg_result_destroy(vlg_result* r);

/* ------------------------------------------------------------------------------------------
 * The paper's index: vlg_index<alphabet_tag, wt_int<>> -- the text plus a wavelet tree over its suffix
 * array (include/sdsl/vlg_index.hpp:109-198, construct :375-392), searched lazily by vlg_iterator (:209-373): no occurrence list
 * is ever located or sorted; a match costs a few root-to-leaf walks of the tree, so the first matches of a query come cheaply
 * however long its lists are.  Byte texts (byte_alphabet_tag) and integer texts (int_alphabet_tag: symbols are uint32_t, a
 * query's sub-patterns whitespace-separated decimals, vlg_index.hpp:63-69).
 * On the device the tree is level-contiguous: level l is one rank-enabled bit-vector of 256-bit super-blocks (as K1), nodes are
 * intervals of it (wt_int, include/sdsl/wt_int.hpp:215-255).  Results equal sdsl::locate(vlg_index, query) -- the same tuples as
 * vlg_search_batch on the FM-index -- cut after max_matches_per_query matches of each query when that is not 0 (what a caller
 * that stops iterating early sees, include/sdsl/vlg_index.hpp:357-363).  One corner is defined away: for a query of one
 * sub-pattern of one symbol the reference's iterator drops an occurrence at 2j + 1 that directly follows a match at 2j
 * (vlg_index.hpp:254-266 with wt_helper.hpp:776-779); like the benchmark's merge join this library reports both.
 * ---------------------------------------------------------------------------------------- */
typedef struct vlg_wtsa vlg_wtsa;
typedef struct {
    uint64_t n;                   /* symbols + 1 (sentinel) = size of the suffix array                */
    uint32_t symbol_bytes;        /* 1 or 4                                                           */
    uint32_t levels;              /* bits per suffix-array value = levels of the tree                 */
    uint64_t blocks_per_level;    /* 32-byte super-blocks per level                                   */
    uint64_t hbm_bytes;           /* text + tree                                                      */
} vlg_wtsa_info;
/* symbol_bytes 1: h_text is uint8_t[n_symbols] without a 0 byte (VLG_E_ZERO_BYTE); 4: uint32_t[n_symbols], any values. */
vlg_status vlg_wtsa_build(const void* h_text, uint64_t n_symbols, uint32_t symbol_bytes, vlg_wtsa** out);
vlg_status vlg_wtsa_get_info(const vlg_wtsa* idx, vlg_wtsa_info* info);
void vlg_wtsa_destroy(vlg_wtsa* idx);
/* wt[i] (wt_int::operator[], include/sdsl/wt_int.hpp:339-361) = SA[i] for arbitrary indices.  Asynchronous on `stream`. */
vlg_status vlg_wtsa_sa_batch(const vlg_wtsa* idx, const uint64_t* d_i, uint64_t* d_out, uint64_t count, void* stream);
/* The two walks every search of this index is made of, on arbitrary suffix-array ranges [l, l + len): what the reference gets from
 * wt_int::expand(v) / expand(v, range) as vlg_iterator's wt_range_walker descends (include/sdsl/wt_int.hpp:824-939,
 * wt_helper.hpp:726-785).  quantile == 0: out[j] = number of SA[l, l + len) smaller than x[j]; quantile != 0: out[j] = the x[j]-th
 * smallest of them (0-based, x[j] < len[j]).  A range outside the suffix array (or x[j] >= len[j]) gives ~0.  Asynchronous on `stream`. */
vlg_status vlg_wtsa_range_walk_batch(const vlg_wtsa* idx, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_x, int quantile,
                                     uint64_t* d_out, uint64_t count, void* stream);
/* Level `level` of the tree as plain words (bit i = h_words[i >> 6] >> (i & 63), ceil(n / 64) words): bits [level * n, (level + 1) * n)
 * of wt_int::tree (include/sdsl/wt_int.hpp:162, 215-255) -- what m_wt.serialize stores (vlg_index.hpp:181-190). */
vlg_status vlg_wtsa_export_level(const vlg_wtsa* idx, uint32_t level, uint64_t* h_words);
/* The paper's index on disk: the file of vlg_index<alphabet_tag, wt_int<bit_vector_il<>, rank_support_il<>>> (the reference's default
 * tree type, include/sdsl/vlg_index.hpp:116-119), what `store_to_file(idx, file)` writes (vlg_index.hpp:181-198: m_text, then m_wt):
 *   m_text        int_vector<8> (byte_alphabet_tag): u64 size in bits, the bytes packed into u64 words; int_vector<0> (int_alphabet_tag):
 *                 u64 size in bits, u8 width, the packed words (include/sdsl/sdsl_concepts.hpp:48-49, int_vector.hpp:584-600)
 *   m_wt          wt_int::serialize (wt_int.hpp:708-732): u64 size n = |text| + 1, u64 sigma = n (one leaf per suffix-array value),
 *                 the tree, three supports that store nothing (bit_vector_il.hpp:339-346, 509-516), u32 max_level
 *                 L = hi(max(n - 1, 1)) + 1 (wt_int.hpp:194-204)
 *   the tree      bit_vector_il<512>::serialize (bit_vector_il.hpp:201-213) of S = n * L bits, level l = bits [l * n, (l + 1) * n):
 *                 u64 size S, u64 block_num = (S + 64) / 64 + (S + 512) / 512 + 1, u64 superblocks = (S + 512) / 512, u64 block_shift 9,
 *                 m_data (int_vector<64>: a cumulative count word before every 8 data words, data word i at i + i / 8 + 1, the total
 *                 ones last: :113-150) and m_rank_samples (int_vector<64>, empty unless block_num > 65536, then
 *                 min(1024, 1 << hi(superblocks)) count words in the BFS order of init_rank_samples, :87-104).
 * vlg_sdsl_wtsa_file_* parse such a file on the host only (no GPU needed); symbol_bytes 1 reads the byte tag, 4 the int tag.  Every
 * header field is checked against n and L (text size n - 1, max_level, sigma, the il sizes, block_shift, the data and rank-sample
 * lengths, a text width in 1..64), and a truncated file or trailing bytes are refused: VLG_E_INVALID -- which is also what a file
 * stored with the other alphabet tag gives, and a path that is not a regular file (a directory, a pipe).  The rank samples are
 * checked against the count words they copy.
 * vlg_wtsa_from_parts converts on the device: the data words are gathered into the device tree, an integer text is unpacked to
 * uint32_t.  Before a handle is returned the device checks that every cumulative count word and the final word equal the running
 * popcount, that the bits past S are zero, that level l holds as many ones as there are values v in [0, n) with bit L - 1 - l set
 * (true of every suffix-array tree), and that a byte text has no 0 byte; a failed check gives VLG_E_INVALID (VLG_E_ZERO_BYTE for the
 * 0 byte) and no handle, an integer symbol >= 2^32 VLG_E_UNSUPPORTED, n > 2^32 - 16 VLG_E_UNSUPPORTED.  Whether the tree is the suffix
 * array of the text is NOT checked, as the reference's load does not check it (vlg_index.hpp:193-197).  A loaded index equals the one
 * vlg_wtsa_build makes of the same text: the same device tree, the same text.
 * vlg_wtsa_load_sdsl = open + parts + from_parts.
 * vlg_wtsa_save_sdsl writes the file; text_width is the width of m_text: a byte index takes 0 or 8; an integer index takes 0 (the width
 * of the file it was loaded from, or hi(largest symbol) + 1, at least 1, for a built index) or 1..64 literally (VLG_E_INVALID when a
 * symbol does not fit) -- the reference keeps whatever width its text had (construct_im of an int_vector<> stores 64 bits a symbol).
 * vlg_wtsa_il_device assembles m_data (block_num words) of the tree into device memory d_words: what the save writes.  It is
 * asynchronous on `stream`, like the other entry points that take one: synchronise before reading d_words. */
typedef struct {
    uint64_t n;                   /* wt.size() = |text| + 1                                                                   */
    uint32_t symbol_bytes;        /* 1: byte_alphabet_tag, 4: int_alphabet_tag                                                */
    uint32_t levels;              /* wt.max_level = L                                                                         */
    const uint64_t* text_words;   /* m_text as stored: symbol i = bits [i * text_width, (i + 1) * text_width)                  */
    uint64_t text_count;          /* n - 1 symbols                                                                            */
    uint32_t text_width;          /* 8 for the byte tag, 1..64 for the int tag                                                */
    uint32_t reserved;
    const uint64_t* data;         /* bit_vector_il<512>::m_data                                                               */
    uint64_t data_words;          /* its block_num                                                                            */
    const uint64_t* rank_samples; /* bit_vector_il<512>::m_rank_samples                                                       */
    uint64_t n_rank_samples;
} vlg_wtsa_parts;
typedef struct vlg_sdsl_wtsa_file vlg_sdsl_wtsa_file;
vlg_status vlg_sdsl_wtsa_file_open(const char* path, uint32_t symbol_bytes, vlg_sdsl_wtsa_file** out);
vlg_status vlg_sdsl_wtsa_file_parts(const vlg_sdsl_wtsa_file* f, vlg_wtsa_parts* parts);   /* pointers stay valid until close */
void vlg_sdsl_wtsa_file_close(vlg_sdsl_wtsa_file* f);
vlg_status vlg_wtsa_from_parts(const vlg_wtsa_parts* h_parts, vlg_wtsa** out);
vlg_status vlg_wtsa_load_sdsl(const char* path, uint32_t symbol_bytes, vlg_wtsa** out);
vlg_status vlg_wtsa_save_sdsl(const vlg_wtsa* idx, const char* path, uint32_t text_width);
/* Asynchronous on `stream` (see above): synchronise before reading d_words. */
vlg_status vlg_wtsa_il_device(const vlg_wtsa* idx, uint64_t* d_words, uint64_t n_words, void* stream);
/* forward_search(text.begin(), text.end(), wt, 0, wt.size()-1, pat.begin(), pat.end(), sp, ep)
 * (include/sdsl/suffix_array_algorithm.hpp:48-112) for every sub-pattern of the batch: h_sp/h_ep receive the suffix-array
 * range [sp, ep] (sp = ep + 1: no occurrence).  Synchronises `stream`. */
vlg_status vlg_wtsa_ranges(const vlg_wtsa* idx, const vlg_queries* q, uint64_t* h_sp, uint64_t* h_ep, void* stream);
/* Integer-alphabet query batch: like vlg_queries_parse with VLG_DIALECT_LIBRARY, sub-patterns parsed as the reference parses them
 * for int_alphabet_tag (whitespace-separated decimals; gaps count symbols).  Only vlg_wtsa_* entry points accept such a batch. */
vlg_status vlg_queries_parse_int(const char* h_text, const uint64_t* h_off, uint64_t n_queries, int* h_status, vlg_queries** out);
/* the same through a symbol map (above): tokens are the ORIGINAL 64-bit symbols, the batch holds their mapped values */
vlg_status vlg_queries_parse_int_mapped(const vlg_symbol_map* map, const char* h_text, const uint64_t* h_off, uint64_t n_queries,
                                        int* h_status, vlg_queries** out);
/* sdsl::locate / count on the batch, at most max_matches_per_query matches each (0 = all). */
vlg_status vlg_wtsa_search_batch(const vlg_wtsa* idx, const vlg_queries* q, uint64_t max_matches_per_query, vlg_workspace* ws,
                                 vlg_result** out);
/* The same search inside a text window per query: query j is answered on [h_begin[j], h_end[j]) and its matches are exactly those of
 * the same query on the stand-alone text T[begin, end), with begin added to every position -- what a caller with a document
 * collection, or one that pages through matches, asks for.  An occurrence of a sub-pattern of m symbols counts only if it lies wholly
 * inside: begin <= v and v + m <= end.  h_begin / h_end are host arrays of vlg_queries_count(q) entries; a NULL h_begin means all
 * zeros, a NULL h_end "to the end of the text", an end beyond the text is clamped to it (and a begin beyond it is an empty window).
 * begin[j] > end[j] gives VLG_E_INVALID, decided on the host before any launch; a window shorter than a sub-pattern, or begin == end,
 * is an empty query and no error.  Gaps, end_len, max_matches_per_query and the workspace's "tuples" option keep their meaning; the
 * checksum is the sum over what is returned; byte and integer alphabets, parsed and caller-built batches are taken.
 * The occurrence list of a sub-pattern exists only as the sorted values of its suffix-array range, so the window is a rank interval of
 * it: two count_less walks per sub-pattern (wt_int::range_search_2d's descent to the value bounds, include/sdsl/wt_int.hpp:612-700),
 * nothing located, nothing sorted -- the cost follows the matches inside the window.  vlg_wtsa_search_batch is this call with two NULLs.
 * A batch that carries windows of its own (vlg_queries_set_windows) is refused here with VLG_E_INVALID.
 * (vlg_search_batch on the FM-index takes its windows from the batch, vlg_queries_set_windows: every list is located and sorted whole,
 * once, and a window is a cut of it -- the cost follows the lists, not the matches inside the window.  DESIGN.md 8.) */
vlg_status vlg_wtsa_search_window_batch(const vlg_wtsa* idx, const vlg_queries* q, const uint64_t* h_begin, const uint64_t* h_end,
                                        uint64_t max_matches_per_query, vlg_workspace* ws, vlg_result** out);
/* Where a search stopped, so that it can be continued as the reference's iterator continues (pull_forward, include/sdsl/vlg_index.hpp:254-266):
 * h_next[j] (vlg_queries_count entries) = the position at which the next search of query j has to begin -- the last position of its last
 * returned match + end_len, and never beyond the window's end, so that it can be passed back as it is -- when the query stopped at
 * max_matches_per_query; UINT64_MAX when it ran out of matches inside its window.  Searching again with begin[j] = next[j] and the same
 * end[j], without the queries that gave UINT64_MAX, yields the following matches: all pages together are the uncapped search of the
 * window, whatever the page size.  A query that returned exactly max_matches_per_query matches and has none left reports a position;
 * the following call returns no match and UINT64_MAX.  A result that does not come from a vlg_wtsa_* search gives VLG_E_INVALID. */
vlg_status vlg_result_next_positions(const vlg_result* r, uint64_t* h_next);
/* wt_int::range_search_2d(lb, rb, vlb, vrb) (include/sdsl/wt_int.hpp:612-700) on the tree over the suffix array, as a batched pair: the
 * occurrences of a suffix-array range whose text position lies in [vlb, vrb].
 * count:  d_count[j] = number of SA[d_l[j], d_l[j] + d_len[j]) with d_vlb[j] <= value <= d_vrb[j]
 *         (range_search_2d(lb, rb, vlb, vrb, false).first, wt_int.hpp:621-635)
 * report: those values, ASCENDING, range j written from d_out[d_out_off[j]] on; d_out_off = the exclusive prefix sum of the counts
 *         (count + 1 entries, as vlg_locate_batch takes it), total = d_out_off[count].
 * The reference returns (suffix-array index, value) pairs in the order of its descent; this returns the values alone, sorted: a text
 * position is what a caller of this index wants, and the index of a value would need a select structure the device tree does not keep.
 * A range outside the suffix array gives the count ~0 and writes nothing (like vlg_wtsa_range_walk_batch); vlb > vrb gives 0; a vrb
 * beyond every value is clamped.  Both calls are asynchronous on `stream`. */
vlg_status vlg_wtsa_range_count_batch(const vlg_wtsa* idx, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_vlb,
                                      const uint64_t* d_vrb, uint64_t* d_count, uint64_t count, void* stream);
vlg_status vlg_wtsa_range_report_batch(const vlg_wtsa* idx, const uint64_t* d_l, const uint64_t* d_len, const uint64_t* d_vlb,
                                       const uint64_t* d_vrb, const uint64_t* d_out_off, uint64_t count, uint64_t total,
                                       uint64_t* d_out, void* stream);

/* Per-kernel accounting of the last calls on this workspace (HIP events on the workspace stream).
 * Enabled with vlg_workspace_profile(ws, 1); reset by vlg_workspace_profile(ws, 1) again. */
typedef struct {
    char name[32];                /* "backward_search", "locate", "sort", "join", ...           */
    uint64_t launches;
    double total_ms;              /* sum of event-timed launch durations                       */
    uint64_t algorithmic_bytes;   /* SURVEY.md 8(d) accounting, 0 if not defined for the kernel */
} vlg_kernel_stat;
vlg_status vlg_workspace_profile(vlg_workspace* ws, int enable);
/* Options: "dedup" (default 1): share one located+sorted list between all sub-patterns of a batch that
 * have the same SA interval; 0 = locate every sub-pattern of every query separately like the reference.
 * "sweep" (default 1): locate by the synchronous sorted LF sweep (coalesced super-block reads) when the batch has
 * at least "sweep_min" occurrences (default 2^22); the last "sweep_tail" (default 2^22) stragglers and smaller
 * batches use the one-lane-per-occurrence random-access kernel.
 * "trail" (default 1, needs "dedup"): inside a sorted sweep an occurrence that steps onto an SA index another occurrence
 * has visited stops there and takes that occurrence's position plus the distance (csa[i] = csa[LF(i)] + 1 shared between
 * lanes), so a batch walks every LF trail once; 0 = every occurrence walks to its own sample like csa_wt::operator[].
 * "quad_walk" (default 1): the locate kernels walk LF on the quad image of an index that has one (vlg_index_quad_image) -- two tree
 * levels per dependent read; 0 = the binary tree (an A/B inside one library).  Results do not depend on it, "lf_steps" and
 * "wt_levels_locate" included.
 * "sweep_compact" (default 1): round 0 of the sorted sweep -- where most walks of a dense batch end -- writes the occurrences that go
 * on to another round densely and in order, and the round's partition by symbol sorts only them; 0 = a finished occurrence keeps its
 * place, is carried through the partition into its last bucket and dropped afterwards, as in every later round (an A/B inside one
 * library).  Results do not depend on it, "lf_steps" and "wt_levels_locate" included.  8 bytes of scratch per VLG_SWEEP_CHUNK (2048)
 * occurrences of a sweep.
 * "list_sort" (default 1): with 32-bit positions every occurrence list is sorted inside itself (short lists in LDS by value ranges;
 * long ones by two LSD radix passes over the top 16 position bits + one LDS pass over windows of whole groups; 2: four LSD passes
 * over all position bits, what lists with clustered positions take anyway); 0, or 64-bit positions: "global_sort_min" (default 2^20): from this many
 * occurrences on all lists are sorted by one radix sort of (list, position) keys instead of one segmented sort.
 * "sort_one_pass" (default 1; with "list_sort" = 1): a long list of at most VLG_ONE_PASS_MAX keys (131072) takes one radix pass, over
 * its top 8 position bits, in front of the window pass -- its groups are short enough for the windows as they are; 0 = every long list
 * takes the two passes (an A/B inside one library).  Results do not depend on it.
 * "filter" (default 1): before the join drop the list elements whose gap windows hold no element of the neighbouring
 * lists (they are in no match); "filter_min" (default 2^12) = join slots below which a query is joined as it is
 * ("filter_stream_min", default 2^16, for the queries filtered by streaming sweeps);
 * "filter_pivot" (default 1): filter outwards from the shortest list of a query when it is >= 6x shorter than all of
 * them together ("filter_pivot_ratio", default 6), otherwise (or with 0) by streaming sweeps over block bitmaps;
 * "pivot_range_ratio" (default 16): a query filtered from its shortest list keeps, for the lists it marks, the index ranges of the
 * windows (8 bytes per element of the shortest list and marked list) instead of a bit per list element when the marked lists
 * together are at least this many times longer than that; 0 = always bits.  Below 64 the ranges are the larger state (by up to
 * 68 / ratio), which counts against "filter_group_bytes": ratios below 8 are meant for tests;
 * "filter_group_bytes" (default 0 = a third of the join scratch) caps the filter state of the queries filtered together.
 * "class_intervals" (default 1024; 1 .. 2^20): SA intervals the frontier of one sub-pattern with character classes may hold at any step
 * of its backward search (32 bytes of scratch per interval and sub-pattern of a group; the sub-patterns of a batch are searched in groups
 * of 64 MiB of such scratch).  A frontier that would pass it: VLG_E_WORKSPACE (see vlg_queries_parse_classes).
 * "reserve" = bytes of scratch to allocate right away (at most the workspace's cap) instead of on first use.
 * "fuse_jump" (default 1): the link pass of the join finds, for the elements of a query's first list, where the next match can start
 * (the jump of the match chain) while it still holds their chain ends; 0 = a separate pass over all first lists does (an A/B inside
 * one library; the environment variable VLG_FUSE_JUMP=0 does the same for every workspace).  Queries of one sub-pattern take the
 * separate pass either way.
 * "tuples" (default 1): materialise every sub-pattern position of every match (what sdsl::locate returns); 0 = first
 * positions only, which is all the benchmark's gapped_search_result holds (index_sasearch.hpp:58-118): n_tuple_values
 * is 0 and vlg_result_fetch refuses a tuples buffer.
 * "emit_direct" (default 1; with "tuples" = 0 only): the pass that lists the matches of every chain tile writes their first
 * positions into the result itself, once the match counts have come back to the host and the result is allocated, and adds them into
 * the checksum; 0 = it writes the matches' slots into scratch and a gather pass turns them into positions (an A/B inside one library;
 * with tuples the gather pass runs either way).  Its time is in the kernel class "join_chain"; "gather" then has no launches.
 * "tile_scan" (default 1): the pass that resolves the match chain inside tiles of 1024 first-list elements finishes every element by
 * one backward scan of its tile in two levels (32 blocks of 32), half a wave per tile; 0 = pointer doubling, a workgroup per tile
 * (an A/B inside one library).  Both leave the same words.
 * "walk_wave" (default 1): a query whose first list spans at least 64 such tiles is walked from tile to tile by a whole wave, which
 * fetches the first 16 words of the next four tiles together with the current one and hops through them without another round trip;
 * 0 = one lane per query for all queries (an A/B inside one library).  Both leave the same records and counts.
 * Counts, first positions, tuples and the checksum are identical whatever the other options are. */
vlg_status vlg_workspace_set_option(vlg_workspace* ws, const char* name, int64_t value);
vlg_status vlg_workspace_kernel_stats(vlg_workspace* ws, vlg_kernel_stat* out, uint32_t cap, uint32_t* n);

/* The build-time constants the library was compiled with: the tile, run and chunk sizes of the kernels and the switches between
 * kept alternates (the VLG_* macros of csrc/, set with -D at build time), one {name, value} per constant, name = the macro's name
 * ("VLG_LINK_RUN", "VLG_RESOLVE_HOPS", ...).  *n = how many there are; at most cap are written.  Needs no device. */
typedef struct {
    char name[32];
    int64_t value;
} vlg_build_constant;
vlg_status vlg_build_constants(vlg_build_constant* out, uint32_t cap, uint32_t* n);

/* ------------------------------------------------------------------------------------------
 * Collective search (one process per GPU): ONE batch answered by all ranks of a communicator.
 * Every rank passes the same index image and the same query batch to vlg_search_batch, with a workspace of the same cap.  A batch
 * is cheap on one GPU because equal SA intervals are located once (vlg_result_summary.located_occurrences << logical_occurrences);
 * sharding only the query loop of gm_search.cpp:91-121 makes every rank locate the frequent lists again.  Here the DISTINCT LISTS are
 * sharded for locate + sort (a contiguous share of the lists in SA order per rank, equal occurrences), the sorted lists are exchanged
 * (one in-place all-gather of positions: the exchange step of this path), and the QUERIES are sharded for filter + join (contiguous
 * pieces of equal join work).  The result holds this rank's queries (vlg_result_owned_queries; counts of the others are 0); counts,
 * checksums and located occurrences are summed over the ranks by the caller (vlg_comm_allreduce_sum_u64).
 * vlg_workspace_set_comm: exchange by RCCL (vlg_comm_allgatherv); NULL = back to single-GPU searches.
 * vlg_workspace_set_exchange: the caller moves the bytes -- `fn` must all-gather IN PLACE: d_buf holds this rank's piece at the offset
 * of the pieces before it (h_counts[r] elements of elem_bytes per rank r), afterwards every piece; work it enqueues must be ordered
 * with `stream`.  (Hosts without RCCL between their ranks; rehearsals with several ranks on one device.) */
typedef int (*vlg_exchange_fn)(void* ctx, void* d_buf, const uint64_t* h_counts, uint32_t elem_bytes, int n_ranks, int rank, void* stream);
vlg_status vlg_workspace_set_comm(vlg_workspace* ws, void* nccl_comm);
vlg_status vlg_workspace_set_exchange(vlg_workspace* ws, int n_ranks, int rank, vlg_exchange_fn fn, void* ctx);
/* The exchange step as it runs by default over a communicator: PAIRWISE and NEEDED-ONLY.  Every rank knows the whole plan of the
 * batch (which rank sorts which list, which rank joins which queries), so a sorted list travels only to the ranks whose queries
 * use it: the lists a rank owes a peer are packed into one buffer per peer and sent point to point -- vlg_comm_alltoallv, one
 * grouped ncclSend / ncclRecv pair per peer, one xGMI link each -- instead of every list visiting every rank in a ring.  Workspace
 * option "exchange_all" = 1 goes back to the in-place all-gather of everything (vlg_comm_allgatherv).
 * vlg_workspace_set_exchange_alltoall: the same with the caller moving the bytes (hosts without RCCL between their ranks,
 * rehearsals on one device): fn sends h_send_counts[r] elements to rank r (packed in rank order at d_send) and receives
 * h_recv_counts[r] from it (packed at d_recv), its own piece included, ordered with `stream`.
 * Before the payload moves, the ranks all-gather ONE status word each: a rank whose part of the batch failed up to there (workspace
 * too small for its share, out of memory, a failed kernel) tells the others, and vlg_search_batch returns an error on EVERY rank --
 * its own on the failed one, VLG_E_INTERNAL "rank r failed ..." on its peers -- instead of leaving them inside a collective.
 * An error after the exchange (in a rank's joins) is that rank's alone: the product issues no further collective; a caller that
 * reduces counters afterwards (vlg_comm_allreduce_sum_u64) has to handle it like any failure of one of its own ranks. */
vlg_status vlg_comm_alltoallv(void* nccl_comm, const void* d_send, const uint64_t* h_send_counts, void* d_recv,
                              const uint64_t* h_recv_counts, uint32_t elem_bytes, void* stream);
typedef int (*vlg_alltoall_fn)(void* ctx, const void* d_send, const uint64_t* h_send_counts, void* d_recv, const uint64_t* h_recv_counts,
                               uint32_t elem_bytes, int n_ranks, int rank, void* stream);
vlg_status vlg_workspace_set_exchange_alltoall(vlg_workspace* ws, int n_ranks, int rank, vlg_alltoall_fn fn, void* ctx);
/* [begin, end) pairs of the queries this rank joined in a collective search (n_ranges = 0: a single-GPU search, all of them) */
vlg_status vlg_result_owned_queries(const vlg_result* r, uint64_t* h_ranges, uint32_t cap_ranges, uint32_t* n_ranges);

#ifdef __cplusplus
}
#endif
#endif /* VLG_HIP_H */
