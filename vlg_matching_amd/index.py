"""Host-side mirror of the reference interface for the VLG hot path.

  VlgIndex          ~ sdsl::vlg_index<> / the benchmark index concept (construct, serialize/load via parts, search)
  count / locate    ~ sdsl::count / sdsl::locate (include/sdsl/vlg_index.hpp:395-411)
  VlgIndex.search   ~ index_*::search for a batch of gapped_pattern (benchmark/gapped-matching/src/gm_search.cpp:91-121)
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import VlgError, check, lib

NODE_DTYPE = np.dtype([("bv_pos", "<u8"), ("bv_pos_rank", "<u8"), ("parent", "<u2"), ("child", "<u2", (2,))], align=True)
assert NODE_DTYPE.itemsize == C.sizeof(capi.WtNode)


def _u8(a):
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    if isinstance(a, str):
        return np.frombuffer(a.encode("latin-1"), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


NO_NEXT = (1 << 64) - 1           # SearchResult.next_positions(): the query ran out of matches


class SearchResult:
    """Per-query match counts, first positions (gapped_search_result::positions) and full tuples."""

    def __init__(self, handle, ks):
        self._h = handle
        self._ks = ks
        s = capi.ResultSummary()
        check(lib().vlg_result_summary_get(handle, C.byref(s)))
        self.summary = {k: int(getattr(s, k)) for k, _ in capi.ResultSummary._fields_}
        self._fetched = None

    def __del__(self):
        try:
            if self._h:
                lib().vlg_result_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def owned_queries(self):
        """[(begin, end), ...] of the queries this rank joined in a collective search; [] after a single-GPU search (all of them)"""
        n = C.c_uint32()
        check(lib().vlg_result_owned_queries(self._h, None, 0, C.byref(n)))
        r = np.zeros(2 * max(n.value, 1), dtype=np.uint64)
        check(lib().vlg_result_owned_queries(self._h, r.ctypes.data, n.value, C.byref(n)))
        return [(int(r[2 * i]), int(r[2 * i + 1])) for i in range(n.value)]

    def fetch(self):
        if self._fetched is None:
            nq = self.summary["n_queries"]
            counts = np.zeros(max(nq, 1), dtype=np.uint64)
            offsets = np.zeros(nq + 1, dtype=np.uint64)
            first = np.zeros(max(self.summary["n_matches"], 1), dtype=np.uint64)
            tuples = np.zeros(max(self.summary["n_tuple_values"], 1), dtype=np.uint64)
            has_tuples = self.summary["n_tuple_values"] or not self.summary["n_matches"]       # workspace option "tuples" = 0: none
            check(lib().vlg_result_fetch(self._h, counts.ctypes.data, offsets.ctypes.data, first.ctypes.data,
                                         tuples.ctypes.data if has_tuples else None))
            self._fetched = (counts[:nq], offsets, first[: self.summary["n_matches"]], tuples[: self.summary["n_tuple_values"]])
        return self._fetched

    def fetch_into(self, counts_ptr, offsets_ptr, first_ptr, tuples_ptr):
        """vlg_result_fetch into caller-provided host buffers (e.g. pinned memory); any pointer may be None."""
        check(lib().vlg_result_fetch(self._h, counts_ptr, offsets_ptr, first_ptr, tuples_ptr))

    def fetch32_into(self, first_ptr, tuples_ptr):
        """vlg_result_fetch32: the positions as they are held in HBM when they fit 32 bits (VlgError otherwise)."""
        check(lib().vlg_result_fetch32(self._h, first_ptr, tuples_ptr))

    def fetch32(self):
        first = np.zeros(max(self.summary["n_matches"], 1), dtype=np.uint32)
        tuples = np.zeros(max(self.summary["n_tuple_values"], 1), dtype=np.uint32)
        self.fetch32_into(first.ctypes.data, tuples.ctypes.data if self.summary["n_tuple_values"] else None)
        return first[: self.summary["n_matches"]], tuples[: self.summary["n_tuple_values"]]

    def next_positions(self):
        """vlg_result_next_positions: per query, where the next search has to begin to continue this one (a WtsaIndex.search that
        stopped at max_matches), NO_NEXT (2^64 - 1) when the query ran out of matches inside its window.  VlgError for the result
        of any other search."""
        nq = self.summary["n_queries"]
        nxt = np.zeros(max(nq, 1), dtype=np.uint64)
        check(lib().vlg_result_next_positions(self._h, nxt.ctypes.data))
        return nxt[:nq]

    def class_intervals(self):
        """vlg_result_class_intervals: the SA intervals of every sub-pattern of a batch with character classes (Queries.from_classes)
        -> (ivoff[nsub + 1], l[], r[]): sub-pattern s has the intervals [l[j], r[j]], ivoff[s] <= j < ivoff[s + 1], ascending and
        disjoint.  VlgError for the result of a batch without classes."""
        nsub = int(np.sum(np.asarray(self._ks, dtype=np.int64)))
        off = np.zeros(nsub + 1, dtype=np.uint64)
        check(lib().vlg_result_class_intervals(self._h, off.ctypes.data, None, None))
        l, r = np.zeros(max(int(off[-1]), 1), np.uint64), np.zeros(max(int(off[-1]), 1), np.uint64)
        check(lib().vlg_result_class_intervals(self._h, off.ctypes.data, l.ctypes.data, r.ctypes.data))
        return off, l[: int(off[-1])], r[: int(off[-1])]

    def list_documents(self, documents, pairs=True):
        """vlg_result_list_documents: which documents each query matches, reduced on the device -> DocListing.  pairs=False computes
        only df (and the number of pairs)."""
        h = C.c_void_p()
        check(lib().vlg_result_list_documents(self._h, documents._h, capi.DOCLIST_PAIRS if pairs else capi.DOCLIST_DF, C.byref(h)))
        return DocListing(h, bool(pairs))

    def extract_matches(self, queries, text_access, flank=0, documents=None, matches=None, max_symbols=0):
        """vlg_result_extract_matches: the text every match matched, extracted on the device -> MatchTexts.  `queries` is the Queries
        batch that was searched, `text_access` a TextAccess of an index of the same text.  flank: an int or (left, right), None on a
        side = to the bound (the text's ends, or the ends of the document of the match's first position when `documents` is given);
        matches: (begin, end) in the numbering of fetch(), end None = to the last match; max_symbols: refuse a slice with more
        symbols before they are allocated (0: no cap)."""
        left, right = flank if isinstance(flank, (tuple, list)) else (flank, flank)
        left, right = (NO_NEXT if f is None else int(f) for f in (left, right))
        begin, end = (0, None) if matches is None else matches
        if left < 0 or right < 0 or int(begin) < 0 or (end is not None and int(end) < 0) or int(max_symbols) < 0:
            raise ValueError("flank, matches and max_symbols are non-negative")
        h = C.c_void_p()
        check(lib().vlg_result_extract_matches(self._h, queries._h, text_access._h, documents._h if documents is not None else None, left, right,
                                               int(begin), NO_NEXT if end is None else int(end), int(max_symbols), C.byref(h)))
        return MatchTexts(h)

    @property
    def counts(self):
        return self.fetch()[0]

    def positions(self, q):
        _, off, first, _ = self.fetch()
        return first[int(off[q]): int(off[q + 1])]

    def tuples(self, q):
        counts, _, _, tup = self.fetch()
        if self.summary["n_matches"] and not self.summary["n_tuple_values"]:
            raise VlgError(capi.E_INVALID, "tuples were not materialised (workspace option \"tuples\" is 0)")
        ks = np.asarray(self._ks, dtype=np.uint64)
        toff = np.concatenate([[0], np.cumsum(counts * ks)]).astype(np.int64)
        k = int(ks[q])
        return tup[toff[q]: toff[q + 1]].reshape(-1, max(k, 1)) if k else np.zeros((0, 0), np.uint64)


class DocListing:
    """The documents each query of a result matches (vlg_doc_listing), on the device until an attribute asks for it: query q owns the
    pairs [offsets[q], offsets[q + 1]); pair p says that `counts[p]` consecutive matches of q, from match `first_match[p]` of the
    result on, begin in document `docs[p]`.  df[q] is the number of pairs of q.  A listing made with pairs=False has df and offsets only."""

    def __init__(self, handle, has_pairs):
        self._h = handle
        self.has_pairs = has_pairs
        nq, npairs = C.c_uint64(), C.c_uint64()
        check(lib().vlg_doc_listing_info(handle, C.byref(nq), C.byref(npairs)))
        self.n_queries, self.n_pairs = int(nq.value), int(npairs.value)
        self._df = self._pairs = None

    def __del__(self):
        try:
            if self._h:
                lib().vlg_doc_listing_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def fetch_into(self, df_ptr, offsets_ptr, docs_ptr, counts_ptr, first_match_ptr):
        """vlg_doc_listing_fetch into caller-provided host buffers; any pointer may be None."""
        check(lib().vlg_doc_listing_fetch(self._h, df_ptr, offsets_ptr, docs_ptr, counts_ptr, first_match_ptr))

    def _fetch_df(self):
        if self._df is None:
            df, off = np.zeros(max(self.n_queries, 1), np.uint64), np.zeros(self.n_queries + 1, np.uint64)
            self.fetch_into(df.ctypes.data, off.ctypes.data, None, None, None)
            self._df = (df[: self.n_queries], off)
        return self._df

    def _fetch_pairs(self):
        if self._pairs is None:
            a = [np.zeros(max(self.n_pairs, 1), np.uint64) for _ in range(3)]
            self.fetch_into(None, None, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data)       # (VlgError for a df-only listing)
            self._pairs = tuple(x[: self.n_pairs] for x in a)
        return self._pairs

    df = property(lambda self: self._fetch_df()[0])
    offsets = property(lambda self: self._fetch_df()[1])
    docs = property(lambda self: self._fetch_pairs()[0])
    counts = property(lambda self: self._fetch_pairs()[1])
    first_match = property(lambda self: self._fetch_pairs()[2])

    def of(self, q):
        """-> (docs, counts, first_match) of query q"""
        a, b = int(self.offsets[q]), int(self.offsets[q + 1])
        return self.docs[a:b], self.counts[a:b], self.first_match[a:b]


class MatchTexts:
    """The texts of a slice of a result's matches (vlg_match_texts), on the device until fetched: text i of the slice is
    symbols[offsets[i] : offsets[i + 1]] and begins at text position begin[i] (a sub-pattern's offset inside its text is its tuple
    value - begin[i]).  Symbols are uint8 for a byte index, the original uint32 symbols for an integer one."""

    def __init__(self, handle):
        self._h = handle
        nm, ns, sb = C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(lib().vlg_match_texts_info(handle, C.byref(nm), C.byref(ns), C.byref(sb)))
        self.n_matches, self.n_symbols = int(nm.value), int(ns.value)
        self.symbol_dtype = np.uint32 if sb.value == 4 else np.uint8
        self._fetched = None

    def __del__(self):
        try:
            if self._h:
                lib().vlg_match_texts_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def fetch_into(self, offsets_ptr, begin_ptr, symbols_ptr):
        """vlg_match_texts_fetch into caller-provided host buffers; any pointer may be None."""
        check(lib().vlg_match_texts_fetch(self._h, offsets_ptr, begin_ptr, symbols_ptr))

    def fetch(self):
        """-> (offsets[n_matches + 1], begin[n_matches], symbols[n_symbols])"""
        if self._fetched is None:
            off, beg = np.zeros(self.n_matches + 1, np.uint64), np.zeros(max(self.n_matches, 1), np.uint64)
            sym = np.zeros(max(self.n_symbols, 1), self.symbol_dtype)
            self.fetch_into(off.ctypes.data, beg.ctypes.data, sym.ctypes.data)
            self._fetched = (off, beg[: self.n_matches], sym[: self.n_symbols])
        return self._fetched

    def of(self, i):
        """text i of the slice -> bytes (byte index) or np.uint32 array (integer index)"""
        off, _, sym = self.fetch()
        s = sym[int(off[i]): int(off[i + 1])]
        return s if self.symbol_dtype == np.uint32 else s.tobytes()


def read_sdsl_file(path, dens=32, rrr=False):
    """Host-only parse of a stock sdsl csa_wt<wt_huff<>> file (rrr: csa_wt<wt_huff<rrr_vector<63>>>, its blocks decoded back to
    plain bits) -> parts dict (same keys as VlgIndex.export_parts())."""
    f = C.c_void_p()
    check(lib().vlg_sdsl_file_open_kind(str(path).encode(), dens, 1 if rrr else 0, C.byref(f)))
    try:
        p = capi.IndexParts()
        check(lib().vlg_sdsl_file_parts(f, C.byref(p)))
        nw = (p.bv_bits + 63) // 64
        return {"n": int(p.n), "sigma": int(p.sigma), "dens": int(p.sa_sample_dens),
                "char2comp": np.ctypeslib.as_array(C.cast(p.char2comp, C.POINTER(C.c_uint8)), shape=(256,)).copy(),
                "C": np.ctypeslib.as_array(C.cast(p.C, C.POINTER(C.c_uint64)), shape=(p.sigma + 1,)).copy(),
                "bv_bits": int(p.bv_bits),
                "bv_words": np.ctypeslib.as_array(C.cast(p.bv_words, C.POINTER(C.c_uint64)), shape=(max(nw, 1),))[:nw].copy(),
                "nodes": np.frombuffer(C.string_at(p.nodes, p.n_nodes * C.sizeof(capi.WtNode)), dtype=NODE_DTYPE).copy(),
                "samples": np.ctypeslib.as_array(C.cast(p.sa_samples, C.POINTER(C.c_uint64)), shape=(max(p.n_samples, 1),))[: p.n_samples].copy()}
    finally:
        lib().vlg_sdsl_file_close(f)


def read_sdsl_int_file(path, dens=32, rrr=False):
    """Host-only parse of a stock sdsl csa_wt<wt_int<>, dens, ., sa_order_sa_sampling<>, isa_sampling<>, int_alphabet<>> file (rrr: over
    wt_int<rrr_vector<63>>, its blocks decoded back to plain bits) -> dict: n, sigma, max_level, dens, comp2char, C, tree_bits,
    tree_words (wt_int::tree, level l = bits [l * n, (l + 1) * n)), samples."""
    f = C.c_void_p()
    check(lib().vlg_sdsl_int_file_open(str(path).encode(), dens, 1 if rrr else 0, C.byref(f)))
    try:
        p = capi.IntIndexParts()
        check(lib().vlg_sdsl_int_file_parts(f, C.byref(p)))
        nw = (p.tree_bits + 63) // 64

        def u64(ptr, count):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(max(count, 1),))[:count].copy()
        return {"n": int(p.n), "sigma": int(p.sigma), "max_level": int(p.max_level), "dens": int(p.sa_sample_dens),
                "comp2char": u64(p.comp2char, p.sigma), "C": u64(p.C, p.sigma + 1), "tree_bits": int(p.tree_bits),
                "tree_words": u64(p.tree_words, nw), "samples": u64(p.sa_samples, p.n_samples)}
    finally:
        lib().vlg_sdsl_int_file_close(f)


def _wtsa_parts_dict(p):
    def u64(ptr, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(max(count, 1),))[:count].copy() if count else np.zeros(0, np.uint64)
    count, width = int(p.text_count), int(p.text_width)
    words = u64(p.text_words, (count * width + 63) // 64)
    return {"n": int(p.n), "symbol_bytes": int(p.symbol_bytes), "levels": int(p.levels), "text_width": width, "text_count": count,
            "text_words": words, "text": _unpack_symbols(words, count, width, int(p.symbol_bytes)),
            "data": u64(p.data, p.data_words), "rank_samples": u64(p.rank_samples, p.n_rank_samples)}


def _unpack_symbols(words, count, width, symbol_bytes):
    """int_vector words -> the symbols (uint8 for the byte tag, uint64 for the int tag)"""
    if symbol_bytes == 1:
        return words.view(np.uint8)[:count].copy()
    i = np.arange(count, dtype=np.uint64) * np.uint64(width)
    w, o = (i >> np.uint64(6)).astype(np.int64), i & np.uint64(63)
    ext = np.concatenate([words, np.zeros(1, np.uint64)])
    lo = ext[w] >> o
    sh = (np.uint64(64) - o) & np.uint64(63)
    hi = np.where(o + np.uint64(width) > np.uint64(64), ext[w + 1] << sh, np.uint64(0))
    v = lo | hi
    return v if width == 64 else v & np.uint64((1 << width) - 1)


def read_sdsl_wtsa_file(path, int_alphabet=False):
    """Host-only parse of a stock sdsl vlg_index<byte_alphabet_tag> file (int_alphabet: vlg_index<int_alphabet_tag>), tree type
    wt_int<bit_vector_il<>, rank_support_il<>> -> dict: n, symbol_bytes, levels, text_width, text_count, text_words (m_text as stored),
    text (its symbols), data (bit_vector_il<512>::m_data), rank_samples."""
    f = C.c_void_p()
    check(lib().vlg_sdsl_wtsa_file_open(str(path).encode(), 4 if int_alphabet else 1, C.byref(f)))
    try:
        p = capi.WtsaParts()
        check(lib().vlg_sdsl_wtsa_file_parts(f, C.byref(p)))
        return _wtsa_parts_dict(p)
    finally:
        lib().vlg_sdsl_wtsa_file_close(f)


class Workspace:
    def __init__(self, max_hbm_bytes=0, stream=None):
        h = C.c_void_p()
        check(lib().vlg_workspace_create(int(max_hbm_bytes), stream, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().vlg_workspace_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_option(self, name, value):
        check(lib().vlg_workspace_set_option(self._h, name.encode(), int(value)))

    def set_comm(self, comm):
        """Collective searches over the ranks of an RCCL communicator (vlg_matching_amd.dist.Comm): the distinct lists of a batch are
        sharded for locate + sort and all-gathered, the queries are sharded for the joins.  None: single-GPU searches again."""
        check(lib().vlg_workspace_set_comm(self._h, comm._h if comm is not None else None))
        self._comm = comm

    def set_exchange(self, n_ranks, rank, callback):
        """The same with the caller moving the bytes: callback(d_buf, counts, elem_bytes, n_ranks, rank, stream) -> 0, an in-place
        all-gather of device pieces (vlg_workspace_set_exchange)."""
        def trampoline(ctx, d_buf, counts_ptr, elem_bytes, n, r, stream):
            try:
                return int(callback(d_buf, [int(counts_ptr[i]) for i in range(n)], int(elem_bytes), int(n), int(r), stream) or 0)
            except Exception as e:                                   # an exception must not cross the C frame
                import sys
                print("exchange callback failed: %r" % (e,), file=sys.stderr)
                return 1
        self._exchange_cb = capi.EXCHANGE_FN(trampoline)
        check(lib().vlg_workspace_set_exchange(self._h, int(n_ranks), int(rank), self._exchange_cb, None))

    def set_exchange_alltoall(self, n_ranks, rank, callback):
        """The pairwise exchange with the caller moving the bytes (vlg_workspace_set_exchange_alltoall):
        callback(d_send, send_counts, d_recv, recv_counts, elem_bytes, n_ranks, rank, stream) -> 0 sends send_counts[r] elements to rank r
        (packed in rank order at d_send) and receives recv_counts[r] from it (packed at d_recv)."""
        def trampoline(ctx, d_send, sc, d_recv, rc, elem_bytes, n, r, stream):
            try:
                return int(callback(d_send or 0, [int(sc[i]) for i in range(n)], d_recv or 0, [int(rc[i]) for i in range(n)], int(elem_bytes),
                                    int(n), int(r), stream) or 0)
            except Exception as e:                                   # an exception must not cross the C frame
                import sys
                print("exchange callback failed: %r" % (e,), file=sys.stderr)
                return 1
        self._exchange_cb = capi.ALLTOALL_FN(trampoline)
        check(lib().vlg_workspace_set_exchange_alltoall(self._h, int(n_ranks), int(rank), self._exchange_cb, None))

    def profile(self, enable=True):
        check(lib().vlg_workspace_profile(self._h, 1 if enable else 0))

    def kernel_stats(self):
        arr = (capi.KernelStat * 32)()
        n = C.c_uint32()
        check(lib().vlg_workspace_kernel_stats(self._h, arr, 32, C.byref(n)))
        return {arr[i].name.decode(): dict(launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                                           algorithmic_bytes=int(arr[i].algorithmic_bytes)) for i in range(min(n.value, 32))}


class SymbolMap:
    """vlg_symbol_map: the sorted distinct symbols of a 64-bit integer text, symbol -> rank + 1 (dense, order-preserving, never 0).
    The device indexes hold uint32 symbols; a text with larger ones is mapped, indexed, and queried through the same map."""

    def __init__(self, text):
        t = np.ascontiguousarray(text, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vlg_symbol_map_create(t.ctypes.data if len(t) else None, len(t), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().vlg_symbol_map_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def sigma(self):
        return int(lib().vlg_symbol_map_sigma(self._h))

    def symbols(self):
        out = np.zeros(self.sigma, dtype=np.uint64)
        check(lib().vlg_symbol_map_symbols(self._h, out.ctypes.data if len(out) else None))
        return out

    def apply(self, symbols):
        """-> uint32 array: rank + 1 of every symbol (sigma + 1 for a symbol the map's text does not hold)"""
        t = np.ascontiguousarray(symbols, dtype=np.uint64)
        out = np.zeros(len(t), dtype=np.uint32)
        check(lib().vlg_symbol_map_apply(self._h, t.ctypes.data if len(t) else None, len(t), out.ctypes.data if len(t) else None))
        return out

    def queries(self, regexps, strict=True):
        return Queries.from_int(regexps, strict=strict, symbol_map=self)


def parse_query(regexp, dialect=capi.DIALECT_LIBRARY):
    """gapped_pattern_query / gapped_pattern on the host: -> (sub-patterns, lo[], hi[], end_len).  Raises VlgError(E_PARSE)."""
    raw = regexp.encode("latin-1") if isinstance(regexp, str) else bytes(regexp)
    p = capi.ParsedQuery()
    check(lib().vlg_parse_query(raw, len(raw), dialect, C.byref(p)))
    subs = [raw[p.sub_off[i]: p.sub_off[i] + p.sub_len[i]] for i in range(p.k)]
    return subs, [int(p.lo[i]) for i in range(1, p.k)], [int(p.hi[i]) for i in range(1, p.k)], int(p.end_len)


def parse_class_query(regexp):
    """The library dialect with character classes on the host (vlg_parse_class_query): -> (sub-patterns, lo[], hi[], end_len), a
    sub-pattern being a uint8 array [positions, 32] of 256-bit sets (bit c of a row = byte c is accepted; class_mask_members reads
    one).  Lengths count positions.  Raises VlgError(E_PARSE / E_INVALID)."""
    raw = regexp.encode("latin-1") if isinstance(regexp, str) else bytes(regexp)
    p = capi.ParsedQuery()
    n = C.c_uint64()
    masks = np.zeros((max(len(raw), 1), 32), dtype=np.uint8)           # (a position takes at least one byte of the query)
    check(lib().vlg_parse_class_query(raw, len(raw), C.byref(p), masks.ctypes.data, len(masks), C.byref(n)))
    subs = [masks[p.sub_off[i]: p.sub_off[i] + p.sub_len[i]].copy() for i in range(p.k)]
    return subs, [int(p.lo[i]) for i in range(1, p.k)], [int(p.hi[i]) for i in range(1, p.k)], int(p.end_len)


def class_mask_members(row):
    """the bytes a 32-byte mask row accepts, ascending"""
    return np.flatnonzero(np.unpackbits(np.asarray(row, dtype=np.uint8), bitorder="little")).astype(np.uint8)


def class_mask(members):
    """the 32-byte mask row that accepts exactly `members` (bytes or integers)"""
    bits = np.zeros(256, dtype=np.uint8)
    bits[np.frombuffer(bytes(members), dtype=np.uint8) if isinstance(members, (bytes, bytearray)) else np.asarray(list(members), dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little")


class Queries:
    """A parsed query batch resident in HBM."""

    def __init__(self, regexps, dialect=capi.DIALECT_LIBRARY, strict=True):
        raws = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in regexps]
        off = np.zeros(len(raws) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in raws])
        text = b"".join(raws)
        h = C.c_void_p()
        status = np.zeros(max(len(raws), 1), dtype=np.int32)
        check(lib().vlg_queries_parse(text, off.ctypes.data, len(raws), dialect, None if strict else status.ctypes.data, C.byref(h)))
        self._h = h
        self.status = status[: len(raws)]
        self.n = len(raws)

    @classmethod
    def from_blob(cls, text, off, dialect=capi.DIALECT_LIBRARY):
        """The regexps already concatenated (query i = text[off[i], off[i+1])): one vlg_queries_parse call, nothing else."""
        self = cls.__new__(cls)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vlg_queries_parse(text, off.ctypes.data, len(off) - 1, dialect, None, C.byref(h)))
        self._h = h
        self.n = len(off) - 1
        self.status = np.zeros(self.n, dtype=np.int32)
        return self

    @classmethod
    def from_int(cls, regexps, strict=True, symbol_map=None):
        """Integer-alphabet batch (gapped_pattern_query<int_alphabet_tag>): sub-patterns are whitespace-separated decimals, gaps count
        symbols -- for an integer-alphabet index (VlgIndex.build_int) or WtsaIndex over an integer text.  symbol_map: the SymbolMap
        the index's text went through (64-bit symbols): tokens are the original symbols."""
        raws = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in regexps]
        off = np.zeros(len(raws) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in raws])
        self = cls.__new__(cls)
        h = C.c_void_p()
        status = np.zeros(max(len(raws), 1), dtype=np.int32)
        st = None if strict else status.ctypes.data
        if symbol_map is not None:
            check(lib().vlg_queries_parse_int_mapped(symbol_map._h, b"".join(raws), off.ctypes.data, len(raws), st, C.byref(h)))
        else:
            check(lib().vlg_queries_parse_int(b"".join(raws), off.ctypes.data, len(raws), st, C.byref(h)))
        self._h, self.n, self.status = h, len(raws), status[: len(raws)]
        return self

    @classmethod
    def from_classes(cls, regexps, strict=True):
        """The library dialect with character classes (vlg_queries_parse_classes): a[bc]d, [^a], \\[ ...; VlgIndex.search takes the
        batch as any other.  A batch in which no position accepts more than one byte is the batch Queries(regexps) makes."""
        raws = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in regexps]
        off = np.zeros(len(raws) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in raws])
        self = cls.__new__(cls)
        h = C.c_void_p()
        status = np.zeros(max(len(raws), 1), dtype=np.int32)
        check(lib().vlg_queries_parse_classes(b"".join(raws), off.ctypes.data, len(raws), None if strict else status.ctypes.data, C.byref(h)))
        self._h, self.n, self.status = h, len(raws), status[: len(raws)]
        return self

    @classmethod
    def from_class_arrays(cls, subpatterns, lo, hi, end_len):
        """As from_arrays with mask rows for bytes (vlg_queries_create_classes): subpatterns is a list (per query) of lists of uint8
        arrays [positions, 32] (class_mask builds a row); lo / hi: per query lists of k-1 start-to-start bounds, in positions."""
        self = cls.__new__(cls)
        rows, suboff, qsub, flo, fhi = [], [0], [0], [], []
        for subs, l, h in zip(subpatterns, lo, hi):
            for i, s in enumerate(subs):
                s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 32)
                rows.append(s)
                suboff.append(suboff[-1] + len(s))
                flo.append(0 if i == 0 else int(l[i - 1]))
                fhi.append(0 if i == 0 else int(h[i - 1]))
            qsub.append(len(suboff) - 1)
        m = np.ascontiguousarray(np.concatenate(rows + [np.zeros((1, 32), np.uint8)]))
        a = [np.asarray(x, dtype=np.uint64) for x in (suboff, qsub, flo + [0], fhi + [0], list(end_len) + [0])]
        hq = C.c_void_p()
        check(lib().vlg_queries_create_classes(m.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                               a[4].ctypes.data, len(subpatterns), C.byref(hq)))
        self._h, self.n, self.status = hq, len(subpatterns), np.zeros(len(subpatterns), dtype=np.int32)
        return self

    def subpattern_range(self):
        """qsub[nq+1]: query i owns the sub-patterns [qsub[i], qsub[i+1]) of the batch"""
        return np.concatenate([[0], np.cumsum(self.ks.astype(np.int64))])

    @classmethod
    def from_arrays(cls, subpatterns, lo, hi, end_len):
        """subpatterns: list (per query) of lists of bytes; lo/hi: per query lists of k-1 start-to-start bounds."""
        self = cls.__new__(cls)
        blob, suboff, qsub, flo, fhi = [], [0], [0], [], []
        for subs, l, h in zip(subpatterns, lo, hi):
            for i, s in enumerate(subs):
                blob.append(bytes(s))
                suboff.append(suboff[-1] + len(s))
                flo.append(0 if i == 0 else int(l[i - 1]))
                fhi.append(0 if i == 0 else int(h[i - 1]))
            qsub.append(len(suboff) - 1)
        b = np.frombuffer(b"".join(blob) + b"\0", dtype=np.uint8)
        a = [np.asarray(x, dtype=np.uint64) for x in (suboff, qsub, flo + [0], fhi + [0], list(end_len) + [0])]
        hq = C.c_void_p()
        check(lib().vlg_queries_create(b.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                       a[4].ctypes.data, len(subpatterns), C.byref(hq)))
        self._h = hq
        self.n = len(subpatterns)
        self.status = np.zeros(self.n, dtype=np.int32)
        return self

    def set_windows(self, begin=None, end=None):
        """Text windows of the batch (vlg_queries_set_windows): VlgIndex.search answers query j on [begin[j], end[j]) -- its matches
        are those of the query on text[begin:end], shifted by begin.  A scalar for the whole batch or one value per query; None: from
        0 / to the end of the text; both None removes the windows."""
        b, e = _window_array(begin, self.n, "begin"), _window_array(end, self.n, "end")
        check(lib().vlg_queries_set_windows(self._h, b.ctypes.data if b is not None else None, e.ctypes.data if e is not None else None))

    def windows(self):
        """-> (begin[], end[]) as they were set (an end of 2^64 - 1: to the end of the text), or None for a batch without windows"""
        has = C.c_int(0)
        b, e = np.zeros(max(self.n, 1), np.uint64), np.zeros(max(self.n, 1), np.uint64)
        check(lib().vlg_queries_get_windows(self._h, C.byref(has), b.ctypes.data, e.ctypes.data))
        return (b[: self.n], e[: self.n]) if has.value else None

    def set_documents(self, documents):
        """Documents of the batch (vlg_queries_set_documents): VlgIndex.search then gives, for every document in turn, the matches
        the query has on that document alone -- no match crosses a boundary.  A Documents, or None to remove them.  The batch keeps
        the Documents alive."""
        if documents is not None and not isinstance(documents, Documents):
            raise TypeError("a Documents (or None) expected")
        check(lib().vlg_queries_set_documents(self._h, documents._h if documents is not None else None))
        self._documents = documents

    def documents(self):
        """-> the Documents the batch carries, or None"""
        h = C.c_void_p()
        check(lib().vlg_queries_get_documents(self._h, C.byref(h)))
        d = getattr(self, "_documents", None)
        return d if h.value and d is not None and d._h.value == h.value else None

    def set_mismatches(self, k):
        """Mismatch budgets of the batch (vlg_queries_set_mismatches): VlgIndex.search lets sub-pattern s differ from the text in up
        to k[s] of its positions (substitutions only).  A scalar for every sub-pattern or one value (0 .. 255) per sub-pattern of the
        batch, in batch order (subpattern_range); None or all zeros removes the budgets."""
        nsub = int(lib().vlg_queries_subpatterns(self._h))
        if k is None:
            check(lib().vlg_queries_set_mismatches(self._h, None))
            return
        a = np.asarray(k)
        if a.dtype.kind not in "iu":
            raise ValueError(f"mismatches: budgets are integers, got {a.dtype}")
        if a.ndim == 0:
            a = np.full(nsub, a)
        if a.shape != (nsub,):
            raise ValueError(f"mismatches: {nsub} sub-patterns, got an array of shape {a.shape}")
        if len(a) and (a.min() < 0 or a.max() > 255):
            raise ValueError("mismatches: a budget is 0 .. 255")
        a = np.ascontiguousarray(np.concatenate([a, [0]]), dtype=np.uint8)
        check(lib().vlg_queries_set_mismatches(self._h, a.ctypes.data))

    def mismatches(self):
        """-> the budgets per sub-pattern as they were set, or None for a batch without budgets"""
        has = C.c_int(0)
        nsub = int(lib().vlg_queries_subpatterns(self._h))
        k = np.zeros(max(nsub, 1), np.uint8)
        check(lib().vlg_queries_get_mismatches(self._h, C.byref(has), k.ctypes.data))
        return k[:nsub] if has.value else None

    @property
    def ks(self):
        """sub-patterns per query (0 for a query that failed to parse)"""
        if getattr(self, "_ks", None) is None:
            k = np.zeros(max(self.n, 1), dtype=np.uint32)
            check(lib().vlg_queries_k(self._h, k.ctypes.data))
            self._ks = k[: self.n]
        return self._ks

    def __del__(self):
        try:
            if self._h:
                lib().vlg_queries_destroy(self._h)
                self._h = None
        except Exception:
            pass


class VlgIndex:
    """FM-index (csa_wt<wt_huff<>>-equivalent) resident in HBM."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep          # e.g. the torch tensor backing an attached blob
        self._ws = None

    # -- construction ---------------------------------------------------------------------------
    @classmethod
    def build(cls, text, dens=32):
        """sdsl::construct equivalent, on the device (suffix sort, BWT, wavelet tree, sampling)."""
        t = _u8(text)
        h = C.c_void_p()
        check(lib().vlg_index_build(t.ctypes.data if len(t) else None, len(t), dens, C.byref(h)))
        return cls(h)

    @classmethod
    def build_int(cls, text, dens=32):
        """FM-index of an integer text (csa_wt<wt_int<>, dens, ..., int_alphabet<>>): symbols uint32, none of them 0."""
        t = np.ascontiguousarray(text, dtype=np.uint32)
        h = C.c_void_p()
        check(lib().vlg_index_build_int(t.ctypes.data if len(t) else None, len(t), dens, C.byref(h)))
        return cls(h)

    def int_alphabet(self):
        """(C[sigma + 1], comp2char[sigma]) of an integer-alphabet index"""
        sg = C.c_uint64()
        check(lib().vlg_index_export_int_alphabet(self._h, C.byref(sg), None, None))
        Cc, c2c = np.zeros(sg.value + 1, np.uint64), np.zeros(max(sg.value, 1), np.uint64)
        check(lib().vlg_index_export_int_alphabet(self._h, C.byref(sg), Cc.ctypes.data, c2c.ctypes.data))
        return Cc, c2c[: sg.value]

    @classmethod
    def build_device(cls, d_text_ptr, n_text, dens=32, stream=None):
        h = C.c_void_p()
        check(lib().vlg_index_build_device(d_text_ptr, n_text, dens, stream, C.byref(h)))
        return cls(h)

    @classmethod
    def from_parts(cls, p):
        """Adopt an index in the reference's own layout (dict as produced by export_parts())."""
        nodes = np.ascontiguousarray(p["nodes"])
        c2c = np.ascontiguousarray(p["char2comp"], dtype=np.uint8)
        Cc = np.ascontiguousarray(p["C"], dtype=np.uint64)
        bv = np.ascontiguousarray(p["bv_words"], dtype=np.uint64)
        smp = np.ascontiguousarray(p["samples"], dtype=np.uint64)
        parts = capi.IndexParts(int(p["n"]), int(p["sigma"]), int(p.get("dens", 32)), c2c.ctypes.data, Cc.ctypes.data,
                                bv.ctypes.data if len(bv) else None, int(p["bv_bits"]), nodes.ctypes.data, len(nodes),
                                smp.ctypes.data, len(smp))
        h = C.c_void_p()
        check(lib().vlg_index_from_parts(C.byref(parts), C.byref(h)))
        return cls(h)

    @classmethod
    def load_sdsl(cls, path, dens=32, rrr=False):
        """An index stored by stock sdsl: a csa_wt<wt_huff<>> file, or (rrr) a csa_wt<wt_huff<rrr_vector<63>>> file."""
        h = C.c_void_p()
        check(lib().vlg_index_load_sdsl_kind(str(path).encode(), dens, 1 if rrr else 0, C.byref(h)))
        return cls(h)

    @classmethod
    def load_sdsl_int(cls, path, dens=32, rrr=False):
        """An integer index stored by stock sdsl: a csa_wt<wt_int<>, dens, ., ., ., int_alphabet<>> file, or (rrr) one over
        wt_int<rrr_vector<63>>; the level-wise tree is converted to this library's wavelet matrix on the device."""
        h = C.c_void_p()
        check(lib().vlg_index_load_sdsl_int(str(path).encode(), dens, 1 if rrr else 0, C.byref(h)))
        return cls(h)

    @classmethod
    def from_int_parts(cls, p):
        """An integer index from the members of a csa_wt<wt_int<>> file (dict as read_sdsl_int_file returns it)."""
        c2c = np.ascontiguousarray(p["comp2char"], dtype=np.uint64)
        Cc = np.ascontiguousarray(p["C"], dtype=np.uint64)
        tw = np.ascontiguousarray(p["tree_words"], dtype=np.uint64)
        smp = np.ascontiguousarray(p["samples"], dtype=np.uint64)
        parts = capi.IntIndexParts(int(p["n"]), int(p["sigma"]), int(p["max_level"]), int(p.get("dens", 32)), c2c.ctypes.data, Cc.ctypes.data,
                                   tw.ctypes.data if len(tw) else None, int(p["tree_bits"]), smp.ctypes.data if len(smp) else None, len(smp))
        h = C.c_void_p()
        check(lib().vlg_index_from_int_parts(C.byref(parts), C.byref(h)))
        return cls(h)

    def save_sdsl(self, path, isa_dens=64):
        """Store in the reference's on-disk format (stock sdsl can load_from_file it): csa_wt<wt_huff<>,32,64> for a byte index,
        csa_wt<wt_int<>, dens, isa_dens, ., ., int_alphabet<>> for an integer one (plain or rrr, SA order, any dens)."""
        if self.info()["bv_kind"] in (2, 3):
            check(lib().vlg_index_save_sdsl_int(self._h, str(path).encode(), int(isa_dens)))
        else:
            if isa_dens != 64:
                raise ValueError("a byte index is stored as csa_wt<wt_huff<>,32,64>: its ISA density is 64")
            check(lib().vlg_index_save_sdsl(self._h, str(path).encode()))

    def int_tree(self):
        """wt_int::tree of an integer index, converted on the device -> (max_level, uint64 words of n * max_level bits)"""
        L = C.c_uint32()
        check(lib().vlg_index_export_int_tree(self._h, C.byref(L), None))
        n = self.info()["n"]
        w = np.zeros((n * L.value + 63) // 64 + 1, np.uint64)
        check(lib().vlg_index_export_int_tree(self._h, C.byref(L), w.ctypes.data))
        return int(L.value), w[: (n * L.value + 63) // 64]

    def isa_samples(self, inv_dens=64):
        """isa_sample of csa_wt: out[j] = SA index of text position j * inv_dens.  Byte or integer alphabet, plain or rrr; the index
        must be SA-order sampled (a text-order one raises VLG_E_UNSUPPORTED)."""
        n = self.info()["n"]
        out = np.zeros((n - 1) // inv_dens + 1, dtype=np.uint64)
        check(lib().vlg_index_isa_samples(self._h, inv_dens, out.ctypes.data, len(out)))
        return out

    def text_access(self, inv_dens=64, stream=None):
        """A TextAccess over this index: extract(csa, b, e), csa.text[i] and csa.isa[i] from ISA samples of density inv_dens kept in
        HBM.  SA-order indexes only (a text-order one raises VLG_E_UNSUPPORTED)."""
        return TextAccess(self, inv_dens, stream)

    def select_support(self, sample=0, stream=None):
        """A SelectSupport over the BWT of this index: wt.select(k, c) and csa.psi[i] from select hints `sample` ones / zeros apart per
        wavelet-tree node or matrix level (0 = the default, 512; otherwise a power of two in [64, 65536]).  Any kind of index."""
        return SelectSupport(self, sample, stream)

    def lf_device(self, d_i_ptr, d_out_ptr, count, stream=None):
        """vlg_lf_batch on device pointers"""
        check(lib().vlg_lf_batch(self._h, d_i_ptr, d_out_ptr, int(count), stream))

    def bwt_device(self, d_i_ptr, d_out_ptr, count, stream=None):
        """vlg_bwt_batch on device pointers (uint8 out for a byte index, uint32 for an integer one)"""
        check(lib().vlg_bwt_batch(self._h, d_i_ptr, d_out_ptr, int(count), stream))

    def lf(self, i):
        """csa.lf[i] for a scalar (-> int) or an array (-> np.uint64 array); an i >= n gives 2^64 - 1"""
        return _u64_batch(i, "i", lambda d_i, d_o, count: self.lf_device(d_i, d_o, count))

    def bwt(self, i):
        """csa.bwt[i] for a scalar (-> int) or an array (-> np.uint8 / np.uint32 array of original symbols); the sentinel and an
        i >= n give 0"""
        import torch
        scalar = np.ndim(i) == 0
        p = _u64_index_array(i, "i")
        is_int = self.info()["bv_kind"] in (2, 3)
        if not len(p):
            return np.zeros(0, np.uint32 if is_int else np.uint8)
        d_i = torch.from_numpy(p.view(np.int64)).cuda()
        d_o = torch.empty(len(p), dtype=torch.int32 if is_int else torch.uint8, device="cuda")
        self.bwt_device(d_i.data_ptr(), d_o.data_ptr(), len(p))
        out = d_o.cpu().numpy()
        out = out.view(np.uint32) if is_int else out
        return int(out[0]) if scalar else out

    @classmethod
    def attach_blob(cls, d_ptr, nbytes, keep=None):
        h = C.c_void_p()
        check(lib().vlg_index_attach_blob(d_ptr, nbytes, C.byref(h)))
        return cls(h, keep)

    def __del__(self):
        try:
            if self._h:
                lib().vlg_index_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- introspection ----------------------------------------------------------------------------
    def info(self):
        i = capi.IndexInfo()
        check(lib().vlg_index_get_info(self._h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in capi.IndexInfo._fields_}

    def quad_image(self):
        """The quad image beside the blob (vlg_index_quad_image): {"bytes", "n_nodes", "build_s"}; all zero where the index has none"""
        b, nn, s = C.c_uint64(0), C.c_uint32(0), C.c_double(0)
        check(lib().vlg_index_quad_image(self._h, C.byref(b), C.byref(nn), C.byref(s)))
        return {"bytes": int(b.value), "n_nodes": int(nn.value), "build_s": float(s.value)}

    def quad_lf_device(self, d_i_ptr, d_lf_ptr, d_comp_ptr, d_levels_ptr, count):
        """vlg_quad_lf_batch on device pointers (uint64 LF, uint8 compact symbols, uint32 levels; any output may be None); synchronous"""
        check(lib().vlg_quad_lf_batch(self._h, d_i_ptr, d_lf_ptr, d_comp_ptr, d_levels_ptr, int(count)))

    def compress(self, bv_kind=1):
        """A csa_wt<wt_huff<rrr_vector<63>>>-equivalent of this (plain) index (wt_int<rrr_vector<63>> for an integer index); same answers, compressed bit-vectors."""
        h = C.c_void_p()
        check(lib().vlg_index_compress(self._h, bv_kind, C.byref(h)))
        return VlgIndex(h)

    def resample(self, text_order=True, dens=32):
        """A second index over the same BWT with text_order_sa_sampling (or SA-order sampling of another density; dens=1 keeps the suffix
        array resident); same answers.  Byte or integer alphabet, plain or rrr; this index must be SA-order sampled (VLG_E_INVALID)."""
        h = C.c_void_p()
        check(lib().vlg_index_resample(self._h, 1 if text_order else 0, int(dens), C.byref(h)))
        return VlgIndex(h)

    def marked(self):
        """text-order sampling: the marks over the SA indices -> uint8 array of n zeros / ones (byte or integer alphabet; an SA-order
        index raises VLG_E_INVALID)"""
        n = self.info()["n"]
        w = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(lib().vlg_index_export_marked(self._h, w.ctypes.data))
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:n]

    def export_parts(self):
        sz = capi.IndexParts()
        check(lib().vlg_index_export_parts(self._h, C.byref(sz), None))
        c2c = np.zeros(256, np.uint8)
        Cc = np.zeros(257, np.uint64)
        bv = np.zeros(max((sz.bv_bits + 63) // 64, 1), np.uint64)
        nodes = np.zeros(max(sz.n_nodes, 1), dtype=NODE_DTYPE)
        smp = np.zeros(max(sz.n_samples, 1), np.uint64)
        out = capi.IndexPartsOut(c2c.ctypes.data, Cc.ctypes.data, bv.ctypes.data, nodes.ctypes.data, smp.ctypes.data)
        check(lib().vlg_index_export_parts(self._h, C.byref(sz), C.byref(out)))
        return {"n": int(sz.n), "sigma": int(sz.sigma), "dens": int(sz.sa_sample_dens), "char2comp": c2c,
                "C": Cc[: sz.sigma + 1], "bv_bits": int(sz.bv_bits), "bv_words": bv[: (sz.bv_bits + 63) // 64],
                "nodes": nodes[: sz.n_nodes], "samples": smp[: sz.n_samples]}

    def blob_bytes(self):
        b = C.c_uint64()
        check(lib().vlg_index_blob_bytes(self._h, C.byref(b)))
        return int(b.value)

    def blob_export(self, d_ptr, nbytes, stream=None):
        check(lib().vlg_index_blob_export(self._h, d_ptr, nbytes, stream))

    # -- search -----------------------------------------------------------------------------------
    def _queries(self, queries, dialect=capi.DIALECT_LIBRARY, strict=True):
        if isinstance(queries, Queries):
            return queries
        if self.info()["bv_kind"] in (2, 3):                       # integer-alphabet index: the integer query dialect
            return Queries.from_int(queries, strict)
        return Queries(queries, dialect, strict)

    def occurrences(self, queries, dialect=capi.DIALECT_LIBRARY):
        """sdsl::count of every sub-pattern of the batch (one backward-search pass) -> uint64[n sub-patterns]"""
        q = self._queries(queries, dialect)
        nsub = int(lib().vlg_queries_subpatterns(q._h))
        occ = np.zeros(max(nsub, 1), dtype=np.uint64)
        check(lib().vlg_queries_occurrences(self._h, q._h, occ.ctypes.data, None))
        return occ[:nsub], q

    def intervals(self, queries, dialect=capi.DIALECT_LIBRARY):
        """SA interval [l, r] of every sub-pattern of the batch (one backward-search pass) -> (l[], r[], Queries)"""
        q = self._queries(queries, dialect)
        nsub = int(lib().vlg_queries_subpatterns(q._h))
        l, r = np.zeros(max(nsub, 1), dtype=np.uint64), np.zeros(max(nsub, 1), dtype=np.uint64)
        check(lib().vlg_queries_intervals(self._h, q._h, l.ctypes.data, r.ctypes.data, None))
        return l[:nsub], r[:nsub], q

    def query_weights(self, queries, dialect=capi.DIALECT_LIBRARY):
        """Estimated work per query = sum of the SA-interval sizes of its sub-patterns (0 when one of them does not occur: such a
        query locates nothing) -- what vlg_matching_amd.dist.shard_by_work balances."""
        occ, q = self.occurrences(queries, dialect)
        qsub = q.subpattern_range()
        w = np.zeros(q.n, dtype=np.float64)
        if len(occ):
            cs = np.concatenate([[0], np.cumsum(occ.astype(np.float64))])
            w = cs[qsub[1:]] - cs[qsub[:-1]]
            dead = np.zeros(q.n, dtype=bool)
            zero = np.concatenate([[0], np.cumsum(occ == 0)])
            dead = (zero[qsub[1:]] - zero[qsub[:-1]]) > 0
            w[dead] = 0.0
        return w + 1.0                                         # every query costs something (parse, plan)

    def workspace(self, max_hbm_bytes=0):
        if self._ws is None:
            self._ws = Workspace(max_hbm_bytes)
        return self._ws

    def search(self, queries, dialect=capi.DIALECT_LIBRARY, workspace=None, strict=True, begin=None, end=None):
        """Batched `idx.search(pat)`: queries is a list of regexps or a Queries object.  begin / end: text windows for this call
        (Queries.set_windows); the batch carries afterwards what it carried before."""
        q = self._queries(queries, dialect, strict)
        ws = workspace or self.workspace()
        h = C.c_void_p()
        if begin is None and end is None:
            check(lib().vlg_search_batch(self._h, q._h, ws._h, C.byref(h)))
            return SearchResult(h, q.ks)
        before = q.windows()
        q.set_windows(begin, end)
        try:
            check(lib().vlg_search_batch(self._h, q._h, ws._h, C.byref(h)))
        finally:
            q.set_windows(*(before or (None, None)))
        return SearchResult(h, q.ks)


def _u64_index_array(a, name):
    """a host array / scalar of non-negative integers as uint64 (negative values and non-integers raise ValueError)"""
    arr = np.asarray(a)
    if arr.size == 0:
        return np.zeros(0, np.uint64)
    if arr.dtype.kind not in "iu":
        raise ValueError("%s: integer values expected, got %s" % (name, arr.dtype))
    if arr.dtype.kind == "i" and arr.size and int(arr.min()) < 0:
        raise ValueError("%s: negative value" % name)
    return np.ascontiguousarray(arr.reshape(-1), dtype=np.uint64)


def _window_array(v, nq, name):
    """begin / end of a windowed search: None, a scalar for every query, or one value per query -> uint64 array or None"""
    if v is None:
        return None
    if np.ndim(v) == 0:
        a = np.full(nq, int(v), dtype=np.uint64)
    elif isinstance(v, np.ndarray):
        a = _u64_index_array(v, name)
    else:
        a = np.array([int(x) for x in v], dtype=np.uint64)
    if len(a) != nq:
        raise ValueError("%s: one value per query expected (%d), got %d" % (name, nq, len(a)))
    return a


class TextAccess:
    """The text of an SA-order index given back on the device (vlg_text_access): extract = sdsl::extract(csa, begin, end)
    (inclusive end), isa = csa.isa[i].  Byte indexes give bytes, integer indexes np.uint32 arrays of the original symbols.  Position
    n - 1 (n = |text| + 1) is the sentinel and reads as 0."""

    def __init__(self, index, inv_dens=64, stream=None):
        inv_dens = int(inv_dens)
        if inv_dens < 1 or inv_dens >= 1 << 32:
            raise ValueError("inv_dens must be in [1, 2^32)")
        self.index = index                        # the handle refers to the index: keep it alive
        info = index.info()
        self.n = info["n"]
        self.is_int = info["bv_kind"] in (2, 3)
        self.inv_dens = inv_dens
        self._h = None
        h = C.c_void_p()
        check(lib().vlg_text_access_create(index._h, inv_dens, stream, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().vlg_text_access_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def symbol_dtype(self):
        return np.uint32 if self.is_int else np.uint8

    def extract_device(self, d_begin_ptr, d_end_ptr, d_out_off_ptr, n_ranges, total, d_out_ptr, stream=None):
        """vlg_extract_batch on device pointers"""
        check(lib().vlg_extract_batch(self._h, d_begin_ptr, d_end_ptr, d_out_off_ptr, int(n_ranges), int(total), d_out_ptr, stream))

    def isa_device(self, d_i_ptr, d_out_ptr, count, stream=None):
        """vlg_isa_batch on device pointers"""
        check(lib().vlg_isa_batch(self._h, d_i_ptr, d_out_ptr, int(count), stream))

    def extract_batch(self, begins, ends):
        """T[begins[r] .. ends[r]] for every r -> (concatenated symbols, offsets[n_ranges + 1]).  Host arrays give a numpy array (uint8
        or uint32) and numpy offsets; device tensors (torch, int64 / uint64) give a device tensor (uint8 or int32 holding the uint32
        symbols) and device offsets."""
        import torch
        if isinstance(begins, torch.Tensor) or isinstance(ends, torch.Tensor):
            return self._extract_batch_device(begins, ends)
        b, e = _u64_index_array(begins, "begins"), _u64_index_array(ends, "ends")
        if len(b) != len(e):
            raise ValueError("begins and ends differ in length")
        if len(b) and ((b > e).any() or int(e.max()) >= self.n):
            raise ValueError("every range needs begin <= end < n (n = %d)" % self.n)
        off = np.zeros(len(b) + 1, dtype=np.uint64)
        np.cumsum(e - b + 1, out=off[1:])
        total = int(off[-1])
        if not len(b):
            return np.zeros(0, self.symbol_dtype), off
        d_b = torch.from_numpy(b.view(np.int64)).cuda()
        d_e = torch.from_numpy(e.view(np.int64)).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        d_out = torch.empty(max(total, 1), dtype=torch.int32 if self.is_int else torch.uint8, device="cuda")
        self.extract_device(d_b.data_ptr(), d_e.data_ptr(), d_off.data_ptr(), len(b), total, d_out.data_ptr())
        out = d_out[:total].cpu().numpy()
        return (out.view(np.uint32) if self.is_int else out), off

    def _extract_batch_device(self, begins, ends):
        import torch
        for name, t in (("begins", begins), ("ends", ends)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or t.dim() != 1:
                raise ValueError("%s: a 1-d int64 / uint64 device tensor expected" % name)
        if begins.numel() != ends.numel():
            raise ValueError("begins and ends differ in length")
        b, e = begins.contiguous().to(torch.int64), ends.contiguous().to(torch.int64)
        off = torch.zeros(b.numel() + 1, dtype=torch.int64, device=b.device)
        torch.cumsum(e - b + 1, 0, out=off[1:])
        total = int(off[-1].item()) if b.numel() else 0
        d_out = torch.empty(max(total, 1), dtype=torch.int32 if self.is_int else torch.uint8, device=b.device)
        if total < 0:
            raise ValueError("every range needs begin <= end < n (n = %d)" % self.n)
        if b.numel():                                 # (a bad range among them: the device check refuses the batch, VLG_E_INVALID)
            self.extract_device(b.data_ptr(), e.data_ptr(), off.data_ptr(), b.numel(), total, d_out.data_ptr())
        return d_out[:total], off

    def extract(self, begin, end):
        """sdsl::extract(csa, begin, end): T[begin .. end] (inclusive) -> bytes (byte index) or np.uint32 array (integer index)"""
        begin, end = int(begin), int(end)
        if begin < 0 or begin > end or end >= self.n:
            raise ValueError("extract needs 0 <= begin <= end < n (n = %d)" % self.n)
        out, _ = self.extract_batch(np.array([begin], np.uint64), np.array([end], np.uint64))
        return out if self.is_int else out.tobytes()

    def text(self, i):
        """csa.text[i]"""
        r = self.extract(i, i)
        return int(r[0])

    def isa(self, i):
        """csa.isa[i] for a scalar (-> int) or an array (-> np.uint64 array) of positions < n"""
        import torch
        scalar = np.ndim(i) == 0
        p = _u64_index_array(i, "i")
        if len(p) and int(p.max()) >= self.n:
            raise ValueError("isa needs positions < n (n = %d)" % self.n)
        if not len(p):
            return np.zeros(0, np.uint64)
        d_i = torch.from_numpy(p.view(np.int64)).cuda()
        d_o = torch.empty_like(d_i)
        self.isa_device(d_i.data_ptr(), d_o.data_ptr(), len(p))
        out = d_o.cpu().numpy().view(np.uint64)
        return int(out[0]) if scalar else out


def _u64_batch(a, name, run, *more):
    """run(d_in_ptr, d_out_ptr, count, *device pointers of `more`) on a host scalar / array of uint64 -> int / np.uint64 array"""
    import torch
    scalar = np.ndim(a) == 0
    p = _u64_index_array(a, name)
    if not len(p):
        return np.zeros(0, np.uint64)
    d_i = torch.from_numpy(p.view(np.int64)).cuda()
    d_o = torch.empty_like(d_i)
    d_more = [torch.from_numpy(x).cuda() for x in more]
    run(d_i.data_ptr(), d_o.data_ptr(), len(p), *[x.data_ptr() for x in d_more])
    out = d_o.cpu().numpy().view(np.uint64)
    return int(out[0]) if scalar else out


class Documents:
    """The documents a text is made of (vlg_documents): their starts in HBM beside the index.  Queries.set_documents(d) makes a search
    document-bounded; locate turns positions into (document, offset)."""

    def __init__(self, starts, n_text):
        self._h = None
        s = np.asarray(starts)
        if s.ndim != 1 or (len(s) and s.dtype.kind not in "iu"):
            raise ValueError("starts: a 1-d array of non-negative integers")
        if len(s) and s.dtype.kind == "i" and int(s.min()) < 0:
            raise ValueError("starts: a start is negative")
        s = np.ascontiguousarray(s, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vlg_documents_create(s.ctypes.data if len(s) else None, len(s), int(n_text), C.byref(h)))
        self._h = h
        self.n_text = int(n_text)

    @classmethod
    def from_starts(cls, starts, n_text):
        """starts[0] = 0 < starts[1] < ... < n_text: document j is [starts[j], starts[j + 1]), the last one ends at n_text"""
        return cls(starts, n_text)

    @classmethod
    def from_separator(cls, text, sep):
        """One document per `sep`-terminated piece of `text` (bytes or an integer array; sep a byte or a symbol): a document starts at 0
        and behind every separator, so the separator closes its document."""
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.asarray(text)
        if isinstance(sep, (bytes, bytearray)):
            if len(sep) != 1:
                raise ValueError("sep: one byte")
            sep = sep[0]
        after = np.flatnonzero(a == sep).astype(np.uint64) + 1
        starts = np.concatenate([np.zeros(1, np.uint64), after[after < len(a)]])
        return cls(starts, len(a))

    def __del__(self):
        try:
            if self._h:
                lib().vlg_documents_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def count(self):
        return int(lib().vlg_documents_count(self._h))

    def locate_device(self, d_pos_ptr, count, d_doc_ptr, d_offset_ptr):
        """vlg_documents_locate_batch on device pointers (either output may be None); returns when the results are there"""
        check(lib().vlg_documents_locate_batch(self._h, d_pos_ptr, int(count), d_doc_ptr, d_offset_ptr))

    def locate(self, positions):
        """-> (document, offset) of a position (ints) or of an array of positions (np.uint64 arrays); a position >= n_text gives
        2^64 - 1 twice"""
        import torch
        scalar = np.ndim(positions) == 0
        p = _u64_index_array(positions, "positions")
        if not len(p):
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        d_p = torch.from_numpy(p.view(np.int64)).cuda()
        d_d, d_o = torch.empty_like(d_p), torch.empty_like(d_p)
        self.locate_device(d_p.data_ptr(), len(p), d_d.data_ptr(), d_o.data_ptr())
        doc, off = d_d.cpu().numpy().view(np.uint64), d_o.cpu().numpy().view(np.uint64)
        return (int(doc[0]), int(off[0])) if scalar else (doc, off)


class SelectSupport:
    """Select hints in HBM beside a bit-vector or an index (vlg_select_support).  From a BitVector / RrrBitVector: bit_select =
    select_support_mcl<bit>::select / select_support_rrr<bit>::select.  From a VlgIndex: select = wt.select(k, c) on the BWT (c: a text
    byte, or an original symbol of an integer index), psi = csa.psi[i].  k counts from 1; k = 0, a k past the last occurrence or an
    absent symbol give the size of the sequence (nbits, or n)."""

    def __init__(self, source, sample=0, stream=None):
        sample = int(sample)
        if sample < 0 or sample >= 1 << 32:
            raise ValueError("sample must be in [0, 2^32)")
        self.source = source                      # the handle refers to its source: keep it alive
        self.is_index = isinstance(source, VlgIndex)
        self.is_int = self.is_index and source.info()["bv_kind"] in (2, 3)
        self._h = None
        h = C.c_void_p()
        if self.is_index:
            check(lib().vlg_index_select_create(source._h, sample, stream, C.byref(h)))
        elif isinstance(source, RrrBitVector):
            check(lib().vlg_rrr_bitvector_select_create(source._h, sample, stream, C.byref(h)))
        elif isinstance(source, BitVector):
            check(lib().vlg_bitvector_select_create(source._h, sample, stream, C.byref(h)))
        else:
            raise TypeError("a VlgIndex, BitVector or RrrBitVector expected")
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().vlg_select_support_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def hbm_bytes(self):
        return int(lib().vlg_select_support_hbm_bytes(self._h))

    def bit_select_device(self, d_k_ptr, d_out_ptr, count, bit=1, stream=None):
        """vlg_bit_select_batch on device pointers"""
        check(lib().vlg_bit_select_batch(self._h, int(bit), d_k_ptr, d_out_ptr, int(count), stream))

    def select_device(self, d_k_ptr, d_c_ptr, d_out_ptr, count, stream=None):
        """vlg_wt_select_batch (byte index: uint8 symbols) / vlg_int_select_batch (integer index: uint32 symbols) on device pointers"""
        f = lib().vlg_int_select_batch if self.is_int else lib().vlg_wt_select_batch
        check(f(self._h, d_k_ptr, d_c_ptr, d_out_ptr, int(count), stream))

    def psi_device(self, d_i_ptr, d_out_ptr, count, stream=None):
        """vlg_psi_batch on device pointers"""
        check(lib().vlg_psi_batch(self._h, d_i_ptr, d_out_ptr, int(count), stream))

    def bit_select(self, k, bit=1):
        """position of the k-th `bit` for a scalar (-> int) or an array (-> np.uint64 array) of k"""
        if bit not in (0, 1):
            raise ValueError("bit must be 0 or 1")
        return _u64_batch(k, "k", lambda d_k, d_o, count: self.bit_select_device(d_k, d_o, count, bit))

    def select(self, k, c):
        """wt.select(k, c): SA index of the k-th c in the BWT; scalars (-> int) or arrays of equal length (-> np.uint64 array)"""
        ka = _u64_index_array(k, "k")
        ca = _u64_index_array(c, "c")
        if len(ka) != len(ca):
            raise ValueError("k and c differ in length")
        if len(ca) and int(ca.max()) > (0xFFFFFFFF if self.is_int else 0xFF):
            raise ValueError("c: symbol out of range")
        sym = np.ascontiguousarray(ca.astype(np.uint32).view(np.int32) if self.is_int else ca.astype(np.uint8))
        out = _u64_batch(ka, "k", lambda d_k, d_o, count, d_c: self.select_device(d_k, d_c, d_o, count), sym)
        return int(out[0]) if np.ndim(k) == 0 and np.ndim(c) == 0 else out

    def psi(self, i):
        """csa.psi[i] for a scalar (-> int) or an array (-> np.uint64 array); an i >= n gives 2^64 - 1"""
        return _u64_batch(i, "i", lambda d_i, d_o, count: self.psi_device(d_i, d_o, count))


class WtsaIndex:
    """sdsl::vlg_index<alphabet_tag, wt_int<>> in HBM: the text + a wavelet tree over its suffix array, searched lazily
    (include/sdsl/vlg_index.hpp:109-373).  `text`: bytes / uint8 array (byte alphabet) or a uint32 array (integer alphabet)."""

    def __init__(self, text):
        if isinstance(text, np.ndarray) and text.dtype != np.uint8:
            t = np.ascontiguousarray(text, dtype=np.uint32)
            self.symbol_bytes = 4
        else:
            t = _u8(text)
            self.symbol_bytes = 1
        h = C.c_void_p()
        check(lib().vlg_wtsa_build(t.ctypes.data if len(t) else None, len(t), self.symbol_bytes, C.byref(h)))
        self._h = h
        self._ws = None

    @classmethod
    def _adopt(cls, h):
        self = cls.__new__(cls)
        self._h, self._ws = h, None
        self.symbol_bytes = self.info()["symbol_bytes"]
        return self

    @classmethod
    def load_sdsl(cls, path, int_alphabet=False):
        """An index stored by stock sdsl: `store_to_file(idx, file)` of vlg_index<byte_alphabet_tag> (int_alphabet:
        vlg_index<int_alphabet_tag>) with the default tree wt_int<bit_vector_il<>, rank_support_il<>>."""
        h = C.c_void_p()
        check(lib().vlg_wtsa_load_sdsl(str(path).encode(), 4 if int_alphabet else 1, C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def from_parts(cls, p):
        """An index from the members of such a file (dict as read_sdsl_wtsa_file returns it), converted and checked on the device."""
        tw = np.ascontiguousarray(p["text_words"], dtype=np.uint64)
        data = np.ascontiguousarray(p["data"], dtype=np.uint64)
        rs = np.ascontiguousarray(p["rank_samples"], dtype=np.uint64)
        parts = capi.WtsaParts(int(p["n"]), int(p["symbol_bytes"]), int(p["levels"]), tw.ctypes.data if len(tw) else None,
                               int(p["text_count"]), int(p["text_width"]), 0, data.ctypes.data if len(data) else None, len(data),
                               rs.ctypes.data if len(rs) else None, len(rs))
        h = C.c_void_p()
        check(lib().vlg_wtsa_from_parts(C.byref(parts), C.byref(h)))
        return cls._adopt(h)

    def save_sdsl(self, path, text_width=0):
        """Store as stock sdsl's vlg_index<alphabet_tag> file.  text_width: the width of m_text -- 0 or 8 for a byte index; for an
        integer index 0 (the width of the file it was loaded from, or that of its largest symbol) or 1..64."""
        check(lib().vlg_wtsa_save_sdsl(self._h, str(path).encode(), int(text_width)))

    def il_device(self, d_words_ptr, n_words, stream=None):
        """bit_vector_il<512>::m_data of the tree into device memory (block_num words)"""
        check(lib().vlg_wtsa_il_device(self._h, d_words_ptr, int(n_words), stream))

    def __del__(self):
        try:
            if self._h:
                lib().vlg_wtsa_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def info(self):
        i = capi.WtsaInfo()
        check(lib().vlg_wtsa_get_info(self._h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in capi.WtsaInfo._fields_}

    def queries(self, regexps):
        """a parsed batch for this index's alphabet (integer alphabet: sub-patterns are whitespace-separated decimals)"""
        if isinstance(regexps, Queries):
            return regexps
        if self.symbol_bytes == 1:
            return Queries(regexps)
        raws = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in regexps]
        off = np.zeros(len(raws) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in raws])
        q = Queries.__new__(Queries)
        h = C.c_void_p()
        check(lib().vlg_queries_parse_int(b"".join(raws), off.ctypes.data, len(raws), None, C.byref(h)))
        q._h, q.n, q.status = h, len(raws), np.zeros(len(raws), dtype=np.int32)
        return q

    def sa_device(self, d_idx_ptr, d_out_ptr, count, stream=None):
        check(lib().vlg_wtsa_sa_batch(self._h, d_idx_ptr, d_out_ptr, count, stream))

    def range_walk_device(self, d_l_ptr, d_len_ptr, d_x_ptr, quantile, d_out_ptr, count, stream=None):
        """count_less (quantile False) / quantile (True) on suffix-array ranges, device pointers"""
        check(lib().vlg_wtsa_range_walk_batch(self._h, d_l_ptr, d_len_ptr, d_x_ptr, 1 if quantile else 0, d_out_ptr, count, stream))

    def level_bits(self, level):
        """bits of one level of the tree -> uint8 array of n zeros / ones (wt_int::tree[level * n : (level + 1) * n])"""
        n = self.info()["n"]
        w = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(lib().vlg_wtsa_export_level(self._h, int(level), w.ctypes.data))
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:n]

    def ranges(self, queries):
        """forward_search of every sub-pattern -> (sp[], ep[]) suffix-array ranges (sp = ep + 1: no occurrence)"""
        q = self.queries(queries)
        nsub = int(lib().vlg_queries_subpatterns(q._h))
        sp, ep = np.zeros(max(nsub, 1), np.uint64), np.zeros(max(nsub, 1), np.uint64)
        check(lib().vlg_wtsa_ranges(self._h, q._h, sp.ctypes.data, ep.ctypes.data, None))
        return sp[:nsub], ep[:nsub]

    def search(self, queries, max_matches=0, workspace=None, begin=None, end=None):
        """sdsl::locate(idx, query) for a batch, lazily: at most max_matches matches per query (0 = all).  begin / end: the text window
        [begin, end) every query is answered on (a scalar for the whole batch or one value per query; None: from 0 / to the end of
        the text) -- its matches are those of the query on text[begin:end], shifted by begin."""
        q = self.queries(queries)
        if workspace is None:
            if self._ws is None:
                self._ws = Workspace()
            workspace = self._ws
        b, e = _window_array(begin, q.n, "begin"), _window_array(end, q.n, "end")
        h = C.c_void_p()
        check(lib().vlg_wtsa_search_window_batch(self._h, q._h, b.ctypes.data if b is not None and len(b) else None,
                                                 e.ctypes.data if e is not None and len(e) else None, int(max_matches), workspace._h, C.byref(h)))
        return SearchResult(h, q.ks)

    def pages(self, query, page=16, begin=0, end=None):
        """The matches of one query inside [begin, end), `page` at a time: a generator of tuple arrays [matches, k].  Every page is one
        capped search that begins where the one before stopped (SearchResult.next_positions) -- like the reference's iterator it
        continues (pull_forward, vlg_index.hpp:254-266) and never walks a prefix twice."""
        if int(page) < 1:
            raise ValueError("page must be at least 1")
        q = self.queries([query])
        at = int(begin)
        while at != NO_NEXT:
            r = self.search(q, max_matches=int(page), begin=at, end=end)
            t = r.tuples(0)
            if len(t):
                yield t
            at = int(r.next_positions()[0])

    def range_count_device(self, d_l_ptr, d_len_ptr, d_vlb_ptr, d_vrb_ptr, d_count_ptr, count, stream=None):
        """wt_int::range_search_2d's count: how many of SA[l, l + len) lie in [vlb, vrb], device pointers"""
        check(lib().vlg_wtsa_range_count_batch(self._h, d_l_ptr, d_len_ptr, d_vlb_ptr, d_vrb_ptr, d_count_ptr, count, stream))

    def range_report_device(self, d_l_ptr, d_len_ptr, d_vlb_ptr, d_vrb_ptr, d_out_off_ptr, count, total, d_out_ptr, stream=None):
        """those values, ascending, range j from d_out[d_out_off[j]] on (d_out_off: exclusive prefix sum of the counts, count + 1 entries)"""
        check(lib().vlg_wtsa_range_report_batch(self._h, d_l_ptr, d_len_ptr, d_vlb_ptr, d_vrb_ptr, d_out_off_ptr, count, total, d_out_ptr, stream))

    def range_report(self, l, length, vlb, vrb):
        """Host convenience over the pair: suffix-array ranges [l, l + length) and value windows [vlb, vrb] (arrays of equal length) ->
        (counts, offsets, values): range j's values, ascending, are values[offsets[j]:offsets[j + 1]].  A range outside the suffix
        array raises ValueError."""
        import torch
        a = [_u64_index_array(x, n) for x, n in ((l, "l"), (length, "length"), (vlb, "vlb"), (vrb, "vrb"))]
        m = len(a[0])
        if any(len(x) != m for x in a):
            raise ValueError("l, length, vlb and vrb must be equally long")
        if not m:
            return np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        d = [torch.from_numpy(x.view(np.int64)).cuda() for x in a]
        d_cnt = torch.empty_like(d[0])
        self.range_count_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_cnt.data_ptr(), m)
        counts = d_cnt.cpu().numpy().view(np.uint64)
        if (counts == np.uint64((1 << 64) - 1)).any():
            raise ValueError("a range lies outside the suffix array")
        off = np.zeros(m + 1, dtype=np.uint64)
        off[1:] = np.cumsum(counts)
        total = int(off[m])
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        d_out = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
        self.range_report_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_off.data_ptr(), m, total, d_out.data_ptr())
        return counts, off, d_out.cpu().numpy().view(np.uint64)[:total]

    def locate_window(self, pattern, begin=0, end=None):
        """The occurrences of one pattern (bytes; integer index: an array of symbols) that lie wholly inside the text window
        [begin, end), ascending: forward search, then the values of its suffix-array range inside [begin, end - |pattern|]."""
        n_text = self.info()["n"] - 1
        if self.symbol_bytes == 1:
            pat = bytes(pattern)
            q = Queries.from_arrays([[pat]], [[]], [[]], [1]) if len(pat) else None
        else:
            pat = np.asarray(pattern)
            q = self.queries([" ".join(str(int(x)) for x in pat)]) if len(pat) else None
        b, e = int(begin), n_text if end is None else min(int(end), n_text)
        if b < 0 or (end is not None and int(end) < b):
            raise ValueError("locate_window: 0 <= begin <= end expected")
        if q is None or e - b < len(pat):
            return np.zeros(0, np.uint64)
        sp, ep = self.ranges(q)
        return self.range_report([int(sp[0])], [int(ep[0]) + 1 - int(sp[0])], [b], [e - len(pat)])[2]


def join_batch(d_lists_ptr, list_off, join_list, lo, hi, end_len, workspace, ks=None):
    """vlg_join_batch: the gap-bounded merge join (index_sasearch.hpp:85-116) over caller-provided sorted u64 lists in HBM.
    list_off[n_lists+1], join_list[n_joins+1], lo/hi[n_lists], end_len[n_joins] are host arrays.  -> SearchResult"""
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (list_off, join_list, lo, hi, end_len)]
    n_lists, n_joins = len(a[0]) - 1, len(a[1]) - 1
    if len(a[2]) < max(n_lists, 1):
        a[2] = np.concatenate([a[2], np.zeros(max(n_lists, 1) - len(a[2]), np.uint64)])
    if len(a[3]) < max(n_lists, 1):
        a[3] = np.concatenate([a[3], np.zeros(max(n_lists, 1) - len(a[3]), np.uint64)])
    if len(a[4]) < max(n_joins, 1):
        a[4] = np.concatenate([a[4], np.ones(max(n_joins, 1) - len(a[4]), np.uint64)])
    h = C.c_void_p()
    check(lib().vlg_join_batch(d_lists_ptr, a[0].ctypes.data, n_lists, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                               a[4].ctypes.data, n_joins, workspace._h, C.byref(h)))
    return SearchResult(h, np.diff(a[1].astype(np.int64)).astype(np.uint32) if ks is None else ks)


def locate(idx, query):
    """sdsl::locate(idx, query): tuples [matches, k] of sub-pattern start positions (library dialect)."""
    r = idx.search([query])
    return r.tuples(0)


def count(idx, query):
    """sdsl::count(idx, query)."""
    return int(idx.search([query]).counts[0])


class BitVector:
    """rank_support_v-equivalent on a plain bit-vector, resident in HBM (K1)."""

    def __init__(self, words, nbits):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vlg_bitvector_create(w.ctypes.data if len(w) else None, int(nbits), C.byref(h)))
        self._h = h
        self.nbits = int(nbits)

    def __del__(self):
        try:
            if self._h:
                lib().vlg_bitvector_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def rank_device(self, d_idx_ptr, d_out_ptr, count, stream=None):
        check(lib().vlg_bitvector_rank_batch(self._h, d_idx_ptr, d_out_ptr, count, stream))

    def select_support(self, sample=0, stream=None):
        """select_support_mcl<1> and <0> over this bit-vector (SelectSupport.bit_select)"""
        return SelectSupport(self, sample, stream)

    def hbm_bytes(self):
        return int(lib().vlg_bitvector_hbm_bytes(self._h))


class RrrBitVector:
    """rrr_vector<63> + rank_support_rrr equivalent in HBM (K6): on-the-fly block decode, binomial table in LDS."""

    def __init__(self, words, nbits):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vlg_rrr_bitvector_create(w.ctypes.data if len(w) else None, int(nbits), C.byref(h)))
        self._h = h
        self.nbits = int(nbits)

    def __del__(self):
        try:
            if self._h:
                lib().vlg_rrr_bitvector_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def rank_device(self, d_idx_ptr, d_out_ptr, count, stream=None):
        check(lib().vlg_rrr_bitvector_rank_batch(self._h, d_idx_ptr, d_out_ptr, count, stream))

    def select_support(self, sample=0, stream=None):
        """select_support_rrr<1> and <0> over this bit-vector (SelectSupport.bit_select)"""
        return SelectSupport(self, sample, stream)

    def hbm_bytes(self):
        return int(lib().vlg_rrr_bitvector_hbm_bytes(self._h))
