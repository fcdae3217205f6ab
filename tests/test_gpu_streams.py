"""Stream ordering and concurrent workspaces across the C API (include/vlg_hip.h: "`stream` is a hipStream_t passed as void*",
"batched calls on different streams may share [an index]", "a vlg_workspace / vlg_result belongs to one caller thread at a time").

Every entry point that takes a `stream` has a row in ROWS and runs on a fresh non-blocking stream in the two passes of
tests/stream_order.py (late inputs; a busy NULL stream), against references computed from the text by numpy: the suffix array by
sorting, isa / lf / psi / bwt by their definitions (test_gpu_select.Truth), pattern intervals and range queries by brute force.  A row
also says whether the header calls the entry point synchronising or asynchronous, and the harness checks that on return.  The searches
run on a Workspace that owns such a stream, over the option sets that send every stage of the pipeline through it, against the oracle
and a NULL-stream run; three host threads with a stream, a workspace and a batch each share one text's indexes.
tests/test_stream_table_cpu.py holds ROWS, SEARCH_ENTRIES and EXCLUDED against the header."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import sdsl_wtsa as W
from stream_order import Case, StreamOrder
from test_gpu_select import Truth, pack_bits, suffix_array_doubling, with_sentinel
from util import dna_text, naive_sa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


# ---- device tensors of the dtypes the C API takes --------------------------------------------------------------------------------------
def dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def pair(torch, real, poison):
    real, poison = np.ascontiguousarray(real), np.ascontiguousarray(poison)
    assert real.shape == poison.shape and real.dtype == poison.dtype
    return dev(torch, real), dev(torch, poison)


def rot(a):
    """a rotated copy: in range wherever `a` is, and different from it in most places"""
    return np.roll(a, len(a) // 3 + 1)


# ---- references ------------------------------------------------------------------------------------------------------------------------
def rank_ref(bwt, pos, sym):
    """#sym[j] in bwt[0, pos[j]) for symbols that occur"""
    uniq, inv = np.unique(bwt, return_inverse=True)
    cum = np.zeros((len(uniq), len(bwt) + 1), np.int64)
    cum[inv.reshape(-1), np.arange(len(bwt)) + 1] = 1
    cum = np.cumsum(cum, axis=1)
    k = np.searchsorted(uniq, sym)
    assert (uniq[k] == sym).all()
    return cum[k, np.asarray(pos, np.int64)].astype(np.uint64)


def occurrences(full, pat):
    """start positions of pat (an array of symbols) in the text with its sentinel, by comparing everywhere"""
    m, n = len(pat), len(full)
    ok = np.ones(n - m + 1, bool)
    for j in range(m):
        ok &= full[j:n - m + 1 + j] == pat[j]
    return np.flatnonzero(ok)


def interval_ref(truth, pat):
    """[l, r] of a pattern that occurs: the suffixes that begin with it are consecutive in the suffix array"""
    occ = occurrences(truth.full, pat)
    assert len(occ)
    at = truth.isa[occ].astype(np.int64)
    assert at.max() - at.min() + 1 == len(occ)
    return int(at.min()), int(at.max())


class Side:
    """one alphabet: text, truth, the four kinds of index, patterns with their intervals"""

    def __init__(self, V, text, is_int):
        self.is_int = is_int
        self.text = text
        self.full = with_sentinel(text).astype(np.uint32 if is_int else np.uint8)
        sa = suffix_array_doubling(self.full) if is_int else naive_sa(self.full)
        self.truth = Truth(self.full, sa)
        self.n = self.truth.n
        plain = V.VlgIndex.build_int(text) if is_int else V.VlgIndex.build(text.tobytes())
        self.idx = {"plain": plain, "rrr": plain.compress()}
        assert plain.info()["pos_bytes"] == 4
        self.wtsa = V.WtsaIndex(text)
        rng = np.random.default_rng(11 + is_int)
        starts, lens = rng.integers(0, len(text) - 8, 300), rng.integers(1, 9, 300)
        self.pats = [text[s:s + m] for s, m in zip(starts, lens)]
        self.lr = np.array([interval_ref(self.truth, p) for p in self.pats], np.uint64)
        other = [text[s:s + m] for s, m in zip(rng.integers(0, len(text) - 8, 300), lens)]          # poison: other patterns, the same lengths
        sym = 4 if is_int else 1
        self.blob = np.concatenate(self.pats + [np.zeros(1, text.dtype)]).view(np.uint8)
        self.blob_poison = np.concatenate(other + [np.zeros(1, text.dtype)]).view(np.uint8)
        self.off = (np.concatenate([[0], np.cumsum(lens)]) * sym).astype(np.uint64)
        self.sym_torch = "int32" if is_int else "uint8"


class World:
    def __init__(self, torch, V):
        from vlg_matching_amd.index import Queries
        self.torch, self.V = torch, V
        rng = np.random.default_rng(2024)
        big = np.unique(np.concatenate([rng.integers(1, 2 ** 32 - 1, 49, dtype=np.uint64), np.array([1, 2 ** 32 - 1], np.uint64)]))
        self.side = {"byte": Side(V, dna_text(3000, 5), False), "int": Side(V, rng.choice(big, 3000).astype(np.uint32), True)}
        self.nbits = 10 ** 5
        self.bits = (rng.random(self.nbits) < 0.5).astype(np.uint8)
        self.bv = {"plain": V.BitVector(pack_bits(self.bits), self.nbits), "rrr": V.RrrBitVector(pack_bits(self.bits), self.nbits)}
        self.bv_sel = {k: b.select_support(64) for k, b in self.bv.items()}
        self.sel = {(a, k): ix.select_support(64) for a, s in self.side.items() for k, ix in s.idx.items()}
        self.access = {a: s.idx["plain"].text_access(64) for a, s in self.side.items()}
        # query batches whose sub-patterns are known: (regexps, sub-patterns in batch order)
        self.queries = {}
        for a, s in self.side.items():
            qs, subs = [], []
            for j in range(0, 120, 2):
                p, q = s.pats[j], s.pats[j + 1]
                if a == "byte":
                    qs.append(p.tobytes().decode() + ".{0,40}?" + q.tobytes().decode())
                else:
                    qs.append(" ".join(map(str, p)) + " .{0,40}? " + " ".join(map(str, q)))
                subs += [j, j + 1]
            self.queries[a] = (Queries(qs) if a == "byte" else Queries.from_int(qs), np.array(subs))
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(torch_cuda, V):
    return World(torch_cuda, V)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
class Row:
    """entry: the C entry point; sync: the header says it synchronises `stream` (False: it says asynchronous); make(world) -> Case"""

    def __init__(self, entry, variant, sync, make):
        self.entry, self.variant, self.sync, self.make = entry, variant, sync, make
        self.id = entry[4:] + ("-" + variant if variant else "")


ROWS = []


def row(entry, sync, variants=("",)):
    def deco(fn):
        for v in variants:
            ROWS.append(Row(entry, v, sync, (lambda w, v=v: fn(w, v)) if v else (lambda w: fn(w, ""))))
        return fn
    return deco


INDEX_KINDS = ("byte-plain", "byte-rrr", "int-plain", "int-rrr")
BYTE_KINDS, INT_KINDS = INDEX_KINDS[:2], INDEX_KINDS[2:]


def _side(w, variant):
    a, k = variant.split("-")
    return w.side[a], w.side[a].idx[k]


def _check(w, status):
    w.V.capi.check(status)


def _u64_out(count):
    import torch
    return (count, torch.int64)


@row("vlg_bitvector_rank_batch", False, ("plain",))
@row("vlg_rrr_bitvector_rank_batch", False, ("rrr",))
def bit_rank_row(w, kind):
    L = w.V.lib()
    f = L.vlg_bitvector_rank_batch if kind == "plain" else L.vlg_rrr_bitvector_rank_batch
    i = np.random.default_rng(1).integers(0, w.nbits + 1, 4000).astype(np.uint64)
    want = np.concatenate([[0], np.cumsum(w.bits)]).astype(np.uint64)[i.astype(np.int64)]
    return Case(lambda st, ins, outs, mark: _check(w, f(w.bv[kind]._h, ins[0].data_ptr(), outs[0].data_ptr(), len(i), st)),
                [pair(w.torch, i, rot(i))], [_u64_out(len(i))], [want])


def _rank_row(w, variant):
    s, idx = _side(w, variant)
    L = w.V.lib()
    f = L.vlg_int_rank_batch if s.is_int else L.vlg_wt_rank_batch
    rng = np.random.default_rng(2)
    pos = rng.integers(0, s.n + 1, 4000).astype(np.uint64)
    sym = s.full[rng.integers(0, s.n, 4000)]
    want = rank_ref(s.truth.bwt, pos, sym)
    return Case(lambda st, ins, outs, mark: _check(w, f(idx._h, ins[0].data_ptr(), ins[1].data_ptr(), outs[0].data_ptr(), len(pos), st)),
                [pair(w.torch, pos, rot(pos)), pair(w.torch, sym, rot(sym))], [_u64_out(len(pos))], [want])


row("vlg_wt_rank_batch", False, BYTE_KINDS)(_rank_row)
row("vlg_int_rank_batch", False, INT_KINDS)(_rank_row)


@row("vlg_backward_search_batch", False, INDEX_KINDS)
def backward_search_row(w, variant):
    s, idx = _side(w, variant)
    m = len(s.pats)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_backward_search_batch(idx._h, ins[0].data_ptr(), ins[1].data_ptr(), m,
                                                                                      outs[0].data_ptr(), outs[1].data_ptr(), st)),
                [pair(w.torch, s.blob, s.blob_poison), pair(w.torch, s.off, s.off)], [_u64_out(m), _u64_out(m)], [s.lr[:, 0], s.lr[:, 1]])


@row("vlg_sa_batch", True, INDEX_KINDS)
def sa_row(w, variant):
    s, idx = _side(w, variant)
    i = np.random.default_rng(3).permutation(s.n).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_sa_batch(idx._h, ins[0].data_ptr(), outs[0].data_ptr(), s.n, st)),
                [pair(w.torch, i, i[::-1])], [_u64_out(s.n)], [s.truth.sa.astype(np.uint64)[i.astype(np.int64)]])


@row("vlg_locate_batch", True, INDEX_KINDS)
def locate_row(w, variant):
    s, idx = _side(w, variant)
    l, r = s.lr[:, 0], s.lr[:, 1]
    ln = r + np.uint64(1) - l
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    total = int(off[-1])
    pl = np.uint64(s.n) - (r + np.uint64(1))                          # poison: the mirrored ranges, the same lengths and offsets
    want = np.concatenate([s.truth.sa[int(a):int(b) + 1] for a, b in zip(l, r)]).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_locate_batch(idx._h, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                                                                             len(l), total, outs[0].data_ptr(), st)),
                [pair(w.torch, l, pl), pair(w.torch, r, pl + ln - np.uint64(1)), pair(w.torch, off, off)], [_u64_out(total)], [want])


@row("vlg_lf_batch", False, INDEX_KINDS)
def lf_row(w, variant):
    s, idx = _side(w, variant)
    i = np.random.default_rng(4).permutation(s.n).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_lf_batch(idx._h, ins[0].data_ptr(), outs[0].data_ptr(), s.n, st)),
                [pair(w.torch, i, i[::-1])], [_u64_out(s.n)], [s.truth.lf[i.astype(np.int64)]])


@row("vlg_bwt_batch", False, INDEX_KINDS)
def bwt_row(w, variant):
    s, idx = _side(w, variant)
    i = np.random.default_rng(5).permutation(s.n).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_bwt_batch(idx._h, ins[0].data_ptr(), outs[0].data_ptr(), s.n, st)),
                [pair(w.torch, i, i[::-1])], [(s.n, getattr(w.torch, s.sym_torch))], [s.truth.bwt[i.astype(np.int64)]])


# ---- text access ----------------------------------------------------------------------------------------------------------------------
def _isa_case(w, a, access_of):
    """csa.isa of every position through access_of(stream, mark): the probe of a creation, or the row of vlg_isa_batch itself"""
    s = w.side[a]
    i = np.random.default_rng(6).permutation(s.n).astype(np.uint64)

    def call(st, ins, outs, mark):
        t = access_of(st, mark)
        t.isa_device(ins[0].data_ptr(), outs[0].data_ptr(), s.n, stream=st)
        return t
    return Case(call, [pair(w.torch, i, i[::-1])], [_u64_out(s.n)], [s.truth.isa[i.astype(np.int64)]])


@row("vlg_text_access_create", True, ("byte", "int"))
def text_access_create_row(w, a):
    def create(st, mark):
        t = w.side[a].idx["plain"].text_access(16, stream=st)
        mark()
        return t
    return _isa_case(w, a, create)


@row("vlg_isa_batch", True, ("byte", "int"))
def isa_row(w, a):
    return _isa_case(w, a, lambda st, mark: w.access[a])


@row("vlg_extract_batch", True, ("byte", "int"))
def extract_row(w, a):
    s = w.side[a]
    rng = np.random.default_rng(7)
    ln = rng.integers(1, 200, 400)
    b = rng.integers(0, s.n - ln + 1).astype(np.uint64)
    pb = rng.integers(0, s.n - ln + 1).astype(np.uint64)              # poison: other ranges of the same lengths, the same out_off
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    total = int(off[-1])
    ln = ln.astype(np.uint64)
    want = np.concatenate([s.full[int(x):int(x + m)] for x, m in zip(b, ln)])
    return Case(lambda st, ins, outs, mark: w.access[a].extract_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), len(b), total,
                                                                      outs[0].data_ptr(), stream=st),
                [pair(w.torch, b, pb), pair(w.torch, b + ln - np.uint64(1), pb + ln - np.uint64(1)), pair(w.torch, off, off)],
                [(total, getattr(w.torch, s.sym_torch))], [want])


# ---- select -----------------------------------------------------------------------------------------------------------------------------
def _bit_select_case(w, kind, support_of):
    pos = np.flatnonzero(w.bits == 1).astype(np.uint64)
    k = np.random.default_rng(8).integers(0, len(pos) + 2, 4000).astype(np.uint64)
    want = np.full(len(k), w.nbits, np.uint64)
    ok = (k >= 1) & (k <= len(pos))
    want[ok] = pos[k[ok].astype(np.int64) - 1]

    def call(st, ins, outs, mark):
        ss = support_of(st, mark)
        ss.bit_select_device(ins[0].data_ptr(), outs[0].data_ptr(), len(k), bit=1, stream=st)
        return ss
    return Case(call, [pair(w.torch, k, rot(k))], [_u64_out(len(k))], [want])


def _select_case(w, variant, support_of):
    s, idx = _side(w, variant)
    k, c, want = s.truth.select_queries([])
    c = c.astype(np.uint32 if s.is_int else np.uint8)

    def call(st, ins, outs, mark):
        ss = support_of(st, mark)
        ss.select_device(ins[0].data_ptr(), ins[1].data_ptr(), outs[0].data_ptr(), len(k), stream=st)
        return ss
    return Case(call, [pair(w.torch, k, rot(k)), pair(w.torch, c, rot(c))], [_u64_out(len(k))], [want])


@row("vlg_bitvector_select_create", True, ("plain",))
@row("vlg_rrr_bitvector_select_create", True, ("rrr",))
def bit_select_create_row(w, kind):
    def create(st, mark):
        ss = w.bv[kind].select_support(64, stream=st)
        mark()
        return ss
    return _bit_select_case(w, kind, create)


@row("vlg_index_select_create", True, ("byte-plain", "int-rrr"))
def index_select_create_row(w, variant):
    def create(st, mark):
        ss = _side(w, variant)[1].select_support(64, stream=st)
        mark()
        return ss
    return _select_case(w, variant, create)


@row("vlg_bit_select_batch", False, ("plain", "rrr"))
def bit_select_row(w, kind):
    return _bit_select_case(w, kind, lambda st, mark: w.bv_sel[kind])


def _select_row(w, variant):
    return _select_case(w, variant, lambda st, mark: w.sel[tuple(variant.split("-"))])


row("vlg_wt_select_batch", False, BYTE_KINDS)(_select_row)
row("vlg_int_select_batch", False, INT_KINDS)(_select_row)


@row("vlg_psi_batch", False, ("byte-rrr", "int-plain"))
def psi_row(w, variant):
    s, idx = _side(w, variant)
    ss = w.sel[tuple(variant.split("-"))]
    i = np.random.default_rng(9).permutation(s.n).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: ss.psi_device(ins[0].data_ptr(), outs[0].data_ptr(), s.n, stream=st),
                [pair(w.torch, i, i[::-1])], [_u64_out(s.n)], [s.truth.psi[i.astype(np.int64)]])


# ---- builders and export ----------------------------------------------------------------------------------------------------------------
@row("vlg_suffix_array_device", True)
def suffix_array_row(w, _):
    s = w.side["byte"]
    n_text = len(s.text)
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_suffix_array_device(ins[0].data_ptr(), n_text, outs[0].data_ptr(), st)),
                [pair(w.torch, s.text, s.text[::-1])], [(s.n, w.torch.int32)], [s.truth.sa.astype(np.uint32)])


def _sa_bwt_probe(w, s, idx, st, outs):
    """csa[i] and csa.bwt[i] of every i of a new index, on the stream that made it"""
    i = w.torch.arange(s.n, dtype=w.torch.int64, device="cuda")
    _check(w, w.V.lib().vlg_sa_batch(idx._h, i.data_ptr(), outs[0].data_ptr(), s.n, st))
    _check(w, w.V.lib().vlg_bwt_batch(idx._h, i.data_ptr(), outs[1].data_ptr(), s.n, st))
    return i


@row("vlg_index_build_device", True)
def build_device_row(w, _):
    s = w.side["byte"]

    def call(st, ins, outs, mark):
        idx = w.V.VlgIndex.build_device(ins[0].data_ptr(), len(s.text), 32, stream=st)
        mark()
        return idx, _sa_bwt_probe(w, s, idx, st, outs)
    return Case(call, [pair(w.torch, s.text, s.text[::-1])], [_u64_out(s.n), (s.n, w.torch.uint8)], [s.truth.sa.astype(np.uint64), s.truth.bwt])


@row("vlg_index_blob_export", True, ("byte", "int"))
def blob_export_row(w, a):
    s = w.side[a]
    idx = s.idx["plain"]
    nbytes = idx.blob_bytes()

    def verify(got, returned):
        """the exported image, as the clone on the stream saw it, attached: it answers like the index"""
        blob = w.torch.from_numpy(got[0]).cuda()
        att = w.V.VlgIndex.attach_blob(blob.data_ptr(), nbytes, keep=blob)
        assert att.info() == idx.info()
        outs = [w.torch.zeros(s.n, dtype=w.torch.int64, device="cuda"), w.torch.zeros(s.n, dtype=getattr(w.torch, s.sym_torch), device="cuda")]
        _sa_bwt_probe(w, s, att, None, outs)
        w.torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy().view(np.uint64), s.truth.sa.astype(np.uint64))
        assert np.array_equal(outs[1].cpu().numpy().view(s.full.dtype), s.truth.bwt)
    return Case(lambda st, ins, outs, mark: idx.blob_export(outs[0].data_ptr(), nbytes, stream=st), [], [(nbytes, w.torch.uint8)], [], verify=verify)


# ---- the paper's index ------------------------------------------------------------------------------------------------------------------
def _ranges(s, seed, count=2000, maxlen=300):
    rng = np.random.default_rng(seed)
    ln = rng.integers(1, maxlen, count)
    l = rng.integers(0, s.n - ln + 1)
    return rng, l.astype(np.uint64), ln.astype(np.uint64)


@row("vlg_wtsa_sa_batch", False, ("byte", "int"))
def wtsa_sa_row(w, a):
    s = w.side[a]
    i = np.random.default_rng(12).permutation(s.n).astype(np.uint64)
    return Case(lambda st, ins, outs, mark: s.wtsa.sa_device(ins[0].data_ptr(), outs[0].data_ptr(), s.n, stream=st),
                [pair(w.torch, i, i[::-1])], [_u64_out(s.n)], [s.truth.sa.astype(np.uint64)[i.astype(np.int64)]])


@row("vlg_wtsa_range_walk_batch", False, ("byte-count_less", "byte-quantile", "int-count_less", "int-quantile"))
def wtsa_range_walk_row(w, variant):
    a, what = variant.split("-")
    s = w.side[a]
    quantile = what == "quantile"
    rng, l, ln = _ranges(s, 13)
    x = (rng.integers(0, 2 ** 62, len(l)) % ln.astype(np.int64) if quantile else rng.integers(0, s.n + 1, len(l))).astype(np.uint64)
    pl = np.uint64(s.n) - l - ln                                      # poison: the mirrored ranges; ranks from the other end, other bounds
    px = ln - np.uint64(1) - x if quantile else np.uint64(s.n) - x
    sa = s.truth.sa
    want = np.array([np.sort(sa[int(p):int(p + m)])[int(v)] if quantile else np.count_nonzero(sa[int(p):int(p + m)] < int(v))
                     for p, m, v in zip(l, ln, x)], np.uint64)
    return Case(lambda st, ins, outs, mark: s.wtsa.range_walk_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), quantile,
                                                                    outs[0].data_ptr(), len(l), stream=st),
                [pair(w.torch, l, pl), pair(w.torch, ln, ln), pair(w.torch, x, px)], [_u64_out(len(l))], [want])


def _range_2d(s, seed):
    rng, l, ln = _ranges(s, seed, 600)
    v = np.sort(rng.integers(0, s.n, (len(l), 2)), axis=1).astype(np.uint64)
    vlb, vrb = np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1])
    inside = []
    for p, m, a, b in zip(l, ln, vlb, vrb):
        x = s.truth.sa[int(p):int(p + m)]
        inside.append(np.sort(x[(x >= int(a)) & (x <= int(b))]))
    mirror = np.uint64(s.n - 1)
    return l, ln, vlb, vrb, inside, [(l, np.uint64(s.n) - l - ln), (ln, ln), (vlb, mirror - vrb), (vrb, mirror - vlb)]


@row("vlg_wtsa_range_count_batch", False, ("byte", "int"))
def wtsa_range_count_row(w, a):
    s = w.side[a]
    l, ln, vlb, vrb, inside, pairs = _range_2d(s, 14)
    return Case(lambda st, ins, outs, mark: s.wtsa.range_count_device(*[t.data_ptr() for t in ins], outs[0].data_ptr(), len(l), stream=st),
                [pair(w.torch, r, p) for r, p in pairs], [_u64_out(len(l))], [np.array([len(x) for x in inside], np.uint64)])


@row("vlg_wtsa_range_report_batch", False, ("byte", "int"))
def wtsa_range_report_row(w, a):
    """the poison ranges hold other numbers of values than the offsets say: the kernel writes no element past a range's own count and
    none past `total` (wtsa_range_report_kernel), so a premature read leaves sentinels and wrong values, nothing else"""
    s = w.side[a]
    l, ln, vlb, vrb, inside, pairs = _range_2d(s, 15)
    off = np.concatenate([[0], np.cumsum([len(x) for x in inside])]).astype(np.uint64)
    total = int(off[-1])
    return Case(lambda st, ins, outs, mark: s.wtsa.range_report_device(*[t.data_ptr() for t in ins], len(l), total, outs[0].data_ptr(), stream=st),
                [pair(w.torch, r, p) for r, p in pairs] + [pair(w.torch, off, off)], [_u64_out(total)], [np.concatenate(inside).astype(np.uint64)])


@row("vlg_wtsa_il_device", False, ("byte", "int"))
def wtsa_il_row(w, a):
    s = w.side[a]
    data = W.il_members(W.wt_levels(s.truth.sa))[3]
    return Case(lambda st, ins, outs, mark: s.wtsa.il_device(outs[0].data_ptr(), len(data), stream=st), [], [_u64_out(len(data))], [data])


# ---- calls that return host data; the stand-alone sort ----------------------------------------------------------------------------------
def _query_intervals(w, a):
    s = w.side[a]
    q, subs = w.queries[a]
    return s, q, s.lr[subs, 0], s.lr[subs, 1]


@row("vlg_wtsa_ranges", True, ("byte", "int"))
def wtsa_ranges_row(w, a):
    s, q, l, r = _query_intervals(w, a)

    def call(st, ins, outs, mark):
        sp, ep = np.zeros(len(l), np.uint64), np.zeros(len(l), np.uint64)
        _check(w, w.V.lib().vlg_wtsa_ranges(s.wtsa._h, q._h, sp.ctypes.data, ep.ctypes.data, st))
        return sp, ep
    return Case(call, host=(l, r))


@row("vlg_queries_intervals", True, ("byte-plain", "int-rrr"))
def queries_intervals_row(w, variant):
    s, q, l, r = _query_intervals(w, variant.split("-")[0])
    idx = _side(w, variant)[1]

    def call(st, ins, outs, mark):
        hl, hr = np.zeros(len(l), np.uint64), np.zeros(len(l), np.uint64)
        _check(w, w.V.lib().vlg_queries_intervals(idx._h, q._h, hl.ctypes.data, hr.ctypes.data, st))
        return hl, hr
    return Case(call, host=(l, r))


@row("vlg_queries_occurrences", True, ("byte-rrr", "int-plain"))
def queries_occurrences_row(w, variant):
    s, q, l, r = _query_intervals(w, variant.split("-")[0])
    idx = _side(w, variant)[1]

    def call(st, ins, outs, mark):
        occ = np.zeros(len(l), np.uint64)
        _check(w, w.V.lib().vlg_queries_occurrences(idx._h, q._h, occ.ctypes.data, st))
        return (occ,)
    return Case(call, host=(r + np.uint64(1) - l,))


@row("vlg_sort_lists_u32", True, ("mode1", "mode2"))
def sort_lists_row(w, variant):
    rng = np.random.default_rng(16)
    lens = [0, 1, 65, 257, 2049, 4097, 12289]                         # empty, single, short (LDS), long (windows)
    lists = [rng.choice(1 << 30, n, replace=False).astype(np.uint32) for n in lens]
    poison = [rng.choice(1 << 30, n, replace=False).astype(np.uint32) for n in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mode = int(variant[-1])
    return Case(lambda st, ins, outs, mark: _check(w, w.V.lib().vlg_sort_lists_u32(ins[0].data_ptr(), off.ctypes.data, len(lens), 30, mode, None, st)),
                [pair(w.torch, np.concatenate(lists), np.concatenate(poison))], in_place={0: np.concatenate([np.sort(x) for x in lists])})


# the searches of section 3 (they take their stream from the workspace) and what no row covers, each with its reason
SEARCH_ENTRIES = ("vlg_search_batch", "vlg_join_batch", "vlg_wtsa_search_batch", "vlg_wtsa_search_window_batch")
EXCLUDED = {
    "vlg_index_broadcast": "a collective: needs the ranks of an RCCL communicator (tests/test_gpu_parity.py runs it with its ranks)",
    "vlg_comm_allreduce_sum_u64": "a collective: needs the ranks of an RCCL communicator",
    "vlg_comm_allgatherv": "a collective: needs the ranks of an RCCL communicator",
    "vlg_comm_alltoallv": "a collective: needs the ranks of an RCCL communicator",
    "vlg_workspace_create": "stores the stream, launches nothing; every search test creates one with a stream",
    "vlg_workspace_destroy": "launches nothing",
    "vlg_workspace_profile": "launches nothing (waits for the events of earlier searches); the search tests turn it on",
    "vlg_workspace_set_option": "launches nothing",
    "vlg_workspace_kernel_stats": "launches nothing (waits for the events of earlier searches); the search tests read it",
    "vlg_workspace_set_comm": "launches nothing; needs an RCCL communicator",
    "vlg_workspace_set_exchange": "launches nothing; the exchange belongs to the collective search",
    "vlg_workspace_set_exchange_alltoall": "launches nothing; the exchange belongs to the collective search",
}


# ---- the harness --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(torch_cuda, world):
    """the calibrated delay: at least the floor, at least ten times the longest call of the table on the NULL stream"""
    h = StreamOrder(torch_cuda)
    longest, slowest = 0.0, ""
    for r in ROWS:
        case = r.make(world)
        ins = [real.clone() for real, _ in case.inputs]
        outs = [torch_cuda.empty(shape, dtype=dtype, device="cuda") for shape, dtype in case.outputs]
        kept = []
        run = lambda: kept.append(case.call(None, ins, outs, lambda: None))      # noqa: E731
        ms = min(h.time_on_null_stream(run), h.time_on_null_stream(run))           # (the first run also loads the kernels' code)
        if ms > longest:
            longest, slowest = ms, r.id
    h.set_delay(longest)
    print("\nstream harness: %.0f sleep cycles per ms; longest call of the table on the NULL stream %.2f ms (%s); delay %.0f ms"
          % (h.cycles_per_ms, longest, slowest, h.delay_ms))
    return h


def test_control_the_harness_sees_a_mistake(harness):
    """torch alone: delay + copy-over-poison on S, and a clone issued at once on a second non-blocking stream.  The clone must hold the
    poison; if it holds the real values, a call that ran ahead of its inputs would pass every test of this file unseen."""
    got, poison, real = harness.control()
    assert not np.array_equal(poison, real)
    assert np.array_equal(got, poison), "the harness is blind: a read that was not ordered behind a %.0f ms delay saw the late copy (%d of %d elements)" % (
        harness.delay_ms, int(np.count_nonzero(got == real)), len(real))


def test_control_a_launch_left_on_the_null_stream_runs_ahead(harness):
    """the early clone on the NULL stream itself: the stream the harness picked does not hold the NULL stream back"""
    got, poison, real = harness.control_null_stream()
    assert np.array_equal(got, poison), "the harness is blind: work on the NULL stream waited for the stream under test (%d of %d elements)" % (
        int(np.count_nonzero(got == real)), len(real))


def test_streams_under_test_are_non_blocking(harness):
    from stream_order import HIP_STREAM_NON_BLOCKING
    s = harness.new_stream()
    assert harness.stream_flags(s) & HIP_STREAM_NON_BLOCKING


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("r", ROWS, ids=[r.id for r in ROWS])
def test_entry_point_on_its_stream(harness, world, r, which):
    """pass A: late inputs; pass B: a busy NULL stream (tests/stream_order.py).  The header's word on synchronisation is checked on
    return: a synchronising call leaves its stream idle; an asynchronous one, in pass A, returns while the delay is still running."""
    case = r.make(world)
    assert which == "B" or case.poison_ok, "row %s has no safe poison: it runs pass B only and must say so in the table" % r.id
    idle = harness.run(case, which)
    print("%s pass %s: stream idle on return: %s (header: %s)" % (r.id, which, idle, "synchronises" if r.sync else "asynchronous"))
    if r.sync:
        assert idle, "%s: the header says it synchronises `stream`, and the stream was busy on return" % r.entry
    elif which == "A":
        assert not idle, "%s: the header says asynchronous, and the stream was idle on return behind a %.0f ms delay" % (r.entry, harness.delay_ms)


# ---- searches on a workspace that owns a stream --------------------------------------------------------------------------------------
def _expected_arrays(want, ks):
    """the oracle's tuple lists as the arrays vlg_result_fetch gives: counts, offsets, first positions, tuples"""
    counts = np.array([len(x) for x in want], np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    first = np.array([t[0] for x in want for t in x], np.uint64)
    tup = np.array([v for x in want for t in x for v in t], np.uint64)
    assert all(len(t) == k for x, k in zip(want, ks) for t in x)
    return counts, off, first, tup


class SearchWorld:
    def __init__(self, V, oracle):
        from test_gpu_parity import TEXTS, _int_queries, random_queries
        from vlg_matching_amd.index import Queries
        self.V = V
        self.text = TEXTS["dna_50k"]()
        o = oracle.Index.from_text(self.text)
        qs = random_queries(self.text, np.random.default_rng(9), 300, kmax=3, mmax=3)
        qs += ["\xfe.{0,5}?" + qs[0][:1], qs[1][:1] + ".{0,5}?\xfe"]
        self.qs = qs
        self.want = [o.search(q).tolist() for q in qs]
        self.plain = V.VlgIndex.build(self.text)
        self.index = {"plain": self.plain, "rrr": self.plain.compress(), "text-order": self.plain.resample(text_order=True, dens=32)}
        self.q = Queries(qs)
        self.arrays = _expected_arrays(self.want, self.q.ks)
        # the window [B, E) of the whole batch: the oracle on the stand-alone text, shifted
        self.B, self.E = 10000, 35000
        ow = oracle.Index.from_text(self.text[self.B:self.E])
        self.want_window = [[[v + self.B for v in t] for t in ow.search(q).tolist()] for q in qs]
        # an integer text and its batch
        rng = np.random.default_rng(31)
        self.int_text = (1 + rng.zipf(1.3, 20000) % 3000).astype(np.uint32)
        self.int_qs = _int_queries(self.int_text, rng, 150)
        oi = oracle.IntIndex(self.int_text.astype(np.uint64), dens=32)
        self.int_want = [oi.search(q).tolist() for q in self.int_qs]
        self.index["int"] = V.VlgIndex.build_int(self.int_text)
        self.int_q = Queries.from_int(self.int_qs)
        self.int_arrays = _expected_arrays(self.int_want, self.int_q.ks)
        self.wtsa = V.WtsaIndex(self.text)


@pytest.fixture(scope="module")
def sw(V, oracle, torch_cuda):
    return SearchWorld(V, oracle)


SWEEP = {"sweep_min": 1, "sweep_tail": 16}
# (name, index, cap in MiB, options, what the summary / kernel statistics must show)
OPTION_SETS = [
    ("defaults", "plain", 0, {}, None),
    ("dedup0", "plain", 0, {"dedup": 0}, None),
    ("sweep", "plain", 0, dict(SWEEP, global_sort_min=1), lambda s, ks: s["locate_mode"] == 2),
    ("trail", "plain", 0, dict(SWEEP, trail=1, list_sort=0, global_sort_min=1), lambda s, ks: s["locate_mode"] == 2),
    ("segmented-sort", "plain", 0, dict(SWEEP, trail=0, list_sort=0, global_sort_min=1 << 40), lambda s, ks: s["locate_mode"] == 2),
    ("unsample", "plain", 0, dict(SWEEP, unsample_pct=1, unsample_min=1, unsample_tail=16), lambda s, ks: s["locate_mode"] == 3),
    ("streamed-filter", "plain", 0, {"filter_min": 0, "filter_stream_min": 0, "filter_pivot": 0}, lambda s, ks: s["filter_stream_segments"] > 0),
    ("pivot-bits", "plain", 0, {"filter_min": 0, "filter_stream_min": 0, "filter_pivot_ratio": 2, "pivot_range_ratio": 0},
     lambda s, ks: s["filter_bit_segments"] > 0),
    ("cap", "plain", 48, {"reserve": 48 << 20}, lambda s, ks: s["n_chunks"] > 1),
    ("tuples0", "plain", 0, {"tuples": 0}, lambda s, ks: s["n_tuple_values"] == 0),
    ("rrr", "rrr", 0, SWEEP, None),
    ("text-order", "text-order", 0, SWEEP, None),
    ("int", "int", 0, SWEEP, None),
]


def _workspace(opts, cap_mb=0, stream=None, profile=False):
    from vlg_matching_amd.index import Workspace
    ws = Workspace(cap_mb << 20, stream=stream)
    for k, v in opts.items():
        ws.set_option(k, v)
    if profile:
        ws.profile(True)
    return ws


def _launches(ws):
    return {k: v["launches"] for k, v in ws.kernel_stats().items()}


def _compare(res, arrays, tuples=True, fetch32=False):
    """what the call returned, fetched with no synchronisation of the test's own, against the oracle's arrays"""
    counts, off, first, tup = res.fetch()
    assert np.array_equal(counts, arrays[0]), "counts differ from the oracle's"
    assert np.array_equal(off, arrays[1])
    assert np.array_equal(first, arrays[2]), "first positions differ from the oracle's"
    assert np.array_equal(tup, arrays[3] if tuples else arrays[3][:0]), "tuples differ from the oracle's"
    if fetch32:
        f32, t32 = res.fetch32()
        assert np.array_equal(f32.astype(np.uint64), first) and np.array_equal(t32.astype(np.uint64), tup), "fetch32 differs from fetch"
    s = res.summary
    assert s["n_matches"] == int(arrays[0].sum()) and s["checksum"] == int(arrays[2].sum(dtype=np.uint64))
    return counts, off, first, tup


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _search_three_ways(h, torch, search, arrays, opts, cap_mb, shows, fetch32=False, late=None):
    """search(ws) on the NULL stream, then on a workspace that owns a fresh non-blocking stream in pass A (profile off) and pass B
    (profile on): each against the oracle's arrays, against the NULL-stream run array for array and in every summary field (none of
    them is a time), and in the launch counts of the kernel statistics.  late: (staging, real, poison) tensors -- pass A copies the real
    ones over the poison on the stream, behind the delay: the device lists of vlg_join_batch."""
    tuples = opts.get("tuples", 1) != 0
    ws0 = _workspace(opts, cap_mb, None, profile=True)
    if late:
        for buf, real in zip(late[0], late[1]):
            buf.copy_(real)
    torch.cuda.synchronize()
    r0 = search(ws0)
    base = _compare(r0, arrays, tuples, fetch32)
    summary0, launches0 = dict(r0.summary), _launches(ws0)
    if shows is not None:
        assert shows(summary0, ws0.kernel_stats()), (summary0, launches0)
    del r0
    for which in ("A", "B"):
        s = h.new_stream()
        ws = _workspace(opts, cap_mb, s.cuda_stream, profile=which == "B")
        if late and which == "A":
            for buf, poison in zip(late[0], late[2]):
                buf.copy_(poison)
        torch.cuda.synchronize()
        h.delay(s if which == "A" else None)
        if late and which == "A":
            with torch.cuda.stream(s):
                for buf, real in zip(late[0], late[1]):
                    buf.copy_(real, non_blocking=True)
        res = search(ws)
        assert s.query(), "pass %s: the search returned with its workspace's stream still busy" % which
        got = _compare(res, arrays, tuples, fetch32)
        assert _same(got, base), "pass %s differs from the NULL-stream run" % which
        assert dict(res.summary) == summary0, ("pass %s" % which, res.summary, summary0)
        assert _launches(ws) == launches0, ("pass %s" % which, _launches(ws), launches0)
        del res
        torch.cuda.synchronize()


@pytest.mark.parametrize("name,index,cap_mb,opts,shows", OPTION_SETS, ids=[o[0] for o in OPTION_SETS])
def test_search_batch_on_a_workspace_stream(harness, torch_cuda, sw, name, index, cap_mb, opts, shows):
    idx = sw.index[index]
    q, arrays = (sw.int_q, sw.int_arrays) if index == "int" else (sw.q, sw.arrays)
    _search_three_ways(harness, torch_cuda, lambda ws: idx.search(q, workspace=ws), arrays, opts, cap_mb, shows, fetch32=True)


def test_search_batch_with_64bit_positions_on_a_workspace_stream(harness, torch_cuda, sw, V, monkeypatch):
    """VLG_FORCE_POS64=1, set before the build: the pos_t = uint64_t instantiations of locate, sort, filter and join"""
    monkeypatch.setenv("VLG_FORCE_POS64", "1")
    idx = V.VlgIndex.build(sw.text)
    assert idx.info()["pos_bytes"] == 8
    opts = dict(SWEEP, global_sort_min=1, filter_min=0, filter_stream_min=0)
    _search_three_ways(harness, torch_cuda, lambda ws: idx.search(sw.q, workspace=ws), sw.arrays, opts, 0, lambda s, ks: ks["filter_compact"]["launches"] > 0)


@pytest.mark.parametrize("rungs", [0, 2])
def test_search_batch_pivot_ranges_on_a_workspace_stream(harness, torch_cuda, V, oracle, rungs):
    """the range-kind segments of the pivot filter through a search: the bracket searches (pivot_rungs 0) and the ladder (2), on the
    text of test_gpu_pivot_ranges.test_through_a_search_with_both_range_producers"""
    from vlg_matching_amd.index import Queries
    from test_gpu_pivot_ranges import BASE
    lengths = [63, 64, 65, 1023, 1025, 4097]
    rng = np.random.default_rng(4400)
    slots = sum(lengths) + 64
    text = bytearray(rng.choice(np.frombuffer(b"ab", np.uint8), 4 * slots + 16).tobytes())
    at = rng.permutation(slots) * 4
    used = 0
    for i, n_occ in enumerate(lengths):
        for p in at[used:used + n_occ]:
            text[p:p + 2] = bytes([0x80 + i, 0x80 + i])
        used += n_occ
    for p in at[used:used + 12]:
        text[p:p + 2] = b"\xf0\xf0"
    text = bytes(text)
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text)
    qs = []
    for i in range(len(lengths)):
        t = chr(0x80 + i) * 2
        qs += [t + ".{0,300}?\xf0\xf0", t + ".{0,64}?\xf0\xf0.{0,64}?" + t, t + ".{0,200}?" + t + ".{0,200}?\xf0\xf0"]
    q = Queries(qs)
    arrays = _expected_arrays([o.search(x).tolist() for x in qs], q.ks)
    _search_three_ways(harness, torch_cuda, lambda ws: idx.search(q, workspace=ws), arrays, dict(BASE, pivot_rungs=rungs, pivot_range_ratio=1), 0,
                       lambda s, ks: s["filter_range_segments"] > 0 and (ks["filter_ladder"]["launches"] > 0) == (rungs == 2))


JOIN_SETS = [("defaults", {}), ("unfiltered", {"filter": 0}), ("pivot-bits", {"pivot_range_ratio": 0}), ("pivot-ranges", {"pivot_range_ratio": 1})]


@pytest.fixture(scope="module")
def join_world(oracle):
    from test_gpu_pivot_ranges import _direction_cases
    cases = _direction_cases(np.random.default_rng(4100))
    want = [oracle.join(*c)[1].tolist() for c in cases]
    rng = np.random.default_rng(4101)
    poison = []                                                        # other sorted lists of the same lengths, over the same span
    for lists, _, _, _ in cases:
        poison.append([np.sort(rng.choice(60000, size=len(a), replace=False)).astype(np.uint64) for a in lists])
    return cases, want, poison


@pytest.mark.parametrize("name,opts", JOIN_SETS, ids=[j[0] for j in JOIN_SETS])
def test_join_batch_on_a_workspace_stream(harness, torch_cuda, join_world, name, opts):
    """vlg_join_batch gets its device lists late in pass A: copied over other sorted lists of the same lengths behind the delay"""
    from vlg_matching_amd.index import join_batch
    from test_gpu_pivot_ranges import BASE
    torch = torch_cuda
    cases, want, poison = join_world
    if name.startswith("pivot"):
        opts = dict(BASE, **opts)
    flat, pflat, list_off, join_list, lo, hi, end_len = [], [], [0], [0], [], [], []
    for (lists, l, h_, e), plists in zip(cases, poison):
        for i, (a, p) in enumerate(zip(lists, plists)):
            flat.append(np.asarray(a, np.uint64))
            pflat.append(p)
            list_off.append(list_off[-1] + len(a))
            lo.append(0 if i == 0 else l[i - 1])
            hi.append(0 if i == 0 else h_[i - 1])
        join_list.append(len(list_off) - 1)
        end_len.append(e)
    real, bad = dev(torch, np.concatenate(flat)), dev(torch, np.concatenate(pflat))
    buf = real.clone()
    ks = np.diff(np.array(join_list)).astype(np.uint32)
    arrays = _expected_arrays(want, ks)
    shows = {"pivot-bits": lambda s, k: s["filter_bit_segments"] > 0 and s["filter_range_segments"] == 0,
             "pivot-ranges": lambda s, k: s["filter_range_segments"] > 0}.get(name)
    _search_three_ways(harness, torch, lambda ws: join_batch(buf.data_ptr(), list_off, join_list, lo, hi, end_len, ws), arrays, opts, 0, shows,
                       late=([buf], [real], [bad]))


WTSA_SETS = [("defaults", {}, 0), ("tuples0", {"tuples": 0}, 0), ("three-matches", {}, 3)]


def _cut(want, max_matches):
    return [x[:max_matches] for x in want] if max_matches else want


@pytest.mark.parametrize("name,opts,max_matches", WTSA_SETS, ids=[x[0] for x in WTSA_SETS])
def test_wtsa_search_batch_on_a_workspace_stream(harness, torch_cuda, sw, V, name, opts, max_matches):
    def search(ws):
        from vlg_matching_amd.index import SearchResult
        hres = C.c_void_p()
        V.capi.check(V.lib().vlg_wtsa_search_batch(sw.wtsa._h, sw.q._h, max_matches, ws._h, C.byref(hres)))
        return SearchResult(hres, sw.q.ks)
    arrays = _expected_arrays(_cut(sw.want, max_matches), sw.q.ks)
    _search_three_ways(harness, torch_cuda, search, arrays, opts, 0, None)


@pytest.mark.parametrize("name,opts,max_matches", WTSA_SETS, ids=[x[0] for x in WTSA_SETS])
def test_wtsa_search_window_batch_on_a_workspace_stream(harness, torch_cuda, sw, name, opts, max_matches):
    arrays = _expected_arrays(_cut(sw.want_window, max_matches), sw.q.ks)
    _search_three_ways(harness, torch_cuda, lambda ws: sw.wtsa.search(sw.q, max_matches=max_matches, workspace=ws, begin=sw.B, end=sw.E), arrays,
                       opts, 0, None)


# ---- concurrent callers -----------------------------------------------------------------------------------------------------------------
THREAD_SETS = [{}, {"dedup": 0}, dict(SWEEP, global_sort_min=1), {"filter_min": 0, "filter_stream_min": 0, "filter_pivot": 0},
               {"filter_min": 0, "filter_stream_min": 0, "filter_pivot_ratio": 2, "pivot_range_ratio": 1}, dict(SWEEP, trail=0, list_sort=0)]


def test_three_threads_with_a_stream_and_a_workspace_each(harness, torch_cuda, sw, V):
    """Three host threads, each with its own non-blocking stream, Workspace and Queries, on the plain index, the rrr index and the
    paper's index of one text: six batches each under other options, every result fetched, compared with what the oracle answered
    before the threads started, and dropped before the next search -- so that the result cache hands buffers from thread to thread and
    the fetches contend for the staging lanes.  Thread 0 provokes refusals between its batches; every thread finds only its own
    message in vlg_last_error."""
    from vlg_matching_amd.index import Queries
    torch = torch_cuda
    n_q = 100                                                          # (the lazy search of the paper's index pays per match: a third of the batch)
    arrays = _expected_arrays(sw.want[:n_q], sw.q.ks[:n_q])
    targets = [sw.index["plain"], sw.index["rrr"], sw.wtsa]
    errors = [[] for _ in targets]

    def last_error():
        return (V.lib().vlg_last_error() or b"").decode("utf-8", "replace")

    def work(t, stream):
        torch.cuda.set_device(0)
        q = Queries(sw.qs[:n_q])
        for b, opts in enumerate(THREAD_SETS):
            ws = _workspace(opts, 0, stream.cuda_stream if stream is not None else None)
            res = targets[t].search(q, workspace=ws)
            _compare(res, arrays)
            del res
            if t == 0:                                                 # harmless refusals: a query that does not parse, a cap too small
                with pytest.raises(V.VlgError) as e:
                    Queries(["A.{5,1}?C"])
                assert e.value.status == V.capi.E_PARSE and "min-gap > max-gap" in last_error()
                with pytest.raises(V.VlgError) as e:
                    targets[0].search(q, workspace=_workspace({}, 1, stream.cuda_stream if stream is not None else None))
                assert e.value.status == V.capi.E_WORKSPACE and "workspace" in last_error()
            else:                                                      # a refusal of its own, with a text only this thread produces
                name = "no_such_option_of_thread_%d_batch_%d" % (t, b)
                assert V.lib().vlg_workspace_set_option(ws._h, name.encode(), 0) == V.capi.E_INVALID
                assert name in last_error(), last_error()

    def guarded(t, stream):
        try:
            work(t, stream)
        except BaseException as e:          # noqa: B902 -- reported by the parent
            errors[t].append(e)

    # the same work on one thread, one target after the other: the measure of the time limit
    t0 = time.perf_counter()
    for t in range(len(targets)):
        work(t, None)
    torch.cuda.synchronize()
    single = time.perf_counter() - t0
    limit = single * len(targets) * 10
    streams = [harness.new_stream() for _ in targets]
    threads = [threading.Thread(target=guarded, args=(t, streams[t]), daemon=True) for t in range(len(targets))]
    t0 = time.perf_counter()
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, limit - (time.perf_counter() - t0)))
    alive = [t for t, th in enumerate(threads) if th.is_alive()]
    assert not alive, "threads %s still run after %.1f s (the same work took one thread %.1f s)" % (alive, limit, single)
    torch.cuda.synchronize()
    for t, errs in enumerate(errors):
        if errs:
            raise AssertionError("thread %d: %r" % (t, errs[0])) from errs[0]
    print("three threads: %.2f s together, %.2f s one after the other on one thread" % (time.perf_counter() - t0, single))
