"""Document listing (vlg_result_list_documents): per query, the maximal runs of matches whose first positions lie in one document.
The yardstick is numpy on result.fetch() -- per query np.searchsorted(starts, first, "right") - 1, then runs -- cross-checked once
against Documents.locate.  Every case shows on the CPU, before the device is touched, that the border it aims at is really hit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_documents import CLASS_REGEXPS, _brute_docs
from test_gpu_documents import _text as _doc_text
from test_gpu_wtsa_window import U64, _batch, _brute_window, _random_int_queries, _random_queries
from util import dna_text
from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def _runs(first, off, starts):
    """-> (df, pair offsets, docs, counts, first_match) of the matches `first` (all queries, concatenated; query q owns
    [off[q], off[q + 1])) over the documents `starts`"""
    first, off = np.asarray(first, np.uint64), np.asarray(off, np.int64)
    M = len(first)
    doc = np.searchsorted(np.asarray(starts, np.uint64), first, "right") - 1
    head = np.ones(M, bool)
    head[1:] = doc[1:] != doc[:-1]
    head[off[:-1][off[:-1] < M]] = True                                     # a run never continues across a query border
    fm = np.flatnonzero(head)
    pair_off = np.searchsorted(fm, off, "left")
    q_of = np.searchsorted(pair_off, np.arange(len(fm)), "right") - 1
    end = np.minimum(np.append(fm[1:], M), off[q_of + 1]) if len(fm) else np.zeros(0, np.int64)
    return np.diff(pair_off), pair_off, doc[fm], end - fm, fm


def _same(listing, want, tag):
    df, pair_off, docs, counts, fm = want
    assert listing.n_queries == len(df) and listing.n_pairs == len(fm), tag
    assert listing.df.tolist() == df.tolist(), tag
    assert listing.offsets.tolist() == pair_off.tolist(), tag
    if listing.has_pairs:
        assert listing.docs.tolist() == docs.tolist(), tag
        assert listing.counts.tolist() == counts.tolist(), tag
        assert listing.first_match.tolist() == fm.tolist(), tag


def _check(V, res, starts, n_text, tag, docs=None):
    """both kinds of listing of a result against numpy on its fetch(); -> the expected listing"""
    docs = docs or V.Documents.from_starts(starts, n_text)
    _, off, first, _ = res.fetch()
    want = _runs(first, off, starts)
    assert int(want[3].sum()) == len(first)
    pairs = res.list_documents(docs)
    _same(pairs, want, tag)
    for q in (0, len(want[0]) // 2, len(want[0]) - 1):
        a, b = int(want[1][q]), int(want[1][q + 1])
        assert [x.tolist() for x in pairs.of(q)] == [want[2][a:b].tolist(), want[3][a:b].tolist(), want[4][a:b].tolist()]
    only_df = res.list_documents(docs, pairs=False)                          # VLG_DOCLIST_DF: df and the number of pairs agree
    _same(only_df, want, tag)
    with pytest.raises(V.VlgError) as err:
        only_df.docs
    assert err.value.status == V.capi.E_INVALID
    return want


def _firsts(V, text, regexps):
    """first positions of every query by brute force on the CPU -> (first, off)"""
    per = [[t[0] for t in _brute_window(text, V.parse_query(q.encode("latin-1")), 0, len(text))] for q in regexps]
    return np.array([x for p in per for x in p], np.uint64), np.concatenate([[0], np.cumsum([len(p) for p in per])])


# ---- 1. lane and run borders -----------------------------------------------------------------------------------------------------
ABAB = b"ab" * 9000


def _border_sets(R):
    n = len(ABAB)
    return {
        "lane0": list(range(0, n, 128)), "lane1": [0] + list(range(130, n, 128)), "lane63": [0] + list(range(126, n, 128)),
        "run_first": [0, 2 * R], "run_second": [0, 2 * R + 2], "run_last": [0, 2 * R - 2],
        "spanning": [0, 2 * (R + R // 2)], "every": list(range(0, n, 2)), "single": [0],
    }


def test_lane_and_run_borders(V):
    """"ab" stands at 2 e: match e is element e of the only piece, lane e % 64 of its step, and a start at 2 e makes it a head"""
    R = V.capi.build_constants()["VLG_DOCLIST_RUN"]
    first, off = _firsts(V, ABAB, ["ab"])
    assert first.tolist() == list(range(0, 18000, 2)) and len(first) > 4 * R     # more than one workgroup of four runs
    sets = _border_sets(R)
    aimed = {}
    for name, starts in sets.items():
        aimed[name] = _runs(first, off, starts)[4][1:]                       # the heads behind match 0
    for lane in (0, 1, 63):
        assert len(aimed["lane%d" % lane]) >= 140 and set((aimed["lane%d" % lane] % 64).tolist()) == {lane}
    assert aimed["run_first"].tolist() == [R] and aimed["run_second"].tolist() == [R + 1] and aimed["run_last"].tolist() == [R - 1]
    assert aimed["spanning"].tolist() == [R + R // 2] and (R + R // 2) % R != 0      # a document across the border of runs 0 and 1, no head there
    assert len(aimed["every"]) == 8999 and len(aimed["single"]) == 0
    idx = V.VlgIndex.build(ABAB)
    res = idx.search(["ab"])
    assert res.fetch()[2].tolist() == first.tolist()
    for name, starts in sets.items():
        want = _check(V, res, starts, len(ABAB), name)
        assert want[4][1:].tolist() == aimed[name].tolist()
    # the yardstick itself, once, against the device's own lookup
    d, _ = V.Documents.from_starts(sets["lane1"], len(ABAB)).locate(first)
    assert d.tolist() == (np.searchsorted(np.asarray(sets["lane1"], np.uint64), first, "right") - 1).tolist()


def _child(env_extra, k, at_least):
    env = dict(os.environ, **env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_doc_listing.py", "-k", k],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= at_least, tail


def test_small_variant_runs_the_border_cases():
    """VLG_DOCLIST_RUN = 192: the same cases in a child pytest that loads the `small` build -- runs of three steps, 47 of them"""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_DOCLIST_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    _child({"VLG_HIP_LIBRARY": lib}, "lane_and_run_borders or query_borders", 2)


def test_stored_document_ids_list_the_same():
    """VLG_DOCLIST_STORE_IDS=1: the head pass stores every match's document and the scatter pass reads it instead of looking the head's
    position up again -- the kept alternate, the same listings (a child process: the switch is read once)"""
    _child({"VLG_DOCLIST_STORE_IDS": "1"}, "lane_and_run_borders or query_borders or fences", 3)


# ---- 2. query borders ------------------------------------------------------------------------------------------------------------
def test_query_borders(V):
    """empty queries at the front of a run of queries, two in a row, at the end; neighbouring queries whose last and first match share
    a document (the head is forced) and do not"""
    text = b"cd" + b"ab" * 3000 + b"cd"
    qs = ["ab", "\xfe", "\xfd", "ba", "ab.{0,2}?ab", "cda", "ab", "\xfc"]
    first, off = _firsts(V, text, qs)
    counts = np.diff(off).tolist()
    assert [c > 0 for c in counts] == [True, False, False, True, True, True, True, False] and counts[5] == 1
    every128 = list(range(0, len(text), 128))
    doc = np.searchsorted(np.asarray(every128, np.uint64), first, "right") - 1
    live = [q for q in range(len(qs)) if counts[q]]
    shared = [bool(doc[off[a + 1] - 1] == doc[off[b]]) for a, b in zip(live[:-1], live[1:])]
    assert shared == [False, False, False, True]                             # "cda" at 0 and the first "ab" at 2: one document, two queries
    single = _runs(first, off, [0])
    assert single[0].tolist() == [int(c > 0) for c in counts] and single[3].tolist() == [c for c in counts if c]
    w128 = _runs(first, off, every128)
    assert w128[0][5] == 1 and w128[0][6] == len(every128) and w128[2][w128[1][6]] == 0 == w128[2][w128[1][5]]
    idx = V.VlgIndex.build(text)
    res = idx.search(qs)
    assert res.fetch()[2].tolist() == first.tolist()
    for name, starts in (("single", [0]), ("every128", every128), ("every", list(range(len(text))))):
        want = _check(V, res, starts, len(text), name)
        assert [x.tolist() for x in want] == [x.tolist() for x in _runs(first, off, starts)]


# ---- 3. fences -------------------------------------------------------------------------------------------------------------------
def _fence_sets(text, first):
    """document counts around one block of fences and around 64 blocks; a match on a document's first symbol, on its last, and one
    behind its first"""
    n = len(text)
    rng = np.random.default_rng(9)
    p = [int(first[len(first) * k // 7]) for k in (1, 2, 3, 4, 5, 6)]
    on = {0, p[0], p[1] + 1, p[2] - 1, p[3], p[3] + 1, p[4] + 1, p[5] - 1}
    sets = {1: [0]}
    for d in (63, 64, 65, 4096, 4097):
        s = set(on)
        pool = rng.permutation(np.arange(1, n))
        for x in pool:
            if len(s) == d:
                break
            s.add(int(x))
        sets[d] = sorted(s)
        assert len(sets[d]) == d
        st = np.asarray(sets[d])
        f = first.astype(np.int64)
        assert np.isin(f, st).any() and np.isin(f + 1, st).any() and np.isin(f - 1, st).any()
    return sets


def test_fences(V):
    text = dna_text(20_000, 17).tobytes()
    qs = ["AC", "GT.{0,6}?A", "T", "CCG"]
    first, off = _firsts(V, text, qs)
    sets = _fence_sets(text, first[off[0]:off[1]])
    idx = V.VlgIndex.build(text)
    res = idx.search(qs)
    assert res.fetch()[2].tolist() == first.tolist() and len(first) > 4096
    for d, starts in sets.items():
        docs = V.Documents.from_starts(starts, len(text))
        assert docs.count() == d
        want = _check(V, res, starts, len(text), d, docs)
        assert d == 1 or want[0][0] > d // 8


# ---- 4. every road ---------------------------------------------------------------------------------------------------------------
def test_every_road(V):
    import torch
    from vlg_matching_amd.index import Workspace, join_batch
    text = _doc_text("dna3000")
    n = len(text)
    rng = np.random.default_rng(21)
    starts = sorted({0} | {int(x) for x in rng.integers(1, n, 75)})
    qs = _random_queries(text, rng, 48, kmax=4, mmax=2, gapmax=30, gaplo=4)
    fields = [V.parse_query(q) for q in qs]
    memo = {}
    bounded = [_brute_docs(text, f, starts, memo) for f in fields]
    whole = [_brute_docs(text, f, [0], memo) for f in fields]
    assert sum(1 for x, y in zip(bounded, whole) if x != y) > 6 and sum(len(w) for w in whole) > 1000
    docs = V.Documents.from_starts(starts, n)
    idx = V.VlgIndex.build(text)
    # a plain search; the rrr index
    res = idx.search(qs)
    want = _check(V, res, starts, n, "plain", docs)
    assert want[0].max() > 20
    _check(V, idx.compress().search(qs), starts, n, "rrr", docs)
    # a document-bounded search with the same handle: the counts are the matches on the stand-alone documents
    batch = V.index.Queries(qs)
    batch.set_documents(docs)
    res = idx.search(batch)
    want = _check(V, res, starts, n, "bounded", docs)
    per_doc = []
    for w in bounded:
        d = np.searchsorted(np.asarray(starts), [t[0] for t in w], "right") - 1
        per_doc += [int((d == j).sum()) for j in sorted(set(d.tolist()))]
    assert want[3].tolist() == per_doc
    batch.set_documents(None)
    # a windowed batch
    batch.set_windows(rng.integers(0, n // 2, len(qs)), rng.integers(n // 2, n, len(qs)))
    res = idx.search(batch)
    assert 0 < res.summary["n_matches"] < sum(len(w) for w in whole)
    _check(V, res, starts, n, "windows", docs)
    # classes, budgets
    q = V.Queries.from_classes(CLASS_REGEXPS)
    _check(V, idx.search(q), starts, n, "classes", docs)
    q.set_mismatches([1] * sum(len(V.parse_class_query(r)[0]) for r in CLASS_REGEXPS))
    res = idx.search(q)
    assert res.summary["n_matches"] > 500
    _check(V, res, starts, n, "budgets", docs)
    # an integer index
    itext = _doc_text("ints")
    iqs, _ = _random_int_queries(itext, rng, 32, mmax=2, gapmax=30, gaplo=4)
    istarts = sorted({0} | {int(x) for x in rng.integers(1, len(itext), 40)})
    res = V.VlgIndex.build_int(itext).search(V.index.Queries.from_int(iqs))
    assert res.summary["n_matches"] > 200
    _check(V, res, istarts, len(itext), "int")
    # vlg_join_batch: caller-built lists, 8-byte positions
    a, b = np.arange(0, 50_000, 5, dtype=np.uint64), np.arange(2, 50_000, 5, dtype=np.uint64)
    lists = torch.from_numpy(np.concatenate([a, b, a[:100]]).view(np.int64)).cuda()
    res = join_batch(lists.data_ptr(), [0, len(a), len(a) + len(b), len(a) + len(b) + 100], [0, 2, 3], [0, 2, 0], [0, 2, 0], [1, 1], Workspace())
    assert res.counts.tolist() == [len(a), 100]
    _check(V, res, list(range(0, 50_000, 777)), 50_002, "join")
    # the lazy index, both entry points (8-byte positions)
    lazy = V.WtsaIndex(text)
    ws = Workspace()
    h = C.c_void_p()
    lq = V.index.Queries(qs)
    V.capi.check(V.lib().vlg_wtsa_search_batch(lazy._h, lq._h, 0, ws._h, C.byref(h)))
    res = V.SearchResult(h, lq.ks)
    assert res.summary["n_matches"] > 1000
    with pytest.raises(V.VlgError):
        res.fetch32()                                                       # (the positions are 8 bytes wide)
    _check(V, res, starts, n, "wtsa", docs)
    _check(V, lazy.search(qs, max_matches=5, begin=100, end=2500), starts, n, "wtsa window", docs)


# ---- 5. several pieces -----------------------------------------------------------------------------------------------------------
def test_several_pieces(V):
    """the batch of test_several_super_chunks_and_join_chunks under its small workspace: more chunks, the same listing"""
    from vlg_matching_amd.index import Workspace
    text = dna_text(50_000, 7, probs=(0.7, 0.1, 0.1, 0.1)).tobytes()
    n = len(text)
    rng = np.random.default_rng(50)
    qs = _random_queries(text, rng, 300, kmax=4, mmax=4)
    fields = [V.parse_query(q) for q in qs]
    pairs = []
    for j in range(len(qs)):
        for _ in range(3):
            B = int(rng.integers(0, n - 100))
            pairs.append((j, B, B + int(rng.integers(1, 6000))))
        pairs.append((j, 0, U64))
    big = ([b"A"] * 64, [1] * 63, [6] * 63, 1)
    batch = _batch(V, [fields[j] for j, _, _ in pairs] + [big])
    batch.set_windows([B for _, B, _ in pairs] + [20_000], [E for _, _, E in pairs] + [20_600])
    starts = list(range(0, n, 1000))
    docs = V.Documents.from_starts(starts, n)
    idx = V.VlgIndex.build(text)
    ref = idx.search(batch)
    res = idx.search(batch, workspace=Workspace(48 << 20))
    assert res.summary["n_chunks"] > ref.summary["n_chunks"] and res.summary["n_matches"] == ref.summary["n_matches"] > 10_000
    want = _check(V, ref, starts, n, "one workspace", docs)
    got = _check(V, res, starts, n, "small workspace", docs)
    assert [x.tolist() for x in got] == [x.tolist() for x in want]
    assert (want[0] > 1).sum() > 100                                        # many queries hit several documents


# ---- 6. / 7. what is fetched, what is refused ------------------------------------------------------------------------------------
def test_fetch_takes_any_subset_of_pointers(V):
    text = _doc_text("dna3000")
    res = V.VlgIndex.build(text).search(["AC", "\xfe", "G.{0,4}?T"])
    starts = list(range(0, 3000, 100))
    docs = V.Documents.from_starts(starts, 3000)
    want = _check(V, res, starts, 3000, "subset", docs)
    full = [want[0], want[1], want[2], want[3], want[4]]
    L = V.lib()
    for what in (V.capi.DOCLIST_PAIRS, V.capi.DOCLIST_DF):
        h = C.c_void_p()
        V.capi.check(L.vlg_result_list_documents(res._h, docs._h, what, C.byref(h)))
        nq, npairs = C.c_uint64(), C.c_uint64()
        V.capi.check(L.vlg_doc_listing_info(h, C.byref(nq), None))
        V.capi.check(L.vlg_doc_listing_info(h, None, C.byref(npairs)))
        assert (nq.value, npairs.value) == (3, len(want[2]))
        for mask in range(32):
            bufs = [np.full(max(len(f), 1) + 1, 77, np.uint64) for f in full]
            ptrs = [b.ctypes.data if (mask >> i) & 1 else None for i, b in enumerate(bufs)]
            st = L.vlg_doc_listing_fetch(h, *ptrs)
            if what == V.capi.DOCLIST_DF and mask >> 2:
                assert st == V.capi.E_INVALID and b"VLG_DOCLIST_DF" in L.vlg_last_error()
                continue
            assert st == V.capi.OK, mask
            for i, (b, f) in enumerate(zip(bufs, full)):
                assert b[:len(f)].tolist() == (f.tolist() if (mask >> i) & 1 else [77] * len(f)), (mask, i)
                assert b[len(f):].tolist() == [77] * (len(b) - len(f))      # nothing behind the end
        L.vlg_doc_listing_destroy(h)


def test_refusals_and_the_empty_result(V):
    text = _doc_text("dna3000")
    idx = V.VlgIndex.build(text)
    res = idx.search(["AC", "G.{0,4}?T"])
    docs = V.Documents.from_starts([0, 1500], 3000)
    L = V.lib()
    out = C.c_void_p(7)
    for r, d, what in ((None, docs._h, 1), (res._h, None, 1), (res._h, docs._h, 2), (res._h, docs._h, -1)):
        assert L.vlg_result_list_documents(r, d, what, C.byref(out)) == V.capi.E_INVALID and out.value == 7
    assert L.vlg_result_list_documents(res._h, docs._h, 1, None) == V.capi.E_INVALID
    # documents of a shorter text: some match begins behind it
    first = res.fetch()[2]
    assert int(first.max()) >= 2000
    short = V.Documents.from_starts([0, 1500], 2000)
    for what in (0, 1):
        assert L.vlg_result_list_documents(res._h, short._h, what, C.byref(out)) == V.capi.E_INVALID and out.value == 7
        assert b"text length" in L.vlg_last_error()
    exact = V.Documents.from_starts([0, 1500], int(first.max()) + 1)        # ... and the shortest text that holds them all is fine
    _check(V, res, [0, 1500], int(first.max()) + 1, "exact", exact)
    # a batch without any match: zero pairs, and every fetch works
    none = idx.search(["\xfe", "\xfd.{0,3}?A"])
    assert none.summary["n_matches"] == 0
    for pairs in (True, False):
        l = none.list_documents(docs, pairs=pairs)
        assert (l.n_queries, l.n_pairs) == (2, 0) and l.df.tolist() == [0, 0] and l.offsets.tolist() == [0, 0, 0]
    l = none.list_documents(docs)
    assert len(l.docs) == 0 and len(l.counts) == 0 and len(l.first_match) == 0 and [len(x) for x in l.of(1)] == [0, 0, 0]
    # the listing borrows neither the result nor the documents
    l = res.list_documents(docs)
    want = _runs(*res.fetch()[2:0:-1], [0, 1500])
    del res, docs
    _same(l, want, "after the result has gone")
