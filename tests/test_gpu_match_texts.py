"""Match texts (vlg_result_extract_matches): the text every match of a result matched, with flanks, inside the text or the document of
its first position.  The yardstick needs no reference: text[b:e] sliced in numpy, b and e from result.fetch()'s first positions and
tuples and the rule of include/vlg_hip.h written out naively here.  Every case shows on the CPU that the border it aims at is hit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_documents import CLASS_REGEXPS
from test_gpu_documents import _text as _doc_text
from test_gpu_wtsa_window import _batch, _random_int_queries, _random_queries
from util import dna_text
from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def _arr(text):
    return np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text)


def _last_positions(res, ks):
    """-> (query of every match, p0, pl) from fetch(): pl is the match's last tuple value, p0 where k = 1"""
    counts, off, first, tup = res.fetch()
    ks, c = np.asarray(ks, np.int64), counts.astype(np.int64)
    q_of = np.repeat(np.arange(len(ks)), c)
    p0 = first.astype(np.int64)
    if not res.summary["n_tuple_values"]:
        assert (ks[q_of] == 1).all()
        return q_of, p0, p0
    toff = np.concatenate([[0], np.cumsum(c * ks)])
    i_in_q = np.arange(len(p0)) - off.astype(np.int64)[q_of]
    return q_of, p0, tup.astype(np.int64)[toff[q_of] + i_in_q * ks[q_of] + ks[q_of] - 1]


def _rule(p0, ce, n_text, starts, flank):
    """the rule, naively: -> (b, e, B0, B1); a flank of None reaches further than any text"""
    fl, fr = flank if isinstance(flank, tuple) else (flank, flank)
    fl, fr = (n_text + 1 if f is None else f for f in (fl, fr))
    if starts is None:
        B0, B1 = np.zeros(len(p0), np.int64), np.full(len(p0), n_text, np.int64)
    else:
        B = np.append(np.asarray(starts, np.int64), n_text)
        d = np.searchsorted(B[:-1], p0, "right") - 1
        B0, B1 = B[d], B[d + 1]
    b = p0 - np.minimum(fl, p0 - np.minimum(p0, B0))
    e = ce + np.minimum(fr, np.maximum(B1, ce) - ce)
    return b, e, B0, B1


def _check(V, res, batch, ta, text, mlast, tag, starts=None, docs=None, flank=0, sl=None, max_symbols=0):
    """the texts of the slice `sl` of a result against numpy slices of the text; -> (p0, ce, b, e, B0, B1, MatchTexts) of all matches"""
    t = _arr(text)
    q_of, p0, pl = _last_positions(res, batch.ks)
    ce = pl + np.asarray(mlast, np.int64)[q_of]
    assert len(p0) == 0 or (ce.max() <= len(t) and (ce > p0).all()), tag
    if starts is not None and docs is None:
        docs = V.Documents.from_starts(starts, len(t))
    b, e, B0, B1 = _rule(p0, ce, len(t), starts, flank)
    a, z = (0, len(p0)) if sl is None else sl
    mt = res.extract_matches(batch, ta, flank=flank, documents=docs, matches=sl, max_symbols=max_symbols)
    off, beg, sym = mt.fetch()
    lens = (e - b)[a:z]
    assert (lens > 0).all() and mt.n_matches == z - a and mt.n_symbols == int(lens.sum()), tag
    assert sym.dtype == t.dtype == mt.symbol_dtype and len(beg) == z - a and len(sym) == mt.n_symbols, tag
    assert off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist(), tag
    assert beg.tolist() == b[a:z].tolist(), tag
    want = np.concatenate([t[b[i]:e[i]] for i in range(a, z)] + [np.zeros(0, t.dtype)])
    assert np.array_equal(sym, want), tag
    return p0, ce, b, e, B0, B1, mt


def _mlast(V, regexps):
    return [len(V.parse_query(q.encode("latin-1") if isinstance(q, str) else q)[0][-1]) for q in regexps]


# ---- 1. lane and run borders -----------------------------------------------------------------------------------------------------
ABAB = b"ab" * 9000


def test_lane_and_run_borders(V):
    """"a" stands at 2 e: match e is element e of the only piece; slices of 1 .. 2 R + 1 matches, from match 0 and from off a word"""
    R = V.capi.build_constants()["VLG_DOCLIST_RUN"]
    idx = V.VlgIndex.build(ABAB)
    batch = V.Queries(["a"])
    res = idx.search(batch)
    assert res.fetch()[2].tolist() == list(range(0, 18000, 2)) and 9000 > 4 * R + 37     # more than one workgroup of four runs
    ta = idx.text_access(64)
    for n in (1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1):
        for a in (0, 37):
            _, _, b, e, _, _, mt = _check(V, res, batch, ta, ABAB, [1], (n, a), flank=(1, 2), sl=(a, a + n))
            p = 2 * (a + n - 1)
            assert mt.of(n - 1) == ABAB[max(p - 1, 0):p + 3] and len(mt.of(0)) == (3 if a == 0 else 4)
    _check(V, res, batch, ta, ABAB, [1], "all", flank=0)
    _check(V, res, batch, ta, ABAB, [1], "docs", starts=list(range(0, 18000, 2 * R - 2)), flank=(None, None))


def _child(env_extra, k, at_least):
    env = dict(os.environ, **env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_match_texts.py", "-k", k],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= at_least, tail


def test_small_variant_runs_the_border_cases():
    """VLG_DOCLIST_RUN = 192: the same cases in a child pytest that loads the `small` build -- runs of three steps"""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_DOCLIST_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    _child({"VLG_HIP_LIBRARY": lib}, "lane_and_run_borders or query_borders or paging", 3)


# ---- 2. query borders ------------------------------------------------------------------------------------------------------------
def _border_batch():
    """-> (text, regexps): many queries of one to three matches (several end inside one step of 64), runs of more than 64 empty
    queries at the front, in the middle and at the end, queries with hundreds of matches between them, k = 1, 2, 3 and 5 mixed"""
    text = dna_text(5000, 23).tobytes()
    rng = np.random.default_rng(5)
    empty = ["\xfe", "\xfd.{0,3}?A", "A.{0,3}?\xfc.{0,3}?C"]

    def planted(k):
        p = int(rng.integers(0, len(text) - 60))
        q = text[p:p + 3].decode()
        for j in range(1, k):
            q += ".{0,9}?" + text[p + 8 * j:p + 8 * j + 2].decode()
        return q
    qs = [empty[i % 3] for i in range(150)]
    qs += [text[p:p + 7].decode() for p in rng.integers(0, len(text) - 7, 90)]
    qs += ["A", "C.{0,5}?G"]
    qs += [planted(int(k)) for k in rng.choice([1, 2, 3, 5], 120)]
    qs += [empty[i % 3] for i in range(200)]
    qs += ["GT", "T.{1,4}?A.{0,6}?C"]
    qs += [planted(5) for _ in range(70)]
    qs += [empty[i % 3] for i in range(70)]
    return text, qs


def test_query_borders(V):
    text, qs = _border_batch()
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    res = idx.search(batch)
    counts, off, _, _ = res.fetch()
    M = int(off[-1])
    ks = batch.ks
    assert {1, 2, 3, 5} <= set(ks[counts > 0].tolist())
    borders = np.bincount((off[1:-1][counts[1:] > 0] // 64).astype(np.int64), minlength=M // 64 + 1)   # first matches of queries, per step
    assert (borders >= 8).sum() >= 3 and (borders == 0).sum() >= 10 and counts.max() > 1000
    assert (counts[:150] == 0).all() and (counts[-70:] == 0).all() and M > 3000
    ta = idx.text_access(16)
    ml = _mlast(V, qs)
    _check(V, res, batch, ta, text, ml, "core")
    _check(V, res, batch, ta, text, ml, "flanks", flank=(5, 7))
    _check(V, res, batch, ta, text, ml, "docs", starts=list(range(0, 5000, 100)), flank=(5, 7))
    _check(V, res, batch, ta, text, ml, "off a word", flank=(2, 0), sl=(29, M - 3))


# ---- 3. flanks and bounds --------------------------------------------------------------------------------------------------------
def test_flanks_and_bounds(V):
    text = _doc_text("dna3000")
    qs = [text[:3].decode(), text[-4:].decode(), "AC", "G.{0,4}?T", text[:2].decode() + ".{2996,2996}?" + text[-2:].decode()]
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    res = idx.search(batch)
    ta = idx.text_access(64)
    ml = _mlast(V, qs)
    for flank in (0, (5, 7), None, (None, 0), (3, None), 1, 3001, (0, 1)):
        p0, ce, b, e, _, _, mt = _check(V, res, batch, ta, text, ml, flank, flank=flank)
        assert (p0 == 0).any() and (ce == 3000).any() and ((p0 == 0) & (ce == 3000)).any()      # the whole text is a match, too
        if flank is None:
            assert (b == 0).all() and (e == 3000).all() and mt.of(0) == text
        if flank == 0:
            assert mt.of(0) == text[:3] and (b == p0).all() and (e == ce).all()


# ---- 4. documents and fences -----------------------------------------------------------------------------------------------------
def test_documents_and_fences(V):
    """more than 64 and more than 64 * 64 documents of one and two symbols; a boundary exactly at p0, inside a flank, at ce, and a
    core that crosses (the search ran without documents)"""
    text = dna_text(20_000, 17).tobytes()
    n = len(text)
    qs = ["AC", "GT.{0,6}?A", "T", "CCG"]
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    res = idx.search(batch)
    ta = idx.text_access(64)
    ml = _mlast(V, qs)
    first = res.fetch()[2].astype(np.int64)
    assert len(first) > 4096
    rng = np.random.default_rng(9)
    ac = [int(first[i]) for i in (100, 300, 500, 700, 900)]                     # matches of "AC", far from one another
    assert res.fetch()[1][1] > 900 and min(np.diff(ac)) > 40
    aimed = {0, ac[0], ac[1] - 3, ac[2] + 2, ac[3] + 5, ac[4] + 1}              # at p0, inside the left flank, at ce, inside the right flank, inside the core

    def scattered(k):
        """k random starts, none within 8 symbols of an aimed one"""
        pool = [int(x) for x in rng.permutation(np.arange(1, n))[:k]]
        return sorted(aimed | {x for x in pool if min(abs(x - y) for y in aimed) > 8})
    sets = {
        "single": [0],
        "ones": list(range(n)),                                                 # 20 000 documents of one symbol
        "twos": list(range(0, n, 2)),                                           # 10 000 of two
        "few": sorted(set(range(0, 100)) | set(range(100, 240, 2)) | {5000, 5001, 5003, 12_000}),   # 100 + 70 small ones among large ones
        "random65": scattered(70),
        "random4097": scattered(4200),
    }
    assert len(sets["few"]) > 64 and len(sets["random65"]) > 64 and len(sets["random4097"]) > 64 * 64
    for name, starts in sets.items():
        for flank in ((5, 7), None):
            p0, ce, b, e, B0, B1, _ = _check(V, res, batch, ta, text, ml, (name, flank), starts=starts, flank=flank)
            if name == "single":
                continue
            assert (B0 == p0).any() and (B1 == ce).any() and (B1 < ce).any()    # a boundary at p0, at ce, inside a core
            assert (e[B1 <= ce] == ce[B1 <= ce]).all()                          # ... which keeps itself and gets no right flank
            if flank is not None and name != "ones":
                assert ((p0 - B0 > 0) & (p0 - B0 < 5)).any() and ((B1 - ce > 0) & (B1 - ce < 7)).any()     # a boundary inside either flank
            else:
                assert (b == B0).all() and (e == np.maximum(B1, ce)).all()


# ---- 5. every road ---------------------------------------------------------------------------------------------------------------
def _mismatches(V, regexps, res, batch, mt):
    """per match and sub-pattern, the positions of the extracted text that are no member of the query's class -> (worst per
    sub-pattern of the batch, in batch order)"""
    off, beg, sym = mt.fetch()
    worst, g, s0 = [], 0, 0
    for qi, r in enumerate(regexps):
        subs = [np.unpackbits(np.asarray(rows, np.uint8), axis=1, bitorder="little") for rows in V.parse_class_query(r)[0]]
        w = [0] * len(subs)
        for t in res.tuples(qi).tolist():
            txt = sym[int(off[g]):int(off[g + 1])]
            for j, (x, bits) in enumerate(zip(t, subs)):
                o = x - int(beg[g])
                w[j] = max(w[j], int(sum(1 - bits[i, txt[o + i]] for i in range(len(bits)))))
            g += 1
        worst += w
        s0 += len(subs)
    assert g == mt.n_matches
    return worst


def test_every_road(V):
    import torch
    from vlg_matching_amd.index import Workspace, join_batch
    text = _doc_text("dna3000")
    n = len(text)
    rng = np.random.default_rng(21)
    starts = sorted({0} | {int(x) for x in rng.integers(1, n, 75)})
    qs = _random_queries(text, rng, 48, kmax=4, mmax=2, gapmax=30, gaplo=4)
    ml = _mlast(V, qs)
    docs = V.Documents.from_starts(starts, n)
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    # a plain search: every text-access density; the rrr index; SA densities 1 and 7
    res = idx.search(batch)
    assert res.summary["n_matches"] > 1000
    for d in (1, 3, 64, n + 5):
        _check(V, res, batch, idx.text_access(d), text, ml, ("plain", d), flank=(5, 7))
        _check(V, res, batch, idx.text_access(d), text, ml, ("plain docs", d), starts=starts, docs=docs, flank=(5, 7))
    ta = idx.text_access(64)
    rrr = idx.compress()
    _check(V, rrr.search(batch), batch, rrr.text_access(3), text, ml, "rrr", starts=starts, docs=docs, flank=(5, 7))
    _check(V, res, batch, rrr.text_access(64), text, ml, "rrr text, plain result", flank=2)
    for dens in (1, 7):
        ix = V.VlgIndex.build(text, dens=dens)
        _check(V, ix.search(batch), batch, ix.text_access(3), text, ml, ("dens", dens), starts=starts, docs=docs, flank=(5, 7))
    # a document-bounded search with the same handle: no core crosses
    batch.set_documents(docs)
    p0, ce, b, e, B0, B1, _ = _check(V, idx.search(batch), batch, ta, text, ml, "bounded", starts=starts, docs=docs, flank=(5, 7))
    assert (ce <= B1).all() and (B0 <= b).all() and (e <= B1).all()
    batch.set_documents(None)
    # a windowed batch
    batch.set_windows(rng.integers(0, n // 2, len(qs)), rng.integers(n // 2, n, len(qs)))
    res_w = idx.search(batch)
    assert 0 < res_w.summary["n_matches"] < res.summary["n_matches"]
    _check(V, res_w, batch, ta, text, ml, "windows", starts=starts, docs=docs, flank=(5, 7))
    batch.set_windows(None, None)
    # classes: the text at a class position is a member of the class; budgets: at most k positions of a sub-pattern are not
    q = V.Queries.from_classes(CLASS_REGEXPS)
    cml = [len(V.parse_class_query(r)[0][-1]) for r in CLASS_REGEXPS]
    res_c = idx.search(q)
    mt = _check(V, res_c, q, ta, text, cml, "classes", starts=starts, docs=docs, flank=(5, 7))[-1]
    assert res_c.summary["n_matches"] > 100 and max(_mismatches(V, CLASS_REGEXPS, res_c, q, mt)) == 0
    nsub = sum(len(V.parse_class_query(r)[0]) for r in CLASS_REGEXPS)
    budgets = [int(x) for x in rng.integers(0, 3, nsub)]
    q.set_mismatches(budgets)
    res_b = idx.search(q)
    mt = _check(V, res_b, q, ta, text, cml, "budgets", flank=(5, 7))[-1]
    worst = _mismatches(V, CLASS_REGEXPS, res_b, q, mt)
    assert res_b.summary["n_matches"] > res_c.summary["n_matches"] and all(w <= k for w, k in zip(worst, budgets)) and max(worst) > 0
    # an integer index: uint32 symbols, the original ones
    itext = _doc_text("ints")
    iqs, fields = _random_int_queries(itext, rng, 32, mmax=2, gapmax=30, gaplo=4)
    istarts = sorted({0} | {int(x) for x in rng.integers(1, len(itext), 40)})
    iidx = V.VlgIndex.build_int(itext)
    ib = V.index.Queries.from_int(iqs)
    ires = iidx.search(ib)
    assert ires.summary["n_matches"] > 200 and int(itext.max()) == 2 ** 32 - 1
    iml = [len(f[0][-1]) for f in fields]
    for d in (1, 64):
        mt = _check(V, ires, ib, iidx.text_access(d), itext, iml, ("int", d), starts=istarts, flank=(5, 7))[-1]
    assert isinstance(mt.of(0), np.ndarray) and mt.of(0).dtype == np.uint32
    _check(V, ires, ib, iidx.compress().text_access(3), itext, iml, "int rrr", flank=None, sl=(3, 40))
    # vlg_join_batch: caller-built lists, 8-byte positions; the batch gives the shape and the length of the last sub-pattern
    big = dna_text(50_002, 3).tobytes()
    a, b = np.arange(0, 50_000, 5, dtype=np.uint64), np.arange(2, 50_000, 5, dtype=np.uint64)
    lists = torch.from_numpy(np.concatenate([a, b, a[:100]]).view(np.int64)).cuda()
    jres = join_batch(lists.data_ptr(), [0, len(a), len(a) + len(b), len(a) + len(b) + 100], [0, 2, 3], [0, 2, 0], [0, 2, 0], [1, 1], Workspace())
    assert jres.counts.tolist() == [len(a), 100]
    jb = V.index.Queries.from_arrays([[b"x", b"yy"], [b"zzz"]], [[2], []], [[2], []], [1, 1])
    bidx = V.VlgIndex.build(big)
    p0, ce, _, _, _, _, _ = _check(V, jres, jb, bidx.text_access(64), big, [2, 3], "join", starts=list(range(0, 50_000, 777)), flank=(5, 7))
    assert (ce - p0)[:len(a)].tolist() == [4] * len(a) and (ce - p0)[len(a):].tolist() == [3] * 100
    # the lazy index, both entry points (8-byte positions)
    lazy = V.WtsaIndex(text)
    ws = Workspace()
    h = C.c_void_p()
    V.capi.check(V.lib().vlg_wtsa_search_batch(lazy._h, batch._h, 0, ws._h, C.byref(h)))
    lres = V.SearchResult(h, batch.ks)
    assert lres.summary["n_matches"] > 1000
    with pytest.raises(V.VlgError):
        lres.fetch32()                                                      # (the positions are 8 bytes wide)
    _check(V, lres, batch, ta, text, ml, "wtsa", starts=starts, docs=docs, flank=(5, 7))
    _check(V, lazy.search(batch, max_matches=5, begin=100, end=2500), batch, ta, text, ml, "wtsa window", flank=(5, 7))


def test_several_pieces_and_results_without_tuples(V):
    """a small workspace cuts the result into pieces: slices that begin and end inside pieces; "tuples" = 0 is accepted where every
    query with a match in the slice has k = 1"""
    from vlg_matching_amd.index import Workspace
    text = dna_text(50_000, 7, probs=(0.7, 0.1, 0.1, 0.1)).tobytes()
    n = len(text)
    rng = np.random.default_rng(50)
    qs = _random_queries(text, rng, 300, kmax=4, mmax=4)          # (the batch of the listing's test_several_pieces)
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
    ml = [len(fields[j][0][-1]) for j, _, _ in pairs] + [1]
    idx = V.VlgIndex.build(text)
    ref = idx.search(batch)
    res = idx.search(batch, workspace=Workspace(48 << 20))
    M = res.summary["n_matches"]
    assert res.summary["n_chunks"] > max(ref.summary["n_chunks"], 2) and M == ref.summary["n_matches"] > 10_000
    ta = idx.text_access(64)
    starts = list(range(0, 50_000, 1000))
    _check(V, res, batch, ta, text, ml, "pieces", starts=starts, flank=(5, 7))
    _check(V, res, batch, ta, text, ml, "inside pieces", flank=(5, 7), sl=(M // 7, M - M // 5))
    # no tuples: k = 1 everywhere is fine, ...
    ws = Workspace()
    ws.set_option("tuples", 0)
    ones = V.Queries(["AC", "\xfe", "GGT", "T"])
    r1 = idx.search(ones, workspace=ws)
    assert r1.summary["n_matches"] > 1000 and r1.summary["n_tuple_values"] == 0
    _check(V, r1, ones, ta, text, [2, 1, 3, 1], "no tuples", starts=starts, flank=(5, 7))
    # ... a k = 2 query with a match in the slice is refused, and a slice that holds none of its matches is not
    mixed = V.Queries(["AC", "G.{0,4}?T", "T"])
    r2 = idx.search(mixed, workspace=ws)
    off = r2.fetch()[1]
    assert r2.summary["n_tuple_values"] == 0 and off[1] < off[2] < off[3]
    for sl in (None, (int(off[1]) - 1, int(off[1]) + 1), (int(off[2]) - 1, int(off[2]) + 1)):
        with pytest.raises(V.VlgError) as err:
            r2.extract_matches(mixed, ta, matches=sl)
        assert err.value.status == V.capi.E_INVALID and "tuples" in str(err.value)
    for sl in ((0, int(off[1])), (int(off[2]), int(off[3]))):
        mt = r2.extract_matches(mixed, ta, matches=sl)
        first = r2.fetch()[2][sl[0]:sl[1]]
        assert mt.fetch()[1].tolist() == first.tolist() and set(mt.fetch()[2].tobytes()) == ({65, 67} if sl[0] == 0 else {84})


# ---- 6. paging -------------------------------------------------------------------------------------------------------------------
def test_paging(V):
    """slices of 1, 7 and R + 3 matches, concatenated, are the whole; the slice of one query comes from the offsets of fetch()"""
    R = V.capi.build_constants()["VLG_DOCLIST_RUN"]
    text = dna_text(20_000, 17).tobytes()
    qs = ["AC", "GT.{0,6}?A", "\xfe", "T", "CCG"]
    ml = _mlast(V, qs)
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    res = idx.search(batch)
    ta = idx.text_access(64)
    starts = list(range(0, 20_000, 50))
    docs = V.Documents.from_starts(starts, 20_000)
    _, off, _, _ = res.fetch()
    M = int(off[-1])
    assert M > 2 * (R + 3) + 8
    whole = _check(V, res, batch, ta, text, ml, "whole", starts=starts, docs=docs, flank=(5, 7))[-1].fetch()
    for step in (1, 7, R + 3):
        lo = 0 if step > 7 else M - 40 * step                                 # (the small slices: the last forty of them)
        parts = [res.extract_matches(batch, ta, flank=(5, 7), documents=docs, matches=(a, min(a + step, M))).fetch() for a in range(lo, M, step)]
        assert np.concatenate([p[1] for p in parts]).tolist() == whole[1][lo:].tolist()
        assert np.concatenate([p[2] for p in parts]).tobytes() == whole[2][int(whole[0][lo]):].tobytes()
        assert [int(p[0][-1]) for p in parts] == [int(whole[0][min(a + step, M)] - whole[0][a]) for a in range(lo, M, step)]
    for q in range(len(qs)):
        sl = (int(off[q]), int(off[q + 1]))
        _check(V, res, batch, ta, text, ml, ("query", q), starts=starts, docs=docs, flank=(5, 7), sl=sl)
    mt = res.extract_matches(batch, ta, matches=(int(off[3]), None))          # None: to the last match
    assert mt.n_matches == M - int(off[3])


# ---- 7. / 8. what is fetched, what is refused ------------------------------------------------------------------------------------
def test_fetch_takes_any_subset_of_pointers(V):
    text = _doc_text("dna3000")
    idx = V.VlgIndex.build(text)
    batch = V.Queries(["AC", "\xfe", "G.{0,4}?T"])
    res = idx.search(batch)
    ta = idx.text_access(64)
    full = _check(V, res, batch, ta, text, [2, 1, 1], "subset", flank=(5, 7))[-1].fetch()
    L = V.lib()
    h = C.c_void_p()
    V.capi.check(L.vlg_result_extract_matches(res._h, batch._h, ta._h, None, 5, 7, 0, U64, 0, C.byref(h)))
    nm, ns, sb = C.c_uint64(), C.c_uint64(), C.c_uint32()
    V.capi.check(L.vlg_match_texts_info(h, C.byref(nm), None, None))
    V.capi.check(L.vlg_match_texts_info(h, None, C.byref(ns), C.byref(sb)))
    assert (nm.value, ns.value, sb.value) == (len(full[1]), len(full[2]), 1)
    for mask in range(8):
        bufs = [np.full(len(f) + 1, 77, f.dtype) for f in full]
        ptrs = [b.ctypes.data if (mask >> i) & 1 else None for i, b in enumerate(bufs)]
        assert L.vlg_match_texts_fetch(h, *ptrs) == V.capi.OK, mask
        for i, (b, f) in enumerate(zip(bufs, full)):
            assert b[:len(f)].tolist() == (f.tolist() if (mask >> i) & 1 else [77] * len(f)), (mask, i)
            assert b[len(f):].tolist() == [77]                                  # nothing behind the end
    L.vlg_match_texts_destroy(h)


def test_refusals_and_the_empty_result(V):
    text = _doc_text("dna3000")
    idx = V.VlgIndex.build(text)
    qs = ["AC", "G.{0,4}?T"]
    batch = V.Queries(qs)
    res = idx.search(batch)
    ta = idx.text_access(64)
    docs = V.Documents.from_starts([0, 1500], 3000)
    M = res.summary["n_matches"]
    L = V.lib()
    out = C.c_void_p(7)

    def refused(r, q, t, d, begin=0, end=U64, cap=0, status=V.capi.E_INVALID, says=b""):
        st = L.vlg_result_extract_matches(r._h if r else None, q._h if q else None, t._h if t else None, d._h if d else None, 5, 7, begin, end, cap, C.byref(out))
        assert st == status and out.value == 7 and says in L.vlg_last_error(), L.vlg_last_error()
    for r, q, t in ((None, batch, ta), (res, None, ta), (res, batch, None)):
        refused(r, q, t, docs, says=b"null")
    assert L.vlg_result_extract_matches(res._h, batch._h, ta._h, None, 0, 0, 0, U64, 0, None) == V.capi.E_INVALID
    # the slice
    refused(res, batch, ta, docs, begin=5, end=4, says=b"match_begin > match_end")
    refused(res, batch, ta, docs, begin=M + 1, says=b"match_begin > match_end")
    refused(res, batch, ta, docs, end=M + 1, says=b"beyond")
    # queries of another batch: another number of them, another k
    refused(res, V.Queries(["AC"]), ta, docs, says=b"queries")
    refused(res, V.Queries(["AC", "G.{0,4}?T", "T"]), ta, docs, says=b"queries")
    refused(res, V.Queries(["AC", "GT"]), ta, docs, says=b"sub-patterns")
    refused(res, V.Queries(["A.{0,4}?C", "G.{0,4}?T"]), ta, docs, says=b"sub-patterns")
    # the other alphabet, either way
    itext = _doc_text("ints")
    iidx = V.VlgIndex.build_int(itext)
    ita = iidx.text_access(64)
    refused(res, batch, ita, None, says=b"byte batch")
    ib = V.index.Queries.from_int(["1", "2 .{0,4}? 3"])
    ires = iidx.search(ib)
    assert ires.summary["n_matches"] > 0
    refused(ires, ib, ta, None, says=b"integer batch")
    # a text access of a shorter text: some core ends behind it -- counted on the device
    q_of, p0, pl = _last_positions(res, batch.ks)
    behind = int((pl + 1 + (q_of == 0) > 2000).sum())
    short = V.VlgIndex.build(text[:2000])
    assert 0 < behind < M
    refused(res, batch, short.text_access(64), None, says=b"%d match(es)" % behind)
    refused(res, batch, short.text_access(64), V.Documents.from_starts([0, 1500], 2000), says=b"%d match(es)" % behind)
    mt = res.extract_matches(batch, short.text_access(64), matches=(0, int((p0[q_of == 0] + 2 <= 2000).sum())))     # ... the matches in front of it are fine
    assert mt.of(mt.n_matches - 1) == b"AC"
    # documents of another length
    refused(res, batch, ta, V.Documents.from_starts([0, 1500], 2999), says=b"documents of a text of 2999")
    refused(res, batch, ta, V.Documents.from_starts([0, 1500], 3001), says=b"documents of a text of 3001")
    # the cap: one below the total is refused and names both numbers, exactly the total is legal
    total = _check(V, res, batch, ta, text, [2, 1], "total", starts=[0, 1500], docs=docs, flank=(5, 7))[-1].n_symbols
    refused(res, batch, ta, docs, cap=total - 1, status=V.capi.E_WORKSPACE, says=b"%d symbols, max_symbols is %d" % (total, total - 1))
    _check(V, res, batch, ta, text, [2, 1], "cap", starts=[0, 1500], docs=docs, flank=(5, 7), max_symbols=total)
    with pytest.raises(V.VlgError) as err:
        res.extract_matches(batch, ta, flank=(5, 7), documents=docs, max_symbols=total - 1)
    assert err.value.status == V.capi.E_WORKSPACE
    # an empty slice, a batch without any match: zero texts, and every fetch works
    none_b = V.Queries(["\xfe", "\xfd.{0,3}?A"])
    none = idx.search(none_b)
    assert none.summary["n_matches"] == 0
    for mt in (none.extract_matches(none_b, ta, flank=3, documents=docs), res.extract_matches(batch, ta, matches=(4, 4)),
               res.extract_matches(batch, ta, matches=(M, None))):
        off, beg, sym = mt.fetch()
        assert (mt.n_matches, mt.n_symbols) == (0, 0) and off.tolist() == [0] and len(beg) == 0 and len(sym) == 0 and mt.symbol_dtype == np.uint8
    # the handle borrows nothing
    mt = res.extract_matches(batch, ta, flank=(5, 7), documents=docs)
    want = _check(V, res, batch, ta, text, [2, 1], "kept", starts=[0, 1500], docs=docs, flank=(5, 7))[-1].fetch()
    del res, batch, ta, docs, idx
    assert [x.tolist() for x in mt.fetch()] == [x.tolist() for x in want]


# ---- 9. the unchanged path -------------------------------------------------------------------------------------------------------
def test_a_search_launches_what_it_launched_before(V):
    """the launch counts of every kernel class of a search are the same before and after an extract_matches call on its result"""
    from vlg_matching_amd.index import Workspace
    text = dna_text(20_000, 17).tobytes()
    qs = ["AC", "GT.{0,6}?A", "T", "CCG.{1,9}?A.{0,3}?T"]
    idx = V.VlgIndex.build(text)
    batch = V.Queries(qs)
    ws = Workspace()
    ws.profile(True)
    launches = lambda: {k: v["launches"] for k, v in ws.kernel_stats().items()}
    res = idx.search(batch, workspace=ws)
    one = launches()
    assert sum(one.values()) > 5
    ta = idx.text_access(64)
    mt = res.extract_matches(batch, ta, flank=(5, 7), documents=V.Documents.from_starts(list(range(0, 20_000, 64)), 20_000))
    assert mt.n_matches == res.summary["n_matches"] > 4096 and launches() == one
    idx.search(batch, workspace=ws)
    two = launches()
    assert {k: two[k] - one[k] for k in one} == one                             # the search after it launched what the one before did
