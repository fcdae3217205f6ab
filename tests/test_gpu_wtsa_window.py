"""The paper's index searched inside text windows and page by page (vlg_wtsa_search_window_batch, vlg_result_next_positions), and
wt_int::range_search_2d as a batched pair (vlg_wtsa_range_count_batch / _report_batch).  The yardstick is tests/vlg_brute.py: query j on
the window [B, E) has exactly the matches of the same query on the stand-alone text text[B:E], with B added to every position."""
import ctypes as C

import numpy as np
import pytest

from util import I63, array_queries, dna_text, naive_sa
from vlg_brute import lazy_matches, occurrences

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _random_queries(text, rng, nq, kmax=4, mmax=4, gapmax=60, gaplo=20):
    qs = []
    for _ in range(nq):
        k = int(rng.integers(1, kmax + 1))
        subs = [text[s:s + int(rng.integers(1, mmax + 1))] for s in rng.integers(0, max(len(text) - mmax - 1, 1), k)]
        q = subs[0].decode("latin-1")
        for sp in subs[1:]:
            a = int(rng.integers(0, gaplo))
            q += ".{%d,%d}?%s" % (a, a + int(rng.integers(0, gapmax)), sp.decode("latin-1"))
        qs.append(q)
    return qs


def _random_int_queries(text, rng, nq, kmax=4, mmax=3, gapmax=40, gaplo=10):
    """the same for an integer text: (regexps of whitespace-separated decimals, their fields)"""
    qs, fields = [], []
    for _ in range(nq):
        k = int(rng.integers(1, kmax + 1))
        subs = [text[s:s + int(rng.integers(1, mmax + 1))] for s in rng.integers(0, len(text) - mmax - 1, k)]
        gaps = [(int(a), int(a) + int(rng.integers(0, gapmax))) for a in rng.integers(0, gaplo, k - 1)]
        q = " ".join(str(int(x)) for x in subs[0])
        for (a, b), sub in zip(gaps, subs[1:]):
            q += " .{%d,%d}? " % (a, b) + " ".join(str(int(x)) for x in sub)
        qs.append(q)
        fields.append((subs, [a + len(s) for (a, _), s in zip(gaps, subs)], [b + len(s) for (_, b), s in zip(gaps, subs)], len(subs[-1])))
    return qs, fields


def _batch(V, fields):
    return V.index.Queries.from_arrays([f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields], [f[3] for f in fields])


def _brute_window(text, f, B, E, cap=None):
    """the matches of the query with fields f on text[B:E) (E clamped to the text, B to E), shifted by B"""
    subs, lo, hi, end_len = f
    E = min(E, len(text))
    B = min(B, E)
    lists = [[int(v) + B for v in occurrences(text[B:E], s)] for s in subs]
    return lazy_matches(lists, lo, hi, end_len, cap)


def _windows_of(text, f, rng, n_random=32):
    """the windows one query is asked on: the fixed edges, the ones that cut through occurrences of its sub-patterns, random ones"""
    n = len(text)
    subs = f[0]
    w = [(0, n), (0, 0), (n // 2, n // 2), (n, n), (0, U64), (n // 3, U64), (n, U64), (n + 7, U64), (0, n + 1), (1, n - 1)]
    for i in sorted({0, len(subs) - 1, len(subs) // 2}):
        m = len(subs[i])
        occ = occurrences(text, subs[i])
        if not len(occ):
            continue
        p = int(occ[len(occ) // 2])
        w += [(p, n), (p + 1, n), (max(p, 1) - 1, n)]                                   # begin on / behind / before an occurrence start
        w += [(0, max(p + m - 2, 0)), (0, p + m - 1), (0, p + m)]                       # E - m + 1 one before / on / one behind it
        w += [(p, p + m - 1), (p, p + m), (p, p + m + 1)]                               # one symbol too short for it; exactly it
        if i == 0:
            w += [(p + 1, min(p + 200, n))]
        if i == len(subs) - 1:
            w += [(max(p - 200, 0), p + m - 1), (max(p - 200, 0), p + m)]
    for _ in range(n_random):
        a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        w.append((a, b))
    return w


def _check(res, want, tuples=True):
    flat = [t for w in want for t in w]
    assert [int(c) for c in res.counts] == [len(w) for w in want]
    assert res.summary["n_matches"] == len(flat)
    assert res.summary["checksum"] == sum(t[0] for t in flat) % (1 << 64)
    assert res.summary["n_tuple_values"] == (sum(len(t) for t in flat) if tuples else 0)
    counts, off, first, tup = res.fetch()
    assert first.tolist() == [t[0] for t in flat]
    if tuples:
        assert tup.tolist() == [x for t in flat for x in t]


TEXTS = ["dna223", "dna224", "dna225", "dna3000", "abab", "ints"]


def _text(name):
    if name.startswith("dna"):
        return dna_text(int(name[3:]), 31).tobytes()
    if name == "abab":
        return b"ab" * 600 + b"aab" * 100
    rng = np.random.default_rng(12)
    vocab = np.array([0, 1, 2, 7, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.uint64)
    return vocab[rng.choice(len(vocab), 1500)].astype(np.uint32)


@pytest.mark.parametrize("name", TEXTS)
def test_window_edges_against_brute_force(V, monkeypatch, name):
    """Every query of a batch on its own windows (one batch entry per (query, window) pair): the whole text, begin == end, a window one
    symbol shorter than a sub-pattern, windows whose begin / end cut through an occurrence of the first / middle / last sub-pattern,
    E - m + 1 on, before and behind an occurrence start, end = 2^64 - 1, begin = the text's length and beyond, 32 random windows --
    counts, first positions, tuples, n_matches and checksum; with and without tuples; one wavefront and one lane per query; and a
    cap.  Texts around the super-block border of a level (224 bits), a periodic text, integers with symbol 0 and symbols >= 2^31;
    parsed batches, and for two byte texts caller-built ones (lo down to 0, any end_len)."""
    from vlg_matching_amd.index import Workspace
    text = _text(name)
    rng = np.random.default_rng(len(text))
    idx = V.WtsaIndex(text)
    if name == "ints":
        qs, fields = _random_int_queries(text, rng, 60)
        batches = [(lambda reps: idx.queries(reps), qs, fields)]
    else:
        qs = _random_queries(text, rng, 60, mmax=4 if len(text) > 1000 else 3)
        fields = [V.parse_query(q) for q in qs]
        batches = [(lambda reps: V.index.Queries(reps), qs, fields)]
        if name in ("dna3000", "abab"):
            af = [f for f in array_queries(text, 5, n=40) if len(f[0]) <= 9][:16]
            batches.append((lambda reps: _batch(V, reps), af, af))
    first_only = Workspace()
    first_only.set_option("tuples", 0)
    n_win = 0
    for make, reps, fields in batches:
        pairs = [(j, B, E) for j, f in enumerate(fields) for (B, E) in _windows_of(text, f, rng, 32 if len(fields) == 60 else 8)]
        n_win += len(pairs)
        batch = make([reps[j] for j, _, _ in pairs])
        begin = np.array([B for _, B, _ in pairs], dtype=np.uint64)
        end = np.array([E for _, _, E in pairs], dtype=np.uint64)
        want = [_brute_window(text, fields[j], B, E) for j, B, E in pairs]
        assert sum(1 for w in want if w) > len(want) // 8 and any(len(w) > 3 for w in want)
        _check(idx.search(batch, begin=begin, end=end), want)
        _check(idx.search(batch, begin=begin, end=end, workspace=first_only), want, tuples=False)
        _check(idx.search(batch, begin=begin, end=end, max_matches=2), [w[:2] for w in want])
        monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
        _check(idx.search(batch, begin=begin, end=end), want)
        _check(idx.search(batch, begin=begin, end=end, max_matches=2, workspace=first_only), [w[:2] for w in want], tuples=False)
        monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")
    assert n_win > 2000


def test_no_window_is_the_search_of_before(V):
    """NULL / NULL (and begin 0, end = the text's length or beyond) == vlg_wtsa_search_batch on the same batch, field for field"""
    text = dna_text(3000, 31).tobytes()
    rng = np.random.default_rng(9)
    qs = _random_queries(text, rng, 70) + ["\xfe", "A"]
    idx = V.WtsaIndex(text)
    batch = V.index.Queries(qs)
    ws = V.index.Workspace()
    for cap in (0, 1, 5):
        h = C.c_void_p()
        V.capi.check(V.lib().vlg_wtsa_search_batch(idx._h, batch._h, cap, ws._h, C.byref(h)))
        old = V.SearchResult(h, batch.ks)
        n = len(text)
        for b, e in ((None, None), (0, None), (None, n), (0, n), (0, U64), (np.zeros(len(qs), np.uint64), np.full(len(qs), n + 3, np.uint64))):
            new = idx.search(batch, max_matches=cap, workspace=ws, begin=b, end=e)
            assert new.summary == old.summary
            for x, y in zip(new.fetch(), old.fetch()):
                assert x.tolist() == y.tolist()
            assert new.next_positions().tolist() == old.next_positions().tolist()
        if cap == 0:
            assert (old.next_positions() == np.uint64(U64)).all()


def _planted(n_piv, r):
    """the text of test_pivot_list_is_walked_64_elements_at_a_time: a run of `a`, `b` every 40 symbols (the pivot list), eleven `c` behind
    every `b` outside the gap window, and one `c` three symbols before and behind the r-th `b`"""
    t = bytearray(b"a" * (40 * n_piv + 60))
    b_at = [20 + 40 * i for i in range(n_piv)]
    for p in b_at:
        t[p] = ord("b")
        for o in range(20, 31):
            t[p + o] = ord("c")
    t[b_at[r] + 3] = t[b_at[r] - 3] = ord("c")
    return bytes(t), b_at


@pytest.mark.parametrize("rlo", [63, 64, 65])
def test_pivot_is_scanned_inside_the_window(V, rlo):
    """130 pivot elements; the window begins so that the pivot's first rank inside is 63, 64, 65 and ends so that 1, 63 or 64 of its
    elements lie inside -- the 64-at-a-time scan of the pivot starts at rlo and stops at rhi.  The only `b` with partners stands first
    or last inside the window (the match is known by construction), or its partner `c` lies just outside the window while the `b`
    is inside: that one must not count."""
    n_piv = 130
    qs = ["b.{1,3}?c", "c.{1,3}?b", "a.{1,3}?b.{1,3}?c", ([b"b", b"c"], [3], [3], I63), ([b"c", b"b"], [0], [3], 1)]
    for span in (1, 63, 64):
        rhi = rlo + span
        for r in sorted({rlo, rhi - 1}):
            text, b_at = _planted(n_piv, r)
            fields = [V.parse_query(q) if isinstance(q, str) else q for q in qs]
            idx = V.WtsaIndex(text)
            x = b_at[r]
            inside = [[[x, x + 3]], [[x - 3, x]], [[x - 4, x, x + 3]], [[x, x + 3]], [[x - 3, x]]]
            wins, want = [], []
            B, E = b_at[rlo] - 10, b_at[rhi - 1] + 35                                   # pivot ranks [rlo, rhi) and all their `c`
            assert [p for p in b_at if B <= p and p + 1 <= E] == b_at[rlo:rhi]
            wins.append((B, E)); want.append(inside)
            wins.append((x - 2, E)); want.append([inside[0], [], [[x - 2, x, x + 3]], inside[3], []])   # the `c` before x is outside, x is inside
            wins.append((B, x + 3)); want.append([[], inside[1], [], [], inside[4]])    # the `c` behind x is outside, x is inside
            wins.append((x - 4, x + 4)); want.append(inside)                            # exactly the longest match
            wins.append((b_at[r] + 1, E)); want.append([[]] * 5)                        # the pivot element itself is cut away
            if r + 1 < n_piv and r > 0:
                wins.append((b_at[r - 1], b_at[r] - 4)); want.append([[]] * 5)         # its partners exist only outside: nothing
            for (B, E), w in zip(wins, want):
                assert [_brute_window(text, f, B, E) for f in fields] == w, (rlo, span, r, B, E)
                for cap in (0, 1):
                    res = idx.search(_batch(V, fields), max_matches=cap, begin=B, end=E)
                    assert [res.tuples(i).tolist() for i in range(5)] == w, (rlo, span, r, B, E, cap)
            assert occurrences(text, b"b").tolist() == b_at


def test_deep_pointer_machine_inside_a_window(V, monkeypatch):
    """k = 33 on a run of `a` with a window in the middle: pointers at depth >= 32 are not tracked in the `have` mask and are recomputed;
    the pivot (a longer, rarer sub-pattern) stands at level 0, 32 and nowhere"""
    text = b"a" * 400
    chain = ".{0,2}?".join(["a"] * 33)
    fields = [V.parse_query(chain),
              V.parse_query(".{0,2}?".join(["a" * 120] + ["a"] * 32)),
              V.parse_query(".{0,2}?".join(["a"] * 32 + ["a" * 120])),
              ([b"a"] * 33, [0 if i % 3 else 1 for i in range(32)], [(0 if i % 3 else 1) + i % 4 for i in range(32)], 1)]
    idx = V.WtsaIndex(text)
    wins = [(100, 300), (0, 400), (150, 150 + 33), (150, 150 + 32), (399, 400), (57, 391)]
    pairs = [(j, B, E) for j in range(len(fields)) for B, E in wins]
    batch = _batch(V, [fields[j] for j, _, _ in pairs])
    begin, end = [B for _, B, _ in pairs], [E for _, _, E in pairs]
    want = [_brute_window(text, fields[j], B, E) for j, B, E in pairs]
    assert sum(len(w) for w in want) > 40 and want[0] and want[0][0][0] == 100 and not want[3]
    for lane in (False, True):
        if lane:
            monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
        _check(idx.search(batch, begin=begin, end=end), want)
        _check(idx.search(batch, begin=begin, end=end, max_matches=1), [w[:1] for w in want])
    monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")


def _paged(V, idx, fields, begin, end, page):
    """every query page by page through next_positions, dropping the ones that ran out -> (matches per query, pages per query)"""
    nq = len(fields)
    got, pages = [[] for _ in range(nq)], [0] * nq
    live, at = list(range(nq)), list(begin)
    while live:
        res = idx.search(_batch(V, [fields[j] for j in live]), max_matches=page, begin=[at[j] for j in live], end=[end[j] for j in live])
        nxt = res.next_positions()
        assert len(nxt) == len(live)
        keep = []
        for i, j in enumerate(live):
            t = res.tuples(i).tolist()
            assert len(t) <= page
            got[j] += t
            pages[j] += 1
            if int(nxt[i]) == U64:
                assert len(t) < page                                                    # ran out: a query that fills its page reports a position
            else:
                # stopped at the cap: the position behind the last match (never beyond the window's end)
                assert len(t) == page and int(nxt[i]) == min(t[-1][-1] + fields[j][3], end[j]), (j, t[-1], int(nxt[i]))
                at[j] = int(nxt[i])
                keep.append(j)
        live = keep
    return got, pages


@pytest.mark.parametrize("page", [1, 3, 16, 64])
def test_pages_concatenated_are_the_uncapped_search(V, page):
    """Batches of 1, 63, 64 and 65 queries, on the whole text and on a window per query: the pages every query yields when each search
    begins at the next position of the one before, without the queries that ran out, are the uncapped (windowed) search -- and brute
    force.  Queries finish at different pages; queries without a match say so at once."""
    text = dna_text(500, 33).tobytes()
    n = len(text)
    rng = np.random.default_rng(page)
    qs = _random_queries(text, rng, 61, kmax=3, mmax=3, gapmax=30, gaplo=6) + ["\xfe", "A.{0,3}?\xfe", "C", "A.{100000,100001}?A"]
    fields = [V.parse_query(q) for q in qs]
    fields[5:9] = [a for a in array_queries(text, 3, n=30) if len(a[0]) <= 3 and a[3] < I63][:4]      # caller-built: lo down to 0, other end_len
    assert len(fields) == 65
    idx = V.WtsaIndex(text)
    windows = [(int(a), int(b)) for a, b in (sorted(rng.integers(0, n + 1, 2)) for _ in fields)]
    for nq in (1, 63, 64, 65):
        for whole in (True, False):
            f = fields[:nq]
            begin = [0] * nq if whole else [w[0] for w in windows[:nq]]
            end = [n] * nq if whole else [w[1] for w in windows[:nq]]
            want = [_brute_window(text, f[j], begin[j], end[j]) for j in range(nq)]
            full = idx.search(_batch(V, f), begin=begin, end=end)
            assert [full.tuples(j).tolist() for j in range(nq)] == want
            assert (full.next_positions() == np.uint64(U64)).all()
            got, pages = _paged(V, idx, f, begin, end, page)
            assert got == want, (nq, whole)
            # a query takes one page per `page` matches and one more to learn that nothing is left
            assert pages == [len(w) // page + 1 for w in want]
            if nq == 65 and whole:
                assert len(set(pages)) > (3 if page <= 16 else 1) and min(len(w) for w in want) == 0 and max(len(w) for w in want) >= 64


@pytest.mark.parametrize("page", [1, 3, 16, 64])
def test_exactly_one_page_left_reports_a_position_then_nothing(V, page):
    text = b"xab" * page + b"zz"
    idx = V.WtsaIndex(text)
    r = idx.search(["ab"], max_matches=page)
    assert r.positions(0).tolist() == [3 * i + 1 for i in range(page)]
    assert r.next_positions().tolist() == [3 * page]                                   # last position + end_len, though nothing is left
    r2 = idx.search(["ab"], max_matches=page, begin=3 * page)
    assert r2.summary["n_matches"] == 0 and r2.next_positions().tolist() == [U64]
    # the generator that does the same; and on a window that ends inside the last occurrence
    assert [p.tolist() for p in idx.pages("ab", page=page)] == [[[3 * i + 1] for i in range(page)]]
    assert sum(len(p) for p in idx.pages("ab", page=page, begin=2, end=3 * page - 1)) == max(page - 2, 0)
    tup = V.WtsaIndex(dna_text(700, 33).tobytes())
    whole = tup.search(["A.{0,4}?C"]).tuples(0).tolist()
    assert [t for p in tup.pages("A.{0,4}?C", page=page) for t in p.tolist()] == whole and len(whole) > 64


@pytest.mark.parametrize("n", [223, 224, 225, 3000])
def test_range_count_and_report_against_the_suffix_array(V, n):
    """wt_int::range_search_2d as count + report: random suffix-array ranges (empty ones and the whole array among them) and value
    windows (vlb > vrb, vrb beyond n, vlb == vrb), against numpy on the suffix array; the output of every range is ascending; a range
    outside the array gives ~0 and leaves the canary-filled output alone."""
    import torch
    text = dna_text(n, 19).tobytes()
    sa = naive_sa(text + b"\0").astype(np.int64)
    nv = len(sa)
    idx = V.WtsaIndex(text)
    rng = np.random.default_rng(n)
    m = 300
    l = rng.integers(0, nv + 1, m)
    ln = np.array([rng.integers(0, nv - a + 1) for a in l])
    vlb = rng.integers(0, nv + 2, m)
    vrb = np.array([rng.integers(a, nv + 40) for a in vlb])
    swap = rng.integers(0, 8, m) == 0
    vlb, vrb = np.where(swap, vrb + 1, vlb), np.where(swap, vlb, vrb)                   # vlb > vrb
    same = rng.integers(0, 6, m) == 0
    vrb = np.where(same & ~swap, vlb, vrb)
    ln[rng.integers(0, 10, m) == 0] = 0
    edge = [(0, nv, 0, nv), (0, nv, 0, U64), (0, nv, 5, 5), (0, 0, 0, nv), (nv, 0, 0, nv), (nv - 1, 1, 0, U64), (0, nv, U64, U64), (0, nv, 1 << 40, 1 << 41),
            (3, nv - 3, nv - 1, nv - 1), (0, 1, nv - 1, nv - 1)]
    l = np.concatenate([l, [e[0] for e in edge]]).astype(np.uint64)
    ln = np.concatenate([ln, [e[1] for e in edge]]).astype(np.uint64)
    vlb = np.concatenate([vlb.astype(np.uint64), np.array([e[2] for e in edge], dtype=np.uint64)])
    vrb = np.concatenate([vrb.astype(np.uint64), np.array([e[3] for e in edge], dtype=np.uint64)])
    want = [sorted(int(v) for v in sa[int(a):int(a) + int(b)] if int(x) <= v <= int(y)) for a, b, x, y in zip(l, ln, vlb, vrb)]
    assert sum(1 for w in want if w) > 100 and any(not w for w in want)
    counts, off, vals = idx.range_report(l, ln, vlb, vrb)
    assert counts.tolist() == [len(w) for w in want]
    assert [vals[int(off[j]):int(off[j + 1])].tolist() for j in range(len(want))] == want
    # ranges outside the array: ~0, and nothing written -- neither for them nor for ranges whose offsets leave them no room
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=np.uint64)).view(np.int64)).cuda()
    bl, bn = dev([nv + 1, 0, nv, 2]), dev([0, nv + 1, 1, 3])
    blo, bhi = dev([0, 0, 0, 0]), dev([U64, U64, U64, U64])
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    idx.range_count_device(bl.data_ptr(), bn.data_ptr(), blo.data_ptr(), bhi.data_ptr(), d_cnt.data_ptr(), 4)
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().view(np.uint64).tolist() == [U64, U64, U64, 3]
    canary = 0x5AFE5AFE5AFE5AFE
    d_out = torch.full((12,), canary, dtype=torch.int64, device="cuda")
    d_off = dev([0, 2, 4, 6, 9])                                                      # the bad ranges are given room they must not use
    idx.range_report_device(bl.data_ptr(), bn.data_ptr(), blo.data_ptr(), bhi.data_ptr(), d_off.data_ptr(), 4, 9, d_out.data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [canary] * 6 + sorted(int(v) for v in sa[2:5]) + [canary] * 3
    # locate_window: the occurrences of a pattern that lie wholly inside [B, E)
    for pat in (b"A", b"AC", text[5:9], b"\xfe", text[-3:]):
        occ = occurrences(text, pat).tolist()
        for B, E in [(0, n), (0, None), (n // 3, 2 * n // 3), (0, 0), (n, n), (7, 7 + len(pat)), (7, 6 + len(pat)), (0, U64)] + \
                [tuple(sorted(int(x) for x in rng.integers(0, n + 1, 2))) for _ in range(6)]:
            e = n if E is None else min(E, n)
            assert idx.locate_window(pat, B, E).tolist() == [v for v in occ if B <= v and v + len(pat) <= e], (pat, B, E)


def test_locate_window_on_an_integer_text(V):
    text = _text("ints")
    idx = V.WtsaIndex(text)
    n = len(text)
    for pat in (text[3:5], np.array([0], np.uint32), np.array([2 ** 31], np.uint32), np.array([4242], np.uint32)):
        occ = occurrences(text, pat).tolist()
        for B, E in ((0, n), (100, 900), (n, n), (0, None)):
            e = n if E is None else E
            assert idx.locate_window(pat, B, E).tolist() == [v for v in occ if B <= v and v + len(pat) <= e]


def test_refusals(V):
    text = dna_text(500, 2).tobytes()
    idx = V.WtsaIndex(text)
    ws = V.index.Workspace()
    q = V.index.Queries(["A", "C.{0,3}?G"])
    # begin > end: VLG_E_INVALID and no result handle
    b, e = np.array([0, 11], dtype=np.uint64), np.array([500, 10], dtype=np.uint64)
    h = C.c_void_p(12345)
    st = V.lib().vlg_wtsa_search_window_batch(idx._h, q._h, b.ctypes.data, e.ctypes.data, 0, ws._h, C.byref(h))
    assert st == V.capi.E_INVALID and not h.value
    with pytest.raises(V.VlgError) as err:
        idx.search(q, begin=[0, 11], end=[500, 10])
    assert err.value.status == V.capi.E_INVALID
    # begin beyond the text with an end beyond it too is an empty window, not an error
    assert idx.search(q, begin=[600, 700], end=[U64, 800]).summary["n_matches"] == 0
    # arrays given for an empty batch are fine
    empty = V.index.Queries([])
    h = C.c_void_p()
    V.capi.check(V.lib().vlg_wtsa_search_window_batch(idx._h, empty._h, b.ctypes.data, e.ctypes.data, 0, ws._h, C.byref(h)))
    r = V.SearchResult(h, empty.ks)
    assert r.summary["n_queries"] == 0 and r.summary["n_matches"] == 0 and len(r.next_positions()) == 0
    # next positions exist for the lazy index's results only
    fm = V.VlgIndex.build(text).search(["A"])
    with pytest.raises(V.VlgError) as err:
        fm.next_positions()
    assert err.value.status == V.capi.E_INVALID
    # a batch of the other alphabet, as before
    with pytest.raises(V.VlgError) as err:
        idx.search(V.index.Queries.from_int(["1 2"]), begin=0, end=10)
    assert err.value.status == V.capi.E_INVALID
    ints = V.WtsaIndex(np.array([1, 2, 3, 1, 2], dtype=np.uint32))
    with pytest.raises(V.VlgError) as err:
        ints.search(q, begin=[0, 0], end=[3, 3])
    assert err.value.status == V.capi.E_INVALID
    assert ints.search(["1 2"], begin=1).tuples(0).tolist() == [[3]]


def test_cpp_iterator_continues_inside_a_window(V, tmp_path):
    """locate(idx, query, begin, end) of host/vlg_index_gpu.hpp, compiled against the library: the iterator refills several times (16
    matches, then three times what it holds, each request from the next position of the one before) and yields the windowed matches;
    begin > end is the library's refusal."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "vlg_matching_amd")
    exe = str(tmp_path / "wtsa_window_iter_check")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "wtsa_window_iter_check.cpp"), "-L", pkg, "-lvlg_hip", "-Wl,-rpath," + pkg])
    text = dna_text(4000, 77).tobytes()
    (tmp_path / "t.txt").write_bytes(text)
    q = "AC.{0,9}?G"
    f = V.parse_query(q)
    for B, E in ((0, 4000), (500, 3500), (1234, 1300), (10, 1 << 40), (4000, 4000)):
        out = subprocess.run([exe, str(tmp_path / "t.txt"), q, str(B), str(E)], capture_output=True, text=True, check=True).stdout
        want = _brute_window(text, f, B, E)
        assert [[int(x) for x in l.split()] for l in out.splitlines()] == want, (B, E)
        assert len(want) > 100 or E - B < 3000
    bad = subprocess.run([exe, str(tmp_path / "t.txt"), q, "9", "8"], capture_output=True, text=True)
    assert bad.returncode == 1 and "window" in bad.stderr
