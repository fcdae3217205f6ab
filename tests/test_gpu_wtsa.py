"""The paper's index on the GPU: text + wavelet tree over the suffix array, searched lazily
(sdsl::vlg_index / vlg_iterator, include/sdsl/vlg_index.hpp:109-373), byte and integer alphabets -- against the reference's known
answers, the CPU oracle (the survey established vlg_index == merge join tuple for tuple) and brute force."""
import json
import os

import numpy as np
import pytest

from util import dna_text, naive_sa, skewed_text

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vlg_known_answers.json")))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def test_known_answers_byte_and_int(V):
    for case in GOLD["cases"]:
        idx = V.WtsaIndex(case["text"].encode())
        if "error" in case:
            with pytest.raises(V.VlgError):
                idx.search([case["query"]])
        else:
            assert idx.search([case["query"]]).tuples(0).tolist() == case["tuples"], case
    for case in GOLD["int_cases"]:
        idx = V.WtsaIndex(np.array(case["int_text"], dtype=np.uint32))
        r = idx.search([case["query"]])
        assert r.tuples(0).tolist() == case["tuples"], case
        assert int(r.counts[0]) == len(case["tuples"])
        if r.summary["n_matches"]:
            with pytest.raises(V.VlgError):                                 # the lazy index keeps 64-bit positions: no narrow fetch
                r.fetch32()


@pytest.mark.parametrize("name", ["abracadabra", "one_byte", "100a", "dna", "zipf", "empty"])
def test_suffix_array_access_and_ranges(V, oracle, name):
    import torch
    text = {"abracadabra": b"abracadabrasimsalabim", "one_byte": b"a", "100a": b"a" * 100, "dna": dna_text(3000, 4).tobytes(),
            "zipf": skewed_text(5000, 6).tobytes(), "empty": b""}[name]
    idx = V.WtsaIndex(text)
    info = idx.info()
    assert info["n"] == len(text) + 1 and info["symbol_bytes"] == 1
    tz = np.frombuffer(text + b"\0", dtype=np.uint8)
    sa = oracle.suffix_array(tz) if len(text) else np.zeros(1, np.uint64)
    # wt[i] == SA[i] for every i (wt_int::operator[]; csa_byte_test.cpp:136-147 checks csa[j] == SA[j] the same way)
    d_i = torch.arange(len(sa), dtype=torch.int64, device="cuda")
    d_o = torch.zeros_like(d_i)
    idx.sa_device(d_i.data_ptr(), d_o.data_ptr(), len(sa))
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == sa).all()
    if not len(text):
        return
    # forward_search == backward_search of the FM-index oracle (same suffix array, same ranges)
    o = oracle.Index.from_text(text)
    rng = np.random.default_rng(3)
    pats = [text[s:s + int(rng.integers(1, 6))] for s in rng.integers(0, len(text), 60)] + [b"\xfe", text[:1] * 300, text[-3:]]
    qs = [p.decode("latin-1") for p in pats]
    sp, ep = idx.ranges(qs)
    for p, a, b in zip(pats, sp, ep):
        cnt, l, r = o.backward_search(p)
        assert int(b) + 1 - int(a) == cnt, p
        if cnt:
            assert (int(a), int(b)) == (l, r), p


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


@pytest.mark.parametrize("name,seed", [("dna", 1), ("dna_skew", 2), ("zipf", 3), ("100a", 4), ("abab", 5)])
def test_lazy_search_equals_oracle_and_fm_index_path(V, oracle, monkeypatch, name, seed):
    text = {"dna": dna_text(20000, 1).tobytes(), "dna_skew": dna_text(15000, 2, (0.7, 0.1, 0.1, 0.1)).tobytes(),
            "zipf": skewed_text(20000, 3).tobytes(), "100a": b"a" * 100, "abab": (b"ab" * 1200) + b"aab" * 200}[name]      # (abab: matches by the ten thousand per query -- kept short)
    rng = np.random.default_rng(seed)
    qs = _random_queries(text, rng, 150)
    qs += ["\xfe.{0,5}?" + qs[0][:1], qs[1][:1] + ".{0,5}?\xfe", qs[2][:1], text[:2].decode() + ".{0,100000000}?" + text[5:7].decode()]
    w = V.WtsaIndex(text)
    o = oracle.Index.from_text(text)
    fm = V.VlgIndex.build(text).search(qs)
    res = w.search(qs)
    total, chk = 0, 0
    for i, q in enumerate(qs):
        want = o.search(q)
        assert res.tuples(i).tolist() == want.tolist(), q
        assert res.tuples(i).tolist() == fm.tuples(i).tolist()
        total += len(want)
        chk = (chk + int(want[:, 0].sum())) % (1 << 64) if len(want) else chk
    assert res.summary["n_matches"] == total and res.summary["checksum"] == chk
    # lazily: the first N matches of every query are a prefix of all of them (an iterator that is not run to its end)
    for cap in (1, 3, 70):
        part = w.search(qs, max_matches=cap)
        for i in range(len(qs)):
            assert part.tuples(i).tolist() == res.tuples(i).tolist()[:cap], (cap, qs[i])
    # one lane per query (the round-2 kernel) instead of one wavefront: same tuples
    monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
    old = w.search(qs)
    for x, y in zip(old.fetch(), res.fetch()):
        assert (x == y).all()
    assert [w.search(qs, max_matches=2).tuples(i).tolist() for i in range(len(qs))] == [res.tuples(i).tolist()[:2] for i in range(len(qs))]
    monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")
    # first positions only
    from vlg_matching_amd.index import Workspace
    ws = Workspace()
    ws.set_option("tuples", 0)
    fp = w.search(qs, workspace=ws)
    assert (fp.counts == res.counts).all() and fp.summary["checksum"] == chk and fp.summary["n_tuple_values"] == 0
    for i in (0, 7, len(qs) - 1):
        assert fp.positions(i).tolist() == res.tuples(i)[:, 0].tolist() if int(res.counts[i]) else len(fp.positions(i)) == 0


def _int_occurrences(text, pat):
    n, m = len(text), len(pat)
    if m > n:
        return np.zeros(0, np.uint64)
    ok = np.ones(n - m + 1, dtype=bool)
    for t in range(m):
        ok &= text[t:n - m + 1 + t] == pat[t]
    return np.nonzero(ok)[0].astype(np.uint64)


def test_integer_alphabet_index_vs_brute_force(V, oracle):
    """vlg_index<int_alphabet_tag>: symbols far beyond a byte, zero as a symbol, queries as whitespace-separated decimals."""
    rng = np.random.default_rng(11)
    vocab = np.array([0, 1, 2, 255, 256, 1000, 65535, 65536, 2 ** 31, 2 ** 32 - 1, 7, 8], dtype=np.uint64)
    text = vocab[rng.choice(len(vocab), 6000, p=np.array([5, 5, 4, 3, 3, 2, 2, 1, 1, 1, 4, 4]) / 35.0)].astype(np.uint32)
    idx = V.WtsaIndex(text)
    info = idx.info()
    assert info["symbol_bytes"] == 4 and info["n"] == len(text) + 1
    # the suffix array: integer symbols compare as numbers, the sentinel is the smallest
    import torch
    sa = np.array(sorted(range(len(text) + 1), key=lambda i: [int(x) + 1 for x in text[i:]] + [0]), dtype=np.uint64) if len(text) <= 6000 else None
    d_i = torch.arange(len(text) + 1, dtype=torch.int64, device="cuda")
    d_o = torch.zeros_like(d_i)
    idx.sa_device(d_i.data_ptr(), d_o.data_ptr(), len(text) + 1)
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == sa).all()
    qs, parsed = [], []
    for _ in range(120):
        k = int(rng.integers(1, 4))
        subs = [text[s:s + int(rng.integers(1, 4))] for s in rng.integers(0, len(text) - 4, k)]
        gaps = [(a, a + int(rng.integers(0, 40))) for a in rng.integers(0, 10, k - 1)]
        q = " ".join(str(int(x)) for x in subs[0])
        for (a, b), sp in zip(gaps, subs[1:]):
            q += " .{%d,%d}? " % (a, b) + " ".join(str(int(x)) for x in sp)
        qs.append(q)
        parsed.append((subs, gaps))
    qs.append("4242 .{0,5}? 7")                                             # a symbol that does not occur
    parsed.append(([np.array([4242], np.uint32), np.array([7], np.uint32)], [(0, 5)]))
    res = idx.search(qs)
    for i, (subs, gaps) in enumerate(parsed):
        lists = [_int_occurrences(text, sp) for sp in subs]
        lo = [a + len(subs[j]) for j, (a, b) in enumerate(gaps)]                # vlg_index.hpp:95: gaps count symbols
        hi = [b + len(subs[j]) for j, (a, b) in enumerate(gaps)]
        m, want = oracle.join(lists, lo, hi, len(subs[-1])) if all(len(l) for l in lists) else (0, np.zeros((0, len(subs)), np.uint64))
        assert res.tuples(i).tolist() == want.tolist(), qs[i]
    part = idx.search(qs, max_matches=2)
    for i in range(len(qs)):
        assert part.tuples(i).tolist() == res.tuples(i).tolist()[:2]
    # a byte batch is refused by an integer index and the other way round; so is an integer batch by the FM-index entry points
    with pytest.raises(V.VlgError):
        V.capi.check(V.lib().vlg_wtsa_search_batch(idx._h, V.index.Queries(["a"])._h, 0, V.index.Workspace()._h, None)) if False else idx.search(V.index.Queries(["a"]))
    with pytest.raises(V.VlgError):
        V.VlgIndex.build(b"abcabc").search(idx.queries(["1 2"]))


# n_text where a level is added (2^j) and where a level ends on a super-block border (224 data bits a block, nb = n_vals / 224 + 1)
TREE_SIZES = (2, 3, 4, 222, 223, 224, 447, 448, 1023, 1024, 65535, 65536)
INT_TREE_SIZES = (223, 224, 1024)


@pytest.mark.parametrize("name", ["abracadabra", "one_byte", "100a", "dna", "zipf", "ints", "keeper"] + ["dna_n%d" % n for n in TREE_SIZES]
                         + ["ints_n%d" % n for n in INT_TREE_SIZES])
def test_tree_equals_reference_wt_int(V, oracle, refmod, name):
    """The device tree against the reference's OWN wt_int<bit_vector_il<>, rank_support_il<>> (oracle/_ref, built by its constructor
    from the same suffix array, as construct(wts, KEY_SA) does, vlg_index.hpp:386-387): number of levels, every level's bits ==
    wt_int::tree, wt[i] for every i (wt_int.hpp:339-361), and count_less / quantile on random suffix-array ranges == what the
    reference's expand(v) / expand(v, range) descent answers (wt_int.hpp:824-939)."""
    import torch
    if name in ("ints", "keeper") or name.startswith("ints_n"):
        rng = np.random.default_rng(8)
        if name == "keeper":                     # the reference's own integer fixture (test/test_cases/keeper.int; csa_int_test.config:7)
            import os
            itext = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keeper.int"), dtype="<u8").astype(np.uint32)
            assert len(itext) == 63 and int(itext.max()) == 21
        else:
            itext = rng.choice(np.array([3, 7, 7, 19, 1000, 70000, 2 ** 31 + 5], dtype=np.uint32), int(name[6:]) if name.startswith("ints_n") else 1500)
        idx = V.WtsaIndex(itext)
        vals = np.concatenate([itext.astype(np.int64) + 1, [0]])                 # the sentinel is smaller than every symbol
        sa = np.array(sorted(range(len(vals)), key=lambda i: vals[i:].tolist()), dtype=np.uint64)
    else:
        text = dna_text(int(name[5:]), 19).tobytes() if name.startswith("dna_n") else \
            {"abracadabra": b"abracadabrasimsalabim", "one_byte": b"a", "100a": b"a" * 100, "dna": dna_text(3000, 4).tobytes(),
             "zipf": skewed_text(5000, 6).tobytes()}[name]
        idx = V.WtsaIndex(text)
        sa = oracle.suffix_array(np.frombuffer(text + b"\0", dtype=np.uint8))
    n = len(sa)
    ref = oracle.RefWtInt(sa)
    info = idx.info()
    assert info["n"] == n and info["levels"] == ref.levels
    want_bits = ref.level_bits()
    for lvl in range(ref.levels):
        assert (idx.level_bits(lvl) == want_bits[lvl]).all(), lvl
    d_i = torch.arange(n, dtype=torch.int64, device="cuda")
    d_o = torch.zeros_like(d_i)
    idx.sa_device(d_i.data_ptr(), d_o.data_ptr(), n)
    torch.cuda.synchronize()
    got = d_o.cpu().numpy().view(np.uint64)
    assert (got == sa).all()
    # (65 537 values: the reference is asked for a seeded sample of them -- the one check in this file that is sampled)
    which = range(n) if n <= 65536 else sorted(np.random.default_rng(23).choice(n, 5000, replace=False).tolist())
    assert [int(got[i]) for i in which] == [ref[i] for i in which]
    rng = np.random.default_rng(17)
    m = 400
    l = rng.integers(0, n, m).astype(np.uint64)
    ln = np.array([rng.integers(1, n - int(a) + 1) for a in l], dtype=np.uint64)
    x = rng.integers(0, n + 3, m).astype(np.uint64)
    q = np.array([rng.integers(0, int(b)) for b in ln], dtype=np.uint64)
    # the edges: ranges that end at n_vals, of length 1 and of length n_vals; x at both ends of the values, of the tree's
    # value space (2^levels) and far beyond it
    el = [int(a) for a in rng.integers(0, n, 6)] + [0, n - 1, 0, n // 2]
    eln = [n - a for a in el[:6]] + [1, 1, n, 1]
    ex = [0, n - 1, n, (1 << ref.levels) - 1, 1 << ref.levels, 1 << 63]
    l = np.concatenate([l, np.array([a for a in el for _ in ex], dtype=np.uint64)])
    ln = np.concatenate([ln, np.array([b for b in eln for _ in ex], dtype=np.uint64)])
    x = np.concatenate([x, np.array(ex * len(el), dtype=np.uint64)])
    q = np.concatenate([q, np.array([(0, b - 1, b // 2, 0, b - 1, b // 3)[j] for b in eln for j in range(len(ex))], dtype=np.uint64)])
    m = len(l)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    d_l, d_n, d_x, d_q, d_out = dev(l), dev(ln), dev(x), dev(q), torch.zeros(m, dtype=torch.int64, device="cuda")
    idx.range_walk_device(d_l.data_ptr(), d_n.data_ptr(), d_x.data_ptr(), False, d_out.data_ptr(), m)
    torch.cuda.synchronize()
    assert [int(v) for v in d_out.cpu().numpy().view(np.uint64)] == [ref.count_less(a, b, c) for a, b, c in zip(l, ln, x)]
    idx.range_walk_device(d_l.data_ptr(), d_n.data_ptr(), d_q.data_ptr(), True, d_out.data_ptr(), m)
    torch.cuda.synchronize()
    assert [int(v) for v in d_out.cpu().numpy().view(np.uint64)] == [ref.quantile(a, b, c) for a, b, c in zip(l, ln, q)]
    # out-of-range requests are refused per element, not walked
    bad = dev(np.array([n + 5], dtype=np.uint64))
    one = dev(np.array([1], dtype=np.uint64))
    idx.range_walk_device(bad.data_ptr(), one.data_ptr(), one.data_ptr(), False, d_out.data_ptr(), 1)
    torch.cuda.synchronize()
    assert int(d_out.cpu().numpy().view(np.uint64)[0]) == (1 << 64) - 1


# ---- the lazy search at its edges: brute force (tests/vlg_brute.py) and the reference's own iterator as the yardsticks ----------------
from util import I63, array_queries                                     # noqa: E402
from vlg_brute import lazy_matches, occurrences                         # noqa: E402


def _fields(V, q):
    """(sub-patterns, lo, hi, end_len) of a regexp, or the tuple itself"""
    return V.parse_query(q) if isinstance(q, str) else q


def _batch(V, qs):
    f = [_fields(V, q) for q in qs]
    return V.index.Queries.from_arrays([x[0] for x in f], [x[1] for x in f], [x[2] for x in f], [x[3] for x in f])


def _brute(V, text, qs):
    out = []
    for q in qs:
        subs, lo, hi, end_len = _fields(V, q)
        out.append(lazy_matches([occurrences(text, s) for s in subs], lo, hi, end_len))
    return out


def _check_against_iterator(V, oracle, idx, sa, qs, got):
    """every parser-expressible query (but one sub-pattern of one symbol: test_oracle.py::test_vlg_iterator_skips_the_odd_twin...) through
    vlg_iterator on the reference's own tree over the same suffix array, the ranges as the device's forward search found them"""
    w = oracle.RefWtInt(sa)
    f = [_fields(V, q) for q in qs]
    sp, ep = idx.ranges(_batch(V, qs))
    s0, n = 0, 0
    for i, (subs, lo, hi, end_len) in enumerate(f):
        k = len(subs)
        rg = [(int(sp[s0 + j]), int(ep[s0 + j])) if int(ep[s0 + j]) + 1 > int(sp[s0 + j]) else (1, 0) for j in range(k)]
        s0 += k
        expressible = end_len == len(subs[-1]) and all(a >= len(s) for a, s in zip(lo, subs))
        if expressible and (k >= 2 or len(subs[0]) >= 2):
            assert w.vlg_iterate(rg, lo, hi, end_len).tolist() == got[i], (i, subs, lo, hi)
            n += 1
    return n


def _chain(k, pivot, pivot_sub, sub, gap):
    return ".{%d,%d}?".join([pivot_sub if i == pivot else sub for i in range(k)]) % ((gap[0], gap[1]) * (k - 1))


@pytest.mark.parametrize("name", ["400a", "dna"])
def test_pointer_machine_beyond_32_levels(V, oracle, refmod, monkeypatch, name):
    """k in {31, 32, 33, 34, 48, 64}: the kernel remembers in a 32-bit mask which pointers hold a value and recomputes the ones at
    depth >= 32 every time.  The pivot -- the query's shortest list, looked at 64 elements at a time -- stands at level 0, 31, 32, 33
    and k - 1 in turn (one sub-pattern is longer and rarer than the others).  Parsed chains and caller-built batches (lo = 0, end_len 1),
    uncapped and capped at 1 and 2, one wavefront and one lane per query."""
    text = b"a" * 400 if name == "400a" else dna_text(3000, 51).tobytes()
    rng = np.random.default_rng(52)
    qs = []
    for k in (31, 32, 33, 34, 48, 64):
        for piv in sorted({0, 31, 32, 33, k - 1}):
            if piv >= k:
                continue
            if name == "400a":
                qs.append(_chain(k, piv, "a" * 330, "a", (0, 2)))
                subs = ["a" * 330 if i == piv else "a" for i in range(k)]
                qs.append(([s.encode() for s in subs], [0 if i % 3 else 1 for i in range(k - 1)], [(0 if i % 3 else 1) + i % 4 for i in range(k - 1)], 1))
            else:
                s = int(rng.integers(0, len(text) - 1500))                # (an occurrence early enough for a chain behind it)
                rare = text[s + 8 * piv:s + 8 * piv + 4].decode()
                subs = [rare if i == piv else "ACGT"[int(rng.integers(0, 4))] for i in range(k)]
                q = subs[0]
                for i in range(1, k):
                    a = int(rng.integers(0, 4))
                    q += ".{%d,%d}?%s" % (a, a + int(rng.integers(8, 20)), subs[i])
                qs.append(q)
                lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
                qs.append(([x.encode() for x in subs], lo, [a + int(rng.integers(8, 20)) for a in lo], (1, 1000)[k % 2]))
    want = _brute(V, text, qs)
    assert sum(1 for w in want if w) >= len(qs) * 3 // 4 and sum(len(w) for w in want) > 60
    idx = V.WtsaIndex(text)
    # the pivot stands where it was meant to
    sp, ep = idx.ranges(_batch(V, qs))
    s0 = 0
    for q in qs:
        subs = _fields(V, q)[0]
        lens = [int(ep[s0 + j]) + 1 - int(sp[s0 + j]) for j in range(len(subs))]
        assert lens.index(min(lens)) == max(range(len(subs)), key=lambda j: len(subs[j]))
        s0 += len(subs)
    batch = _batch(V, qs)
    for lane in (False, True):
        if lane:
            monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
        res = idx.search(batch)
        for i, w in enumerate(want):
            assert res.tuples(i).tolist() == w, (lane, i, qs[i])
        for cap in (1, 2):
            part = idx.search(batch, max_matches=cap)
            for i, w in enumerate(want):
                assert part.tuples(i).tolist() == w[:cap], (lane, cap, i)
    monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")
    fm = V.VlgIndex.build(text).search(batch)
    for i, w in enumerate(want):
        assert fm.tuples(i).tolist() == w, i
    assert _check_against_iterator(V, refmod, idx, oracle.suffix_array(np.frombuffer(text + b"\0", dtype=np.uint8)), qs, want) >= len(qs) // 2


@pytest.mark.parametrize("name", ["dna", "zipf", "300a", "abab", "ints"])
def test_lazy_search_equals_the_references_iterator(V, oracle, refmod, name):
    """vlg_iterator (oracle/_ref) on the batches the device searches: every query with k >= 2 or |s| >= 2, byte and integer texts"""
    rng = np.random.default_rng(61)
    if name == "ints":
        vocab = np.array([0, 1, 2, 255, 256, 1000, 65535, 65536, 2 ** 31, 2 ** 32 - 1, 7, 8], dtype=np.uint64)
        text = vocab[rng.choice(len(vocab), 3000)].astype(np.uint32)
        vals = np.concatenate([text.astype(np.int64) + 1, [0]])
        sa = np.array(sorted(range(len(vals)), key=lambda i: vals[i:].tolist()), dtype=np.uint64)
        idx = V.WtsaIndex(text)
        qs, parsed = [], []
        for _ in range(100):
            k = int(rng.integers(1, 5))
            subs = [text[s:s + int(rng.integers(1, 4))] for s in rng.integers(0, len(text) - 4, k)]
            gaps = [(int(a), int(a) + int(rng.integers(0, 40))) for a in rng.integers(0, 10, k - 1)]
            q = " ".join(str(int(x)) for x in subs[0])
            for (a, b), sub in zip(gaps, subs[1:]):
                q += " .{%d,%d}? " % (a, b) + " ".join(str(int(x)) for x in sub)
            qs.append(q)
            parsed.append((subs, [a + len(s) for (a, _), s in zip(gaps, subs)], [b + len(s) for (_, b), s in zip(gaps, subs)], len(subs[-1])))
        batch = idx.queries(qs)
    else:
        text = {"dna": dna_text(4000, 41).tobytes(), "zipf": skewed_text(4000, 42).tobytes(), "300a": b"a" * 300, "abab": b"ab" * 600 + b"aab" * 100}[name]
        sa = oracle.suffix_array(np.frombuffer(text + b"\0", dtype=np.uint8))
        idx = V.WtsaIndex(text)
        qs = _random_queries(text, rng, 100, gapmax=40, gaplo=10)
        parsed = [V.parse_query(q) for q in qs]
        batch = V.index.Queries(qs)
    res = idx.search(batch)
    w = refmod.RefWtInt(sa)
    sp, ep = idx.ranges(batch)
    s0 = n = total = 0
    for i, (subs, lo, hi, end_len) in enumerate(parsed):
        k = len(subs)
        rg = [(int(sp[s0 + j]), int(ep[s0 + j])) if int(ep[s0 + j]) + 1 > int(sp[s0 + j]) else (1, 0) for j in range(k)]
        s0 += k
        got = res.tuples(i).tolist()
        assert got == lazy_matches([occurrences(text, s) for s in subs], lo, hi, end_len), qs[i]
        if k >= 2 or len(subs[0]) >= 2:
            assert got == w.vlg_iterate(rg, lo, hi, end_len).tolist(), qs[i]
            n += 1
            total += len(got)
    assert n >= 70 and total > 200


@pytest.mark.parametrize("name", ["dna", "abab"])
def test_capped_searches_are_prefixes_with_their_own_checksum(V, monkeypatch, name):
    """max_matches on every path that takes it: one pass into cap-sized stretches + compaction (cap <= 2^20; with and without
    tuples), the count-then-emit passes with a cap (cap = 2^20 + 1, and one lane per query) -- counts, positions and tuples are the
    uncapped result cut at the cap, the checksum is the sum over what was kept.  Batches of 1, 63, 64 and 65 queries, and one in
    which no query has a match (nothing to compact)."""
    text = {"dna": dna_text(4000, 41).tobytes(), "abab": b"ab" * 600 + b"aab" * 100}[name]
    rng = np.random.default_rng(71)
    qs = _random_queries(text, rng, 62, gapmax=30, gaplo=8) + ["\xfe", text[:1].decode(), text[:2].decode() + ".{0,50}?" + text[2:3].decode()]
    idx = V.WtsaIndex(text)
    full = idx.search(qs)
    want = _brute(V, text, qs)
    assert [full.tuples(i).tolist() for i in range(len(qs))] == want and max(len(w) for w in want) > 65
    from vlg_matching_amd.index import Workspace
    first_only = Workspace()
    first_only.set_option("tuples", 0)

    def check(part, nq, cap, tuples):
        kept = [w[:cap] for w in want[:nq]]
        assert [int(c) for c in part.counts] == [len(w) for w in kept]
        assert part.summary["n_matches"] == sum(len(w) for w in kept)
        assert part.summary["checksum"] == sum(t[0] for w in kept for t in w) % (1 << 64)
        assert part.summary["n_tuple_values"] == (sum(len(t) for w in kept for t in w) if tuples else 0)
        for i, w in enumerate(kept):
            assert part.positions(i).tolist() == [t[0] for t in w], (nq, cap, i)
            if tuples:
                assert part.tuples(i).tolist() == w, (nq, cap, i)

    for nq in (1, 63, 64, 65):
        for cap in (1, 3, 64, 65, (1 << 20) + 1):
            check(idx.search(qs[:nq], max_matches=cap), nq, cap, True)
            check(idx.search(qs[:nq], max_matches=cap, workspace=first_only), nq, cap, False)
    check(idx.search(qs, workspace=first_only), len(qs), 1 << 62, False)
    monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
    for cap in (1, 3, 65):
        check(idx.search(qs, max_matches=cap), len(qs), cap, True)
        check(idx.search(qs[:63], max_matches=cap, workspace=first_only), 63, cap, False)
    monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")
    none = ["\xfe.{0,5}?" + text[:1].decode(), text[:1].decode() + ".{0,5}?\xfe", "\xfd", text[:1].decode() + ".{100000,100001}?" + text[:1].decode()]
    for cap in (0, 1, 64, (1 << 20) + 1):
        for ws in (None, first_only):
            r = idx.search(none, max_matches=cap, workspace=ws)
            assert r.summary["n_matches"] == 0 and r.summary["checksum"] == 0 and r.summary["n_tuple_values"] == 0 and not r.counts.any()


@pytest.mark.parametrize("n_piv", [1, 63, 64, 65, 128, 129])
def test_pivot_list_is_walked_64_elements_at_a_time(V, n_piv):
    """The shortest list has 1, 63, 64, 65, 128, 129 elements, and the first of them with a partner inside the gap window stands at
    rank 0, 63, 64, at the end, or nowhere.  The text is a run of `a` with planted markers: `b` every 40 symbols (the pivot list), eleven
    `c` behind every `b` outside the window, and one `c` three symbols before and after the chosen `b` -- so the only match is known
    by construction: (b_r, b_r + 3), (b_r - 3, b_r) with the pivot last, (b_r - 4, b_r, b_r + 3) with it in the middle."""
    for r in sorted({x for x in (0, 63, 64, n_piv - 1) if x < n_piv}) + [None]:
        t = bytearray(b"a" * (40 * n_piv + 60))
        b_at = [20 + 40 * i for i in range(n_piv)]
        for p in b_at:
            t[p] = ord("b")
            for o in range(20, 31):
                t[p + o] = ord("c")
        if r is not None:
            t[b_at[r] + 3] = t[b_at[r] - 3] = ord("c")
        text = bytes(t)
        qs = ["b.{1,3}?c", "c.{1,3}?b", "a.{1,3}?b.{1,3}?c", ([b"b", b"c"], [3], [3], I63), ([b"c", b"b"], [0], [3], 1)]
        idx = V.WtsaIndex(text)
        res = idx.search(_batch(V, qs))
        x = b_at[r] if r is not None else None
        by_construction = [[[x, x + 3]], [[x - 3, x]], [[x - 4, x, x + 3]], [[x, x + 3]], [[x - 3, x]]] if r is not None else [[]] * 5
        assert _brute(V, text, qs) == by_construction
        assert [res.tuples(i).tolist() for i in range(len(qs))] == by_construction, (n_piv, r)
        assert [idx.search(_batch(V, qs), max_matches=1).tuples(i).tolist() for i in range(len(qs))] == by_construction
        assert occurrences(text, b"b").tolist() == b_at and len(occurrences(text, b"c")) > n_piv          # `b` is the pivot


def test_integer_index_lane_per_query_and_first_positions(V, monkeypatch):
    """the integer-alphabet index through the lane-per-query kernel, capped, and with first positions only: symbol 0, symbols >= 2^31,
    and a symbol the text does not hold as first, middle and last sub-pattern"""
    rng = np.random.default_rng(11)
    vocab = np.array([0, 1, 2, 255, 256, 1000, 65535, 65536, 2 ** 31, 2 ** 32 - 1, 7, 8], dtype=np.uint64)
    text = vocab[rng.choice(len(vocab), 6000, p=np.array([5, 5, 4, 3, 3, 2, 2, 1, 1, 1, 4, 4]) / 35.0)].astype(np.uint32)
    parsed = []
    for _ in range(100):
        k = int(rng.integers(1, 4))
        subs = [text[s:s + int(rng.integers(1, 4))] for s in rng.integers(0, len(text) - 4, k)]
        parsed.append((subs, [(int(a), int(a) + int(rng.integers(0, 40))) for a in rng.integers(0, 10, k - 1)]))
    absent, zero, big = np.array([4242], np.uint32), np.array([0], np.uint32), np.array([2 ** 31, 2 ** 32 - 1], np.uint32)
    for subs in ([absent, zero, big], [zero, absent, big], [zero, big, absent], [zero, zero], [big, zero], [np.array([2 ** 32 - 1], np.uint32)]):
        parsed.append((subs, [(0, 30)] * (len(subs) - 1)))
    qs, want = [], []
    for subs, gaps in parsed:
        q = " ".join(str(int(x)) for x in subs[0])
        for (a, b), sub in zip(gaps, subs[1:]):
            q += " .{%d,%d}? " % (a, b) + " ".join(str(int(x)) for x in sub)
        qs.append(q)
        want.append(lazy_matches([occurrences(text, s) for s in subs], [a + len(s) for (a, _), s in zip(gaps, subs)],
                                 [b + len(s) for (_, b), s in zip(gaps, subs)], len(subs[-1])))
    assert sum(len(w) for w in want) > 1000 and want[-2] and want[-3]
    idx = V.WtsaIndex(text)
    from vlg_matching_amd.index import Workspace
    first_only = Workspace()
    first_only.set_option("tuples", 0)
    for lane in (False, True):
        if lane:
            monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
        for cap in (0, 1, 3):
            kept = [w[:cap] if cap else w for w in want]
            res, fp = idx.search(qs, max_matches=cap), idx.search(qs, max_matches=cap, workspace=first_only)
            chk = sum(t[0] for w in kept for t in w) % (1 << 64)
            assert res.summary["checksum"] == fp.summary["checksum"] == chk
            assert res.summary["n_matches"] == fp.summary["n_matches"] == sum(len(w) for w in kept) and fp.summary["n_tuple_values"] == 0
            for i, w in enumerate(kept):
                assert res.tuples(i).tolist() == w, (lane, cap, qs[i])
                assert fp.positions(i).tolist() == res.positions(i).tolist() == [t[0] for t in w], (lane, cap, qs[i])
    monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY")
