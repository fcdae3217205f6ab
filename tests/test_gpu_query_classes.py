"""Character classes in sub-patterns on the GPU (vlg_queries_parse_classes + vlg_search_batch): the SA intervals of the branching
backward search against a suffix array computed here, and whole searches against tests/vlg_brute.py over the occurrence lists of
tests/vlg_class_brute.py."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import vlg_brute
import vlg_class_brute as B
from util import dna_text, skewed_text

pytestmark = pytest.mark.gpu

KINDS = ["plain", "rrr", "dens1", "textorder"]


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _workspace(opts=None, cap=0, stream=None):
    from vlg_matching_amd.index import Workspace
    ws = Workspace(cap, stream)
    for k, v in (opts or {}).items():
        ws.set_option(k, v)
    return ws


_texts, _sas, _idx = {}, {}, {}


def _text(name):
    if name not in _texts:
        _texts[name] = {"dna3000": lambda: dna_text(3000, 7).tobytes(), "dna50000": lambda: dna_text(50000, 8).tobytes(),
                        "dna40000": lambda: dna_text(40000, 9).tobytes(), "zipf": lambda: skewed_text(20000, 3).tobytes(),
                        "a100": lambda: b"a" * 100, "ab500": lambda: b"ab" * 500}[name]()
    return _texts[name]


def _suffix_array(name):
    """the suffix array of text + sentinel by prefix doubling (numpy), computed once per text"""
    if name not in _sas:
        t = np.frombuffer(_text(name) + b"\0", dtype=np.uint8).astype(np.int64)
        n = len(t)
        rank, k = t.copy(), 1
        while True:
            second = np.concatenate([rank[k:], np.full(min(k, n), -1, dtype=np.int64)])[:n]
            sa = np.lexsort((second, rank))
            changed = (rank[sa][1:] != rank[sa][:-1]) | (second[sa][1:] != second[sa][:-1])
            new = np.zeros(n, dtype=np.int64)
            new[sa] = np.concatenate([[0], np.cumsum(changed)])
            rank = new
            if rank.max() == n - 1:
                break
            k *= 2
        _sas[name] = np.argsort(rank).astype(np.uint64)
    return _sas[name]


def _index(V, name, kind="plain"):
    if (name, kind) not in _idx:
        base = _idx.get((name, "plain")) or V.VlgIndex.build(_text(name))
        _idx[(name, "plain")] = base
        _idx[(name, kind)] = {"plain": lambda: base, "rrr": lambda: base.compress(1), "dens1": lambda: base.resample(False, 1),
                              "textorder": lambda: base.resample(True, 32)}[kind]()
    return _idx[(name, kind)]


def _esc(members):
    return "".join("\\" + chr(c) for c in bytes(members))


def _regexp(subs, gaps):
    """subs: per sub-pattern a list of positions, each a bytes object of members; gaps: k - 1 pairs (a, b) -> the query, every byte escaped"""
    parts = ["".join(_esc(p) if len(p) == 1 else "[" + _esc(p) + "]" for p in s) for s in subs]
    out = parts[0]
    for (a, b), p in zip(gaps, parts[1:]):
        out += ".{%d,%d}?" % (a, b) + p
    return out


def _random_queries(text, rng, n, ks=(1, 2, 3, 5), mmax=4, extra=b""):
    """class queries cut out of the text: every sub-pattern is a substring of it with some positions widened to classes (members of the
    text's alphabet, and bytes the text does not have), gaps around the true distances so that many queries match"""
    alphabet = bytes(sorted(set(text)))
    out = []
    for j in range(n):
        k = ks[j % len(ks)]
        at, subs, gaps = int(rng.integers(0, max(1, len(text) - 400))), [], []
        for i in range(k):
            m = int(rng.integers(1, mmax + 1))
            sub = []
            for t in range(m):
                c = bytes([text[(at + t) % len(text)]])
                if rng.random() < 0.5:
                    more = bytes(rng.choice(list(alphabet + extra), size=int(rng.integers(1, 4))).astype(np.uint8).tolist())
                    c = bytes(sorted(set(c + more)))
                sub.append(c)
            subs.append(sub)
            step = int(rng.integers(0, 12))
            if i + 1 < k:
                gaps.append((max(0, step - int(rng.integers(0, 4))), step + int(rng.integers(0, 30))))
            at += m + step
        out.append(_regexp(subs, gaps))
    return out


_memo = {}


def _expected(text, regexp):
    """the matches of one query by brute force, computed once and shared by the tests (never changed)"""
    key = (len(text), text[:64], regexp)
    if key not in _memo:
        subs, lo, hi, end = B.parse(regexp)
        lists = [B.class_occurrences(text, s) for s in subs]
        _memo[key] = (vlg_brute.lazy_matches(lists, lo, hi, end), subs)
    return _memo[key]


def _check_search(V, text, idx, regexps, ws, tuples=True):
    q = V.Queries.from_classes(regexps)
    res = idx.search(q, workspace=ws)
    total, checksum, nonempty = 0, 0, 0
    for i, r in enumerate(regexps):
        want, _ = _expected(text, r)
        assert int(res.counts[i]) == len(want), r
        assert res.positions(i).tolist() == [w[0] for w in want], r
        if tuples:
            assert res.tuples(i).tolist() == want, r
        total += len(want)
        checksum += sum(w[0] for w in want)
        nonempty += bool(want)
    assert res.summary["n_matches"] == total and res.summary["checksum"] == checksum % (1 << 64)
    assert res.summary["n_tuple_values"] == (sum(len(B.parse(r)[0]) * int(res.counts[i]) for i, r in enumerate(regexps)) if tuples else 0)
    return res, nonempty


def _check_intervals(V, name, regexps, res):
    """every sub-pattern's intervals: ascending, disjoint, exactly its occurrences through the suffix array, one per member string present"""
    text, sa = _text(name), _suffix_array(name)
    off, l, r = res.class_intervals()
    s = 0
    for rx in regexps:
        for rows in B.parse(rx)[0]:
            a, b = int(off[s]), int(off[s + 1])
            ll, rr = l[a:b].astype(np.int64), r[a:b].astype(np.int64)
            assert (ll <= rr).all() and (ll[1:] > rr[:-1]).all(), (rx, s)
            got = np.sort(np.concatenate([sa[x:y + 1] for x, y in zip(ll, rr)] + [np.zeros(0, np.uint64)]))
            assert got.tolist() == B.class_occurrences(text, rows).tolist(), (rx, s)
            assert b - a == len(B.distinct_member_strings(text, rows)), (rx, s)
            s += 1
    assert s + 1 == len(off)


@pytest.mark.parametrize("name", ["dna3000", "zipf", "a100", "ab500"])
def test_intervals_are_the_occurrences(V, name):
    text = _text(name)
    rng = np.random.default_rng(len(text))
    regexps = _random_queries(text, rng, 40, extra=b"\xf0z")
    res = _index(V, name).search(V.Queries.from_classes(regexps))
    _check_intervals(V, name, regexps, res)
    off = res.class_intervals()[0]
    if name in ("dna3000", "zipf"):
        assert (np.diff(off.astype(np.int64)) > 1).sum() > 10               # not vacuous: many sub-patterns have several intervals


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tuples", [1, 0])
def test_search_matches_brute_force(V, kind, tuples):
    ws = _workspace({"tuples": tuples, "filter_min": 0, "filter_stream_min": 0})
    seen = 0
    for name in ("dna3000", "zipf", "ab500"):
        text = _text(name)
        rng = np.random.default_rng(11 + len(text))
        regexps = _random_queries(text, rng, 48, extra=b"\xf0")
        assert {len(B.parse(r)[0]) for r in regexps} == {1, 2, 3, 5}
        res, nonempty = _check_search(V, text, _index(V, name, kind), regexps, ws, bool(tuples))
        assert nonempty > len(regexps) // 2 and res.summary["n_matches"] > 100
        seen += res.summary["n_matches"]
    assert seen > 1000


def test_search_on_dna50000_default_options(V):
    text = _text("dna50000")
    regexps = _random_queries(text, np.random.default_rng(4), 16, mmax=5)
    res, nonempty = _check_search(V, text, _index(V, "dna50000"), regexps, _workspace())
    assert nonempty >= 12
    _check_intervals(V, "dna50000", regexps, res)


@pytest.mark.parametrize("force", ["1", "2"])
def test_wide_sa_indices(V, monkeypatch, force):
    """VLG_FORCE_POS64: an index with 64-bit samples (the kernels of a text beyond 2^32 symbols): the walks run on 64-bit words, the
    lists behind them hold 32-bit positions"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text = _text("dna3000")
    idx = V.VlgIndex.build(text)
    assert idx.info()["pos_bytes"] == 8
    regexps = _random_queries(text, np.random.default_rng(11 + len(text)), 48, extra=b"\xf0")
    res, nonempty = _check_search(V, text, idx, regexps, _workspace())
    assert nonempty > 24
    _check_intervals(V, "dna3000", regexps, res)


def test_wave_borders(V):
    """(symbol, parent) pairs of one step: 63, 64 and 65 -- a wave less one, a wave, a wave and one -- and several hundred"""
    text = _text("zipf")
    rng = np.random.default_rng(21)
    alphabet = np.array(sorted(set(text)), dtype=np.uint8)
    freq = np.array([text.count(bytes([c])) for c in alphabet])
    common = alphabet[np.argsort(-freq)]
    found = {}
    for trial in range(4000):
        if len(found) == 4:
            break
        sizes = rng.integers(1, 9, size=3)
        cls = [bytes(sorted(rng.choice(common[:int(rng.integers(8, 30))], size=int(z), replace=False).tolist())) for z in sizes]
        rows = [B.row(c) for c in cls]
        frontier = len(B.distinct_member_strings(text, rows[1:]))           # intervals in front of the last step
        work = frontier * len(set(cls[0]) & set(text))
        key = work if work in (63, 64, 65) else ("many" if work >= 300 else None)
        if key and key not in found:
            found[key] = cls
    assert set(found) == {63, 64, 65, "many"}, sorted(map(str, found))
    eight = [bytes(sorted(common[:8].tolist()))] * 3                        # 8-member classes over 3 positions: 8 x (up to 64) pairs
    regexps = [_regexp([[c for c in cls]], []) for cls in list(found.values()) + [eight]]
    regexps += [_regexp([[c for c in found[64]], [c for c in found[65]]], [(0, 50)])]
    res, nonempty = _check_search(V, text, _index(V, "zipf"), regexps, _workspace())
    assert nonempty == len(regexps)
    _check_intervals(V, "zipf", regexps, res)
    assert len(B.distinct_member_strings(text, [B.row(c) for c in eight[1:]])) * 8 >= 300


def test_class_shapes(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    regexps = ["[AC]GT", "A[CG]T", "AC[GT]", "[ACG]", "[A]CG", "ACG", "[AZ\xf0]C[Gz]", "[^A]C", "[^ACGT]",
               "[A-C]G.{0,9}?[G-T]", "[Zz]A.{0,5}?C", "AC.{1,8}?[Zz]", "[CG][CG][CG][CG].{0,40}?[AT][AT][AT]"]
    res, nonempty = _check_search(V, text, idx, regexps, _workspace())
    _check_intervals(V, "dna3000", regexps, res)
    counts = res.counts
    assert int(counts[4]) == int(counts[5]) > 0 and res.tuples(4).tolist() == res.tuples(5).tolist()    # a class of one byte is the literal
    assert int(counts[8]) == 0 and int(counts[10]) == 0 and int(counts[11]) == 0                        # no member in the text: that query alone dies
    assert nonempty == len(regexps) - 3
    # sigma == 1: one symbol beside the sentinel
    a = _text("a100")
    res, _ = _check_search(V, a, _index(V, "a100"), ["[^a]", "[a]", "[ab]a.{0,3}?[a]", "a[^a]"], _workspace())
    assert res.counts.tolist() == [0, 100, 33, 0]
    off, l, r = res.class_intervals()
    assert np.diff(off.astype(np.int64)).tolist() == [0, 1, 1, 1, 0] and (int(l[0]), int(r[0])) == (1, 100)
    res, _ = _check_search(V, _text("ab500"), _index(V, "ab500"), ["[ab][ab]", "[ab]", "[^b][^a].{0,0}?[a-b]"], _workspace())
    assert res.counts.tolist() == [500, 1000, 250]


def _with_frontier(text, rng, common, target):
    """a two-position class sub-pattern of which exactly `target` member strings occur (its last frontier), no step above that"""
    for trial in range(20000):
        cls = [bytes(sorted(rng.choice(common, size=int(z), replace=False).tolist())) for z in rng.integers(2, 20, size=2)]
        if len(B.distinct_member_strings(text, [B.row(c) for c in cls])) == target and len(cls[1]) <= target:
            return cls
    raise AssertionError("no sub-pattern with %d alternatives found" % target)


@pytest.mark.parametrize("c", [4, 64])
def test_frontier_cap(V, c):
    text = _text("zipf")
    idx = _index(V, "zipf")
    rng = np.random.default_rng(c)
    alphabet = np.array(sorted(set(text)), dtype=np.uint8)
    ws = _workspace({"class_intervals": c})
    if c == 4:
        legal, over = [bytes(alphabet[:4].tolist())], [bytes(alphabet[:5].tolist())]      # one position: 4 and 5 members, all in the text
    else:
        legal, over = _with_frontier(text, rng, alphabet, c), _with_frontier(text, rng, alphabet, c + 1)
    ok = [_regexp([[c_ for c_ in legal]], []), _regexp([[bytes(alphabet[:1].tolist())], [c_ for c_ in legal]], [(0, 20)])]
    res, nonempty = _check_search(V, text, idx, ok, ws)
    assert nonempty == 2 and int(np.diff(res.class_intervals()[0].astype(np.int64)).max()) == c          # exactly c is legal
    bad = ok[:1] + [_regexp([[bytes(alphabet[:1].tolist())], [c_ for c_ in over]], [(0, 20)])]
    with pytest.raises(V.VlgError) as e:
        idx.search(V.Queries.from_classes(bad), workspace=ws)
    assert e.value.status == V.capi.E_WORKSPACE
    assert "query 1" in str(e.value) and "sub-pattern 1" in str(e.value) and "class_intervals" in str(e.value)
    res, nonempty = _check_search(V, text, idx, ok, ws)                                                   # the workspace answers the next batch
    assert nonempty == 2
    ws.set_option("class_intervals", c + 1)
    res, nonempty = _check_search(V, text, idx, bad, ws)
    assert nonempty == 2


def test_shared_lists_are_located_once(V):
    text = _text("dna3000")
    subs = ["[AC]G", "T[CG]A", "[AT][AT]", "[^A]C", "GG[ACT]"]
    rng = np.random.default_rng(2)
    regexps = []
    for j in range(200):
        i, k = rng.choice(5, size=2)
        regexps.append("%s.{0,%d}?%s" % (subs[i], 20 + j % 7, subs[k]))
    ws = _workspace()
    res, nonempty = _check_search(V, text, _index(V, "dna3000"), regexps, ws)
    assert nonempty == 200
    each = [len(B.class_occurrences(text, B.parse(s)[0][0])) for s in subs]
    assert res.summary["located_occurrences"] == sum(each)
    assert res.summary["logical_occurrences"] == sum(len(B.class_occurrences(text, rows)) for r in regexps for rows in B.parse(r)[0])
    assert ws.kernel_stats()["class_search"]["launches"] == 1


def test_super_chunks(V):
    text = _text("dna40000")
    idx = _index(V, "dna40000")
    sets = ["[AC]", "[AG]", "[AT]", "[CG]", "[CT]", "[GT]", "[ACG]", "[ACT]", "[AGT]", "[CGT]", "[ACGT]"]
    regexps = ["%s.{%d,%d}?%s" % (sets[j], 3 + j, 9 + j, sets[(j + 5) % len(sets)]) for j in range(len(sets))]
    small = _workspace(cap=17 << 20)
    res, nonempty = _check_search(V, text, idx, regexps, small)
    assert nonempty == len(regexps) and res.summary["n_chunks"] >= 2
    # the lists of all queries do not fit the physical budget of this cap at once: 25 bytes per occurrence, half of cap - 8 MiB
    assert res.summary["located_occurrences"] > ((17 << 20) - (8 << 20)) // 2 // 25
    big = idx.search(V.Queries.from_classes(regexps), workspace=_workspace())
    assert big.fetch()[3].tolist() == res.fetch()[3].tolist() and big.summary["checksum"] == res.summary["checksum"]


def test_batch_without_classes_takes_the_existing_path(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    rng = np.random.default_rng(9)
    regexps = []
    for j in range(64):
        a, b = rng.integers(0, len(text) - 40, size=2)
        regexps.append("%s.{0,%d}?%s" % (text[a:a + 3].decode(), 10 + j, text[b:b + 2 + j % 3].decode()))
    regexps += ["\\A\\C", "[A]C[G]", "A[C].{1,2}?\\G"]
    plain = regexps[:64] + ["AC", "ACG", "AC.{1,2}?G"]
    ws1, ws2 = _workspace(), _workspace()
    got, want = idx.search(V.Queries.from_classes(regexps), workspace=ws1), idx.search(V.Queries(plain), workspace=ws2)
    assert got.summary == want.summary and got.summary["n_matches"] > 50
    for a, b in zip(got.fetch(), want.fetch()):
        assert a.tolist() == b.tolist()
    k1, k2 = ws1.kernel_stats(), ws2.kernel_stats()
    assert k1["class_search"]["launches"] == 0
    assert {k: v["launches"] for k, v in k1.items()} == {k: v["launches"] for k, v in k2.items()}
    with pytest.raises(V.VlgError) as e:
        got.class_intervals()
    assert e.value.status == V.capi.E_INVALID
    idx.search(V.Queries.from_classes(["A[CG]"]), workspace=ws1)
    assert ws1.kernel_stats()["class_search"]["launches"] > 0
    # the already-parsed form: the same batch from mask rows
    fields = [V.parse_class_query(r) for r in ["A[CG]T.{0,9}?[^A]", "AC"]]
    qa = V.Queries.from_class_arrays([f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields], [f[3] for f in fields])
    ra, rb = idx.search(qa), idx.search(V.Queries.from_classes(["A[CG]T.{0,9}?[^A]", "AC"]))
    assert ra.summary == rb.summary and ra.fetch()[3].tolist() == rb.fetch()[3].tolist() and ra.summary["n_matches"] > 10
    with pytest.raises(V.VlgError) as e:
        V.Queries.from_class_arrays([[np.zeros((1, 32), np.uint8)]], [[]], [[]], [1])
    assert e.value.status == V.capi.E_INVALID


def test_workspace_with_its_own_stream(V):
    import torch
    text = _text("zipf")
    regexps = _random_queries(text, np.random.default_rng(33), 40)
    stream = torch.cuda.Stream()
    own = _workspace(stream=C.c_void_p(stream.cuda_stream))
    res, nonempty = _check_search(V, text, _index(V, "zipf"), regexps, own)
    null = _index(V, "zipf").search(V.Queries.from_classes(regexps), workspace=_workspace())
    assert nonempty > 20 and res.summary == null.summary
    for a, b in zip(res.fetch(), null.fetch()):
        assert a.tolist() == b.tolist()
    for a, b in zip(res.class_intervals(), null.class_intervals()):
        assert a.tolist() == b.tolist()


def test_refusals(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    q = V.Queries.from_classes(["A[CG]T", "AC.{0,4}?[GT]"])
    ws = _workspace()
    idx.search(q, workspace=ws)
    before = ws.kernel_stats()
    with pytest.raises(V.VlgError) as e:
        q.set_windows(0, 100)
    assert e.value.status == V.capi.E_UNSUPPORTED and q.windows() is None
    for call in (lambda: idx.occurrences(q), lambda: idx.intervals(q)):
        with pytest.raises(V.VlgError) as e:
            call()
        assert e.value.status == V.capi.E_UNSUPPORTED
    w = V.WtsaIndex(text)
    for call in (lambda: w.search(q, workspace=ws), lambda: w.ranges(q), lambda: w.search(q, workspace=ws, begin=0, end=50)):
        with pytest.raises(V.VlgError) as e:
            call()
        assert e.value.status == V.capi.E_UNSUPPORTED
    ints = V.VlgIndex.build_int(np.frombuffer(text, dtype=np.uint8).astype(np.uint32))
    with pytest.raises(V.VlgError) as e:
        ints.search(q, workspace=ws)
    assert e.value.status in (V.capi.E_UNSUPPORTED, V.capi.E_INVALID)
    assert ws.kernel_stats() == before                                      # nothing was launched
    with pytest.raises(V.VlgError) as e:
        ws.set_option("class_intervals", 0)
    assert e.value.status == V.capi.E_INVALID


# ---- recorded behaviour: every counter, interval and match of fixed batches as the commit named in the fixture computed them ---------------
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_batches_recorded.json")


def _digest(a):
    a = np.ascontiguousarray(a)
    return a.tolist() if a.size <= 32 else {"len": int(a.size), "sha256": hashlib.sha256(a.astype("<u8").tobytes()).hexdigest()}


def _observe(res, ws):
    """everything a batch leaves behind that is a deterministic function of index, batch and options"""
    off, l, r = res.class_intervals()
    counts, offsets, first, tuples = res.fetch()
    return {"summary": dict(res.summary),
            "class_intervals": {"off": _digest(off), "l": _digest(l), "r": _digest(r)},
            "fetch": {"counts": _digest(counts), "offsets": _digest(offsets), "first": _digest(first), "tuples": _digest(tuples)},
            "launches": {k: v["launches"] for k, v in ws.kernel_stats().items()}}


def _recorded_cases(V):
    """name -> a function that runs the batch in a fresh workspace with an explicit cap and observes it"""
    text = _text("dna3000")
    regexps = _random_queries(text, np.random.default_rng(11 + len(text)), 48, extra=b"\xf0")      # test_search_matches_brute_force's
    opts = {"tuples": 1, "filter_min": 0, "filter_stream_min": 0}

    def run(kind):
        ws = _workspace(opts, cap=1 << 30)
        return _observe(_index(V, "dna3000", kind).search(V.Queries.from_classes(regexps), workspace=ws), ws)
    return {"classes/dna3000/" + kind: (lambda kind=kind: run(kind)) for kind in ("plain", "rrr")}


def _check_recorded(cases):
    with open(RECORDED) as f:
        want = json.load(f)["cases"]
    for name, run in cases.items():
        got = run()
        assert set(got) == set(want[name]), name
        for part, fields in want[name].items():
            assert fields and {k: got[part][k] for k in fields} == fields, (name, part)


def test_recorded_behaviour(V):
    _check_recorded(_recorded_cases(V))
