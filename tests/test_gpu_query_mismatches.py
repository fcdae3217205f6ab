"""Mismatch budgets per sub-pattern on the GPU (vlg_queries_set_mismatches + vlg_search_batch): the SA intervals of the budgeted
backward search against a suffix array computed here, and whole searches against tests/vlg_brute.py over the occurrence lists of
tests/vlg_approx_brute.py.  Texts, suffix arrays and indexes are those of tests/test_gpu_query_classes.py (one cache)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_query_classes as K
import vlg_approx_brute as A
import vlg_brute
import vlg_class_brute as B
from test_gpu_query_classes import _index, _regexp, _suffix_array, _text, _workspace

pytestmark = pytest.mark.gpu

KINDS = K.KINDS
ROOMY = 1 << 15                    # "class_intervals" for the random batches: the first steps of a budgeted search are unconstrained


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _sigma_text(sigma):
    """2 000 random symbols over exactly `sigma` distinct bytes (33 ..), every one of them present"""
    name = "sigma%d" % sigma
    if name not in K._texts:
        rng = np.random.default_rng(sigma)
        t = np.concatenate([np.arange(sigma), rng.integers(0, sigma, size=2000 - sigma)])
        K._texts[name] = (33 + rng.permutation(t)).astype(np.uint8).tobytes()
    return name


def _batch(V, regexps, budgets):
    """the batch of `regexps` (class dialect, every byte escaped by _regexp) with one budget per sub-pattern, or a scalar"""
    q = V.Queries.from_classes(regexps)
    q.set_mismatches(budgets)
    return q


def _sub_budgets(regexps, budgets):
    nsub = sum(len(B.parse(r)[0]) for r in regexps)
    return [int(budgets)] * nsub if np.ndim(budgets) == 0 else [int(b) for b in budgets]


_memo = {}


def _expected(text, regexp, ks):
    """the matches of one query under the budgets ks (one per sub-pattern) by brute force, computed once and never changed"""
    key = (len(text), text[:64], regexp, tuple(ks))
    if key not in _memo:
        subs, lo, hi, end = B.parse(regexp)
        lists = [A.approx_occurrences(text, s, k) for s, k in zip(subs, ks)]
        _memo[key] = vlg_brute.lazy_matches(lists, lo, hi, end)
    return _memo[key]


def _check_search(V, text, idx, regexps, budgets, ws, tuples=True):
    ks = _sub_budgets(regexps, budgets)
    res = idx.search(_batch(V, regexps, ks), workspace=ws)
    total, checksum, nonempty, s = 0, 0, 0, 0
    for i, r in enumerate(regexps):
        k = len(B.parse(r)[0])
        want = _expected(text, r, ks[s:s + k])
        s += k
        assert int(res.counts[i]) == len(want), (r, i)
        assert res.positions(i).tolist() == [w[0] for w in want], (r, i)
        if tuples:
            assert res.tuples(i).tolist() == want, (r, i)
        total += len(want)
        checksum += sum(w[0] for w in want)
        nonempty += bool(want)
    assert res.summary["n_matches"] == total and res.summary["checksum"] == checksum % (1 << 64)
    if res.summary["located_occurrences"]:
        assert res.summary["locate_mode"] == V.capi.LOCATE_WALKS
    return res, nonempty


def _check_intervals(name, regexps, budgets, res):
    """every sub-pattern's intervals: ascending, disjoint, exactly its occurrences through the suffix array, one per distinct string
    within the budget that occurs"""
    text, sa = _text(name), _suffix_array(name)
    ks = _sub_budgets(regexps, budgets)
    off, l, r = res.class_intervals()
    s, several = 0, 0
    for rx in regexps:
        for rows in B.parse(rx)[0]:
            a, b = int(off[s]), int(off[s + 1])
            ll, rr = l[a:b].astype(np.int64), r[a:b].astype(np.int64)
            assert (ll <= rr).all() and (ll[1:] > rr[:-1]).all(), (rx, s)
            got = np.sort(np.concatenate([sa[x:y + 1] for x, y in zip(ll, rr)] + [np.zeros(0, np.uint64)]))
            assert got.tolist() == A.approx_occurrences(text, rows, ks[s]).tolist(), (rx, s, ks[s])
            assert b - a == (A.frontier_widths(text, rows, ks[s])[-1] if len(rows) <= len(text) else 0), (rx, s, ks[s])
            several += b - a > 1
            s += 1
    assert s + 1 == len(off)
    return several


def _cut(text, rng, at, m, subst, classes=False, alphabet=None):
    """a sub-pattern cut out of text[at:at + m] with `subst` positions replaced by another byte of the alphabet (a real substitution);
    with classes, some of the other positions are widened"""
    alphabet = alphabet or bytes(sorted(set(text)))
    sub = [bytes([text[at + t]]) for t in range(m)]
    for t in rng.choice(m, size=min(subst, m), replace=False):
        others = [c for c in alphabet if c != text[at + t]] or list(alphabet)
        sub[t] = bytes([int(rng.choice(others))])
    if classes:
        for t in range(m):
            if rng.random() < 0.3:
                sub[t] = bytes(sorted(set(sub[t] + bytes(rng.choice(list(alphabet), size=2).astype(np.uint8).tolist()))))
    return sub


def _random_queries(text, rng, n, over=0, ks=(1, 2, 3, 5), mrange=(3, 7), kmax=2, classes=False):
    """queries cut out of the text: sub-pattern i has the budget b_i in 0 .. kmax and b_i + over substituted positions, gaps around the
    true distances -- with over = 0 every query has at least the match it was cut from"""
    regexps, budgets = [], []
    for j in range(n):
        k = ks[j % len(ks)]
        at, subs, gaps = int(rng.integers(0, len(text) - 400)), [], []
        for i in range(k):
            m = int(rng.integers(mrange[0], mrange[1] + 1))
            b = int(rng.integers(0, kmax + 1))
            subs.append(_cut(text, rng, at, m, b + over if b + over <= m else m, classes and j % 2 == 1))
            budgets.append(b)
            step = int(rng.integers(0, 12))
            if i + 1 < k:
                gaps.append((max(0, step - int(rng.integers(0, 4))), step + int(rng.integers(0, 30))))
            at += m + step
        regexps.append(_regexp(subs, gaps))
    return regexps, budgets


# ---- 0. the host contract on real batches (a batch needs a device to exist) -----------------------------------------------------------
def _four_batches(V):
    plain = ["ACG.{1,5}?TT", "GATT"]
    f = [V.parse_query(r) for r in plain]
    fc = [V.parse_class_query(r) for r in ["A[CG]G.{1,5}?TT", "GATT"]]
    return [V.Queries(plain), V.Queries.from_arrays([x[0] for x in f], [x[1] for x in f], [x[2] for x in f], [x[3] for x in f]),
            V.Queries.from_classes(["A[CG]G.{1,5}?TT", "GATT"]),
            V.Queries.from_class_arrays([x[0] for x in fc], [x[1] for x in fc], [x[2] for x in fc], [x[3] for x in fc])]


def test_set_get_round_trip(V):
    for q in _four_batches(V):
        assert q.mismatches() is None
        q.set_mismatches(2)
        assert q.mismatches().tolist() == [2, 2, 2]
        q.set_mismatches([0, 255, 1])
        assert q.mismatches().tolist() == [0, 255, 1] and q.mismatches().dtype == np.uint8
        q.set_mismatches(0)                                                 # all zeros remove
        assert q.mismatches() is None
        q.set_mismatches(np.array([1, 0, 0], np.uint8))
        assert q.mismatches().tolist() == [1, 0, 0]
        q.set_mismatches(None)                                              # NULL removes
        assert q.mismatches() is None
        k, has = (C.c_uint8 * 3)(9, 9, 9), C.c_int(5)
        assert V.lib().vlg_queries_get_mismatches(q._h, C.byref(has), k) == 0 and has.value == 0 and list(k) == [0, 0, 0]
        assert V.lib().vlg_queries_get_mismatches(q._h, None, None) == 0
        for bad in ([1, 2], [1, 2, 3, 4], [0, 256, 0], -1, 1.5, [1.0, 2.0, 0.0], ["1", "2", "3"]):
            with pytest.raises(ValueError):
                q.set_mismatches(bad)
        assert q.mismatches() is None
    empty = V.Queries([])
    empty.set_mismatches(3)
    assert empty.mismatches() is None


def test_host_refusals_leave_the_batch_as_it_was(V):
    ints = V.Queries.from_int(["1 2 3.{0,4}?5 6"])
    with pytest.raises(V.VlgError) as e:
        ints.set_mismatches(1)
    assert e.value.status == V.capi.E_UNSUPPORTED and ints.mismatches() is None
    ints.set_mismatches(0)                                                  # (removing what is not there is no refusal)
    plain, _, classes, _ = _four_batches(V)
    # budgets on a batch that carries windows
    plain.set_windows([0, 5], [100, 200])
    with pytest.raises(V.VlgError) as e:
        plain.set_mismatches(1)
    assert e.value.status == V.capi.E_UNSUPPORTED and plain.mismatches() is None
    assert [w.tolist() for w in plain.windows()] == [[0, 5], [100, 200]]
    plain.set_windows(None, None)
    # windows on a batch that carries budgets
    for q in (plain, classes):
        q.set_mismatches([1, 0, 2])
        with pytest.raises(V.VlgError) as e:
            q.set_windows(0, 100)
        assert e.value.status == V.capi.E_UNSUPPORTED and q.windows() is None and q.mismatches().tolist() == [1, 0, 2]
        q.set_windows(None, None)                                           # (removing windows that are not there is no refusal)
        assert q.mismatches().tolist() == [1, 0, 2]
    plain = V.Queries(["ACG"])
    plain.set_mismatches(1)
    plain.set_mismatches(None)
    plain.set_windows(0, 10)                                                # the batch is what it was: it takes windows again
    assert plain.windows() is not None


# ---- 1. intervals are the occurrences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dna3000", "zipf", "a100", "ab500"])
def test_intervals_are_the_occurrences(V, name):
    text = _text(name)
    rng = np.random.default_rng(len(text) + 1)
    alphabet = bytes(sorted(set(text))) + (b"z" if name in ("a100", "ab500") else b"")
    regexps, budgets = [], []
    for j in range(40):
        # zipf (40 symbols): m = 1, 2, 3, 4 in turn, each under all six budgets -- with k >= 3 and m >= 3 the frontier is every distinct
        # 3-gram of the text (thousands of entries, three levels of the miss count), which stays below ROOMY: at most n of them
        m = 1 + (j // 6) % 4 if name == "zipf" else int(rng.integers(1, 7))
        at = int(rng.integers(0, len(text) - m))
        budget = [0, 1, 2, 3, m, m + 2][j % 6]                              # 0 .. 3 and k >= m
        regexps.append(_regexp([_cut(text, rng, at, m, int(rng.integers(0, 3)), classes=j % 3 == 2, alphabet=alphabet)], []))
        budgets.append(budget)
    res = _index(V, name).search(_batch(V, regexps, budgets), workspace=_workspace({"class_intervals": ROOMY}))
    several = _check_intervals(name, regexps, budgets, res)
    if name in ("dna3000", "zipf"):
        assert several > 20                                                 # not vacuous: most sub-patterns have several intervals
    if name == "zipf":
        widest = int(np.diff(res.class_intervals()[0].astype(np.int64)).max())
        assert 1024 < len({text[i:i + 3] for i in range(len(text) - 2)}) <= widest <= len(text) < ROOMY


# ---- 2. whole searches against brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tuples", [1, 0])
def test_search_matches_brute_force(V, kind, tuples):
    ws = _workspace({"tuples": tuples, "filter_min": 0, "filter_stream_min": 0, "class_intervals": ROOMY})
    for name, mrange in (("dna3000", (4, 8)), ("zipf", (3, 6))):
        text = _text(name)
        rng = np.random.default_rng(17 + len(text))
        regexps, budgets = _random_queries(text, rng, 32, mrange=mrange, classes=True)
        assert {len(B.parse(r)[0]) for r in regexps} == {1, 2, 3, 5} and {0, 1, 2} == set(budgets)
        res, nonempty = _check_search(V, text, _index(V, name, kind), regexps, budgets, ws, bool(tuples))
        assert nonempty == len(regexps)                                     # every query has at least the match it was cut from
        # more substitutions than budget
        regexps, budgets = _random_queries(text, rng, 16, over=1, mrange=mrange)
        _check_search(V, text, _index(V, name, kind), regexps, budgets, ws, bool(tuples))
    # one batch: a sub-pattern under two budgets, a budget-0 sub-pattern beside a budgeted one, class positions under a budget
    text = _text("dna3000")
    p, c = text[100:106].decode(), text[130:135].decode()
    regexps = ["%s.{0,60}?%s" % (p, c), "%s.{0,60}?%s" % (p, c), "%s.{0,60}?%s" % (p, c), "%s[AC]%s.{0,60}?%s" % (p[:2], p[3:], c), "[CG]%s" % c[1:]]
    budgets = [1, 0, 2, 1, 0, 2, 1, 0, 2]
    res, nonempty = _check_search(V, text, _index(V, "dna3000", kind), regexps, budgets, ws, bool(tuples))
    assert nonempty == len(regexps)
    assert _check_intervals("dna3000", regexps, budgets, res) >= 5
    off = np.diff(res.class_intervals()[0].astype(np.int64))
    assert off[2] > off[0] > 1 == off[4] == off[1] and off[5] > off[3] > 1   # p and c under the budgets 1, 2 and 0: three lists each


# ---- 3. wave borders -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [63, 64, 65])
def test_wave_borders(V, sigma):
    """(symbol, parent) pairs of a step: sigma for the first (a wave less one, a wave, a wave and one), sigma^2 for the second of m = 2,
    k = 1, and sigma x (distinct 2-grams) for the third of m = 3, k = 2"""
    name = _sigma_text(sigma)
    text = _text(name)
    assert len(text) == 2000 and len(set(text)) == sigma
    idx = _index(V, name)
    two, three = [bytes([c]) for c in text[700:702]], [bytes([c]) for c in text[900:903]]
    w2, w3 = A.frontier_widths(text, [B.row(c) for c in two], 1), A.frontier_widths(text, [B.row(c) for c in three], 2)
    assert w2[0] == sigma and sigma * w2[0] >= 63 * 63                     # step 1 deals sigma pairs and keeps them all; step 2 deals sigma^2
    assert w3[0] == sigma and w3[1] > 1024 and w3[1] == len({text[i:i + 2] for i in range(len(text) - 1)})
    regexps = [_regexp([two], []), _regexp([three], []), _regexp([two, three], [(0, 400)])]
    budgets = [1, 2, 1, 2]
    ws = _workspace({"class_intervals": max(w2 + w3)})
    res, nonempty = _check_search(V, text, idx, regexps, budgets, ws)
    assert nonempty == 3
    _check_intervals(name, regexps, budgets, res)
    assert np.diff(res.class_intervals()[0].astype(np.int64)).tolist() == [w2[-1], w3[-1], w2[-1], w3[-1]]


# ---- 4. the cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(1, 1), (4, 3)])
def test_frontier_cap(V, m, k):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    sub = [bytes([c]) for c in text[50:50 + m]]
    widths = A.frontier_widths(text, [B.row(c) for c in sub], k)
    cap = max(widths)
    assert cap == 4 if m == 1 else cap >= 64
    regexps = ["A.{0,20}?C", _regexp([[b"A"], sub], [(0, 20)])]
    budgets = [0, 0, 0, k]
    ws = _workspace({"class_intervals": cap})
    res, nonempty = _check_search(V, text, idx, regexps, budgets, ws)                                      # exactly `cap` is legal
    assert nonempty == 2 and int(np.diff(res.class_intervals()[0].astype(np.int64)).max()) == widths[-1]
    ws.set_option("class_intervals", cap - 1)
    with pytest.raises(V.VlgError) as e:
        idx.search(_batch(V, regexps, budgets), workspace=ws)
    assert e.value.status == V.capi.E_WORKSPACE
    assert "query 1" in str(e.value) and "sub-pattern 1" in str(e.value) and "class_intervals" in str(e.value)
    ws.set_option("class_intervals", cap)
    res, nonempty = _check_search(V, text, idx, regexps, budgets, ws)                                      # the workspace answers the next batch
    assert nonempty == 2


# ---- 5. budgets of zero take the existing paths ----------------------------------------------------------------------------------------
def test_zero_budgets_take_the_existing_paths(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    rng = np.random.default_rng(10)
    plain = []
    for j in range(64):
        a, b = rng.integers(0, len(text) - 40, size=2)
        plain.append("%s.{0,%d}?%s" % (text[a:a + 3].decode(), 10 + j, text[b:b + 2 + j % 3].decode()))
    classes = [r.replace("A", "[AC]", 1) for r in plain]
    for make, literal in ((lambda: V.Queries(plain), True), (lambda: V.Queries.from_classes(classes), False)):
        ws1, ws2 = _workspace(), _workspace()
        q = make()
        q.set_mismatches(0)
        got, want = idx.search(q, workspace=ws1), idx.search(make(), workspace=ws2)
        assert got.summary == want.summary and got.summary["n_matches"] > 50
        for a, b in zip(got.fetch(), want.fetch()):
            assert a.tolist() == b.tolist()
        k1, k2 = ws1.kernel_stats(), ws2.kernel_stats()
        assert {k: v["launches"] for k, v in k1.items()} == {k: v["launches"] for k, v in k2.items()}
        assert (k1["class_search"]["launches"] == 0) == literal
        # a budget was there and is gone: the batch is what it was
        q.set_mismatches(1)
        q.set_mismatches(None)
        again = idx.search(q, workspace=_workspace())
        assert again.summary == want.summary
        if literal:
            q.set_mismatches(1)
            idx.search(q, workspace=ws1)
            assert ws1.kernel_stats()["class_search"]["launches"] > 0


# ---- 6. shapes --------------------------------------------------------------------------------------------------------------------------
def test_shapes(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    ws = _workspace()
    regexps = ["AZG", "AZG", "Z", "Z", "ZZ", "A", "ACGZ.{0,9}?T\xf0", "A" * 3001]
    budgets = [1, 0, 1, 0, 1, 1, 1, 1, 2]
    res, _ = _check_search(V, text, idx, regexps, budgets, ws)
    _check_intervals("dna3000", regexps, budgets, res)
    n = len(text)
    assert int(res.counts[0]) > 0 and int(res.counts[1]) == 0               # a byte the text lacks is a forced miss
    assert int(res.counts[2]) == n and int(res.counts[5]) == n              # m = 1, k = 1: every position
    assert int(res.counts[3]) == 0 and int(res.counts[4]) == 0 and int(res.counts[7]) == 0    # (m > n: nowhere, whatever the budget)
    # sigma == 1: one symbol beside the sentinel
    a = _text("a100")
    regexps = ["b", "ab", "bb", "b", "ab", "bb", "bb", "a" * 101]
    budgets = [1, 1, 1, 2, 2, 2, 0, 1]
    res, _ = _check_search(V, a, _index(V, "a100"), regexps, budgets, ws)
    assert res.counts.tolist() == [100, 50, 0, 100, 50, 50, 0, 0]
    _check_intervals("a100", regexps, budgets, res)
    ab = _text("ab500")
    regexps = ["aa", "bb", "ab", "abab.{0,0}?ba", "bbb", "aba"]
    budgets = [1, 1, 1, 2, 0, 1, 3]
    res, _ = _check_search(V, ab, _index(V, "ab500"), regexps, budgets, ws)
    assert res.counts.tolist() == [500, 500, 500, 0, 250, 333]
    _check_intervals("ab500", regexps, budgets, res)


# ---- 7. wide SA indices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", ["1", "2"])
def test_wide_sa_indices(V, monkeypatch, force):
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text = _text("dna3000")
    idx = V.VlgIndex.build(text)
    assert idx.info()["pos_bytes"] == 8
    regexps, budgets = _random_queries(text, np.random.default_rng(17 + len(text)), 32, mrange=(4, 8), classes=True)
    res, nonempty = _check_search(V, text, idx, regexps, budgets, _workspace({"class_intervals": ROOMY}))
    assert nonempty == 32
    _check_intervals("dna3000", regexps, budgets, res)


# ---- 8. super-chunks ----------------------------------------------------------------------------------------------------------------------
def test_super_chunks(V):
    text = _text("dna40000")
    idx = _index(V, "dna40000")
    mers = [a + b for a in "ACGT" for b in "ACGT"]
    regexps = ["%s.{%d,%d}?%s" % (mers[j], 3 + j, 9 + j, mers[(j + 5) % 16]) for j in range(16)]
    small = _workspace(cap=17 << 20)
    res, nonempty = _check_search(V, text, idx, regexps, 1, small)
    assert nonempty == 16 and res.summary["n_chunks"] >= 2
    # the lists of all queries do not fit the physical budget of this cap at once: 25 bytes per occurrence, half of cap - 8 MiB
    assert res.summary["located_occurrences"] > ((17 << 20) - (8 << 20)) // 2 // 25
    big = idx.search(_batch(V, regexps, 1), workspace=_workspace())
    assert big.fetch()[3].tolist() == res.fetch()[3].tolist() and big.summary["checksum"] == res.summary["checksum"]
    assert big.summary["n_matches"] == res.summary["n_matches"] > 1000


# ---- 9. a workspace on its own stream ------------------------------------------------------------------------------------------------------
def test_workspace_with_its_own_stream(V):
    import torch
    text = _text("zipf")
    regexps, budgets = _random_queries(text, np.random.default_rng(34), 32, mrange=(3, 6), classes=True)
    stream = torch.cuda.Stream()
    own = _workspace({"class_intervals": ROOMY}, stream=C.c_void_p(stream.cuda_stream))
    res, nonempty = _check_search(V, text, _index(V, "zipf"), regexps, budgets, own)
    null = _index(V, "zipf").search(_batch(V, regexps, budgets), workspace=_workspace({"class_intervals": ROOMY}))
    assert nonempty == 32 and res.summary == null.summary
    for a, b in zip(res.fetch(), null.fetch()):
        assert a.tolist() == b.tolist()
    for a, b in zip(res.class_intervals(), null.class_intervals()):
        assert a.tolist() == b.tolist()


# ---- 10. shared sub-patterns ----------------------------------------------------------------------------------------------------------------
def test_shared_lists_are_searched_and_located_once(V):
    text = _text("dna3000")
    subs = ["ACGT", "TTGA", "GGC", "CATG", "AAT"]
    rng = np.random.default_rng(3)
    regexps, budgets, pairs = [], [], []
    for j in range(200):
        i, k = (int(x) for x in rng.choice(5, size=2))
        regexps.append("%s.{0,%d}?%s" % (subs[i], 20 + j % 7, subs[k]))
        pairs += [(subs[i], i % 3), (subs[k], 1 + k % 2)]                   # the budget follows from the string and the place: few distinct pairs
    budgets = [b for _, b in pairs]
    ws = _workspace()
    res, nonempty = _check_search(V, text, _index(V, "dna3000"), regexps, budgets, ws)
    assert nonempty > 100
    assert len(set(pairs)) == 9 and {b for _, b in pairs} == {0, 1, 2}
    occ = {p: len(A.approx_occurrences(text, [B.row(bytes([c])) for c in p[0].encode()], p[1])) for p in set(pairs)}
    assert res.summary["located_occurrences"] == sum(occ.values())
    live = [i for i in range(200) if occ[pairs[2 * i]] and occ[pairs[2 * i + 1]]]
    assert res.summary["logical_occurrences"] == sum(occ[pairs[2 * i]] + occ[pairs[2 * i + 1]] for i in live)
    assert ws.kernel_stats()["class_search"]["launches"] == 1


def test_effective_budget_makes_the_distinct_list(V):
    """min(k, m) is part of a distinct sub-pattern's key: budgets m, m + 2 and 255 on one string are ONE list, searched and located once"""
    text = _text("dna3000")
    n = len(text)
    regexps = ["ACG.{0,9}?ACG", "ACG.{0,9}?ACG.{0,9}?TTGA"]
    every3, every4 = n - 2, n - 3                                           # k >= m: every position that fits
    ws = _workspace({"class_intervals": ROOMY})
    res, nonempty = _check_search(V, text, _index(V, "dna3000"), regexps, [3, 5, 255, 3, 4], ws)
    assert nonempty == 2 and res.summary["located_occurrences"] == every3 + every4          # (ACG, 3) and (TTGA, 4), whatever k >= m says
    assert ws.kernel_stats()["class_search"]["launches"] == 1
    off = np.diff(res.class_intervals()[0].astype(np.int64))
    assert off[0] == off[1] == off[2] == off[3] == len({text[i:i + 3] for i in range(n - 2)})
    two = len(A.approx_occurrences(text, [B.row(bytes([c])) for c in b"ACG"], 2))
    res, _ = _check_search(V, text, _index(V, "dna3000"), regexps, [3, 5, 255, 2, 4], _workspace({"class_intervals": ROOMY}))
    assert two < every3 and res.summary["located_occurrences"] == every3 + two + every4  # a budget below m is another list


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(V):
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    q = V.Queries(["ACGT", "AC.{0,4}?GT"])
    q.set_mismatches(1)
    ws = _workspace()
    idx.search(q, workspace=ws)
    before = ws.kernel_stats()
    with pytest.raises(V.VlgError) as e:
        q.set_windows(0, 100)
    assert e.value.status == V.capi.E_UNSUPPORTED and q.windows() is None
    qw = V.Queries(["ACGT", "AC.{0,4}?GT"])
    qw.set_windows(0, 100)
    with pytest.raises(V.VlgError) as e:
        qw.set_mismatches(1)
    assert e.value.status == V.capi.E_UNSUPPORTED and qw.mismatches() is None and qw.windows() is not None
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


# ---- 12. the group loop: more tasks than one group of the frontier scratch holds ---------------------------------------------------------------
GROUP_CAP = 1 << 20                # "class_intervals" at its maximum: 64 MiB of frontier scratch / (32 B x 2^20) = 2 tasks to a group


def _group_batch(text):
    """-> (regexps, budgets): 5 distinct class sub-patterns, 5 distinct budgeted ones (budgets 1 and 2; two of them over classes) and 2
    literal ones, repeated over 9 queries"""
    cls = ["[AC]G", "T[CG]A", "[AT][AT]", "[^A]C", "GG[ACT]"]
    apx = [("ACGT", 1), ("TTGA", 2), ("GGC", 1), ("CA[GT]G", 2), ("[AC]AT", 1)]
    lit = ["ACG", "TTG"]
    subs = [(c, 0) for c in cls] + apx + [(x, 0) for x in lit]
    order = [(0, 5), (1, 6, 10), (2, 7), (3, 8, 11), (4, 9), (0, 9, 1), (5, 10), (6, 2, 8), (11, 7, 3)]
    regexps = [".{0,40}?".join(subs[i][0] for i in q) for q in order]
    budgets = [subs[i][1] for q in order for i in q]
    widths = [max(A.frontier_widths(text, rows, k)) for (rx, k) in subs for rows in B.parse(rx)[0]]
    assert max(widths) < 1024, widths                                       # the comparison run at the default cap does not overflow
    assert len(set(order[j][i] for j in range(len(order)) for i in range(len(order[j])))) == 12 < len(budgets)
    return regexps, budgets


def test_task_groups(V):
    """g0 of the group loop: the tasks, the ids and the rows of the strided frontier copy of every group but the first"""
    text = _text("dna3000")
    idx = _index(V, "dna3000")
    regexps, budgets = _group_batch(text)
    ws = _workspace({"class_intervals": GROUP_CAP})
    res, nonempty = _check_search(V, text, idx, regexps, budgets, ws)
    assert nonempty >= 5
    _check_intervals("dna3000", regexps, budgets, res)
    assert ws.kernel_stats()["class_search"]["launches"] == 6               # ceil(5 / 2) for the class kind + ceil(5 / 2) for the budgeted kind
    ws2 = _workspace()
    small = idx.search(_batch(V, regexps, budgets), workspace=ws2)
    assert ws2.kernel_stats()["class_search"]["launches"] == 2              # (one group per kind at the default cap)
    assert small.summary == res.summary
    for a, b in zip(res.fetch(), small.fetch()):
        assert a.tolist() == b.tolist()
    for a, b in zip(res.class_intervals(), small.class_intervals()):
        assert a.tolist() == b.tolist()


# ---- 13. recorded behaviour (the fixture of tests/test_gpu_query_classes.py) ---------------------------------------------------------------------
def _recorded_cases(V):
    text = _text("dna3000")
    regexps, budgets = _random_queries(text, np.random.default_rng(17 + len(text)), 32, mrange=(4, 8), classes=True)   # test_search_matches_brute_force's
    opts = {"tuples": 1, "filter_min": 0, "filter_stream_min": 0, "class_intervals": ROOMY}
    mers = [a + b for a in "ACGT" for b in "ACGT"]
    chunked = ["%s.{%d,%d}?%s" % (mers[j], 3 + j, 9 + j, mers[(j + 5) % 16]) for j in range(16)]                      # test_super_chunks's

    def run(name, kind, regexps, budgets, opts, cap):
        ws = _workspace(opts, cap=cap)
        return K._observe(_index(V, name, kind).search(_batch(V, regexps, budgets), workspace=ws), ws)
    cases = {"budgets/dna3000/" + kind: (lambda kind=kind: run("dna3000", kind, regexps, budgets, opts, 1 << 30)) for kind in ("plain", "rrr")}
    cases["budgets/dna40000/super_chunks"] = lambda: run("dna40000", "plain", chunked, 1, None, 17 << 20)
    return cases


def test_recorded_behaviour(V):
    K._check_recorded(_recorded_cases(V))
