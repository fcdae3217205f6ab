"""Document-bounded search (vlg_documents + vlg_queries_set_documents): for every document in turn, a query has exactly the matches
it has on that document alone, shifted by the document's start.  The yardstick is tests/vlg_brute.py per document -- the document
semantics are the window semantics -- and, on the device, the windowed batch with one entry per (query, document).  The cases are
built and shown non-vacuous on the CPU before the GPU is touched."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vlg_approx_brute as A
import vlg_class_brute as B
from test_gpu_search_window import OPTION_ROWS, _workspace
from test_gpu_wtsa_window import _brute_window, _check, _random_int_queries, _random_queries
from util import dna_text
from vlg_brute import lazy_matches, occurrences
from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
BENCH = 1                                   # VLG_DIALECT_BENCHMARK


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def _doc_matches(lists, ms, lo, hi, end_len, starts, n):
    """lists[i]: every occurrence of sub-pattern i (m = ms[i] symbols) in the whole text.  -> for j ascending, the matches on document
    j alone: the occurrences that lie wholly inside it are the occurrences of the stand-alone document (shifted)."""
    bounds = list(starts) + [n]
    arr = [np.asarray(l, dtype=np.uint64) for l in lists]
    out = []
    for b, e in zip(bounds[:-1], bounds[1:]):
        cut = []
        for a, m in zip(arr, ms):
            if e - b < m:
                cut = None
                break
            cut.append(a[np.searchsorted(a, b):np.searchsorted(a, e - m + 1)])
        if cut is None or any(len(c) == 0 for c in cut):
            continue
        out += lazy_matches(cut, lo, hi, end_len)
    return out


def _brute_docs(text, f, starts, occ_memo):
    subs, lo, hi, end_len = f
    lists = []
    for s in subs:
        key = bytes(s) if isinstance(s, (bytes, bytearray)) else np.asarray(s).tobytes()
        if key not in occ_memo:
            occ_memo[key] = occurrences(text, s)
        lists.append(occ_memo[key])
    return _doc_matches(lists, [len(s) for s in subs], lo, hi, end_len, starts, len(text))


# ---- texts, queries, document sets ---------------------------------------------------------------------------------------------
TEXTS = ["dna3000", "abab", "ints"]


def _text(name):
    if name == "dna3000":
        return dna_text(3000, 31).tobytes()
    if name == "abab":
        return b"ab" * 3000
    rng = np.random.default_rng(12)                                          # the integer text of test_gpu_search_window.py
    vocab = np.array([1, 2, 3, 7, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.uint64)
    return vocab[rng.choice(len(vocab), 1500)].astype(np.uint32)


def _to_bench(q):
    return q.replace("}?", "}")


def _doc_sets(text, fields, rng):
    n = len(text)
    # two documents: of the boundaries around the middle, the one that cuts through a match of the most queries
    memo = {}
    whole = [_brute_docs(text, f, [0], memo) for f in fields]
    cut = max(range(n // 2 - 8, n // 2 + 8), key=lambda b: sum(_brute_docs(text, f, [0, b], memo) != w for f, w in zip(fields, whole)))
    sets = {"one": [0], "two": [0, cut]}
    sets["64"] = sorted({0} | {int(x) for x in np.linspace(0, n, 65)[1:-1]})
    sets["65"] = sorted({0} | {int(x) for x in np.linspace(0, n, 66)[1:-1]})
    sets["every7"] = list(range(0, n, 7))
    on = {0}
    for f in fields[:12]:                                                    # on an occurrence start, on its last symbol, one past it
        subs = f[0]
        for i in sorted({0, len(subs) // 2, len(subs) - 1}):
            occ = occurrences(text, subs[i])
            if len(occ):
                p, m = int(occ[len(occ) // 2]), len(subs[i])
                on |= {p, p + m - 1, p + m}
    sets["on_occurrence"] = sorted(x for x in on if x < n)
    r = sorted({0} | {int(x) for x in rng.integers(1, n, n // 40)})
    sets["random"] = r
    p = int(rng.integers(n // 3, n // 2))
    sets["one_symbol"] = sorted(set(r[: len(r) // 2]) | {p, p + 1, n - 1})       # [p, p + 1) and the text's last symbol are documents
    assert len(sets["64"]) == 64 and len(sets["65"]) == 65
    return sets


_cases = {}


def _case(name):
    """-> (text, [(dialect, regexps or None, fields)], {set: starts}, {(batch, set): expected per query}).  CPU only; computed once.
    Non-vacuity: for every document set but the single document more than 1/8 of the queries have a match, more than 1/8 differ from
    their answer on the undivided text, one loses a match and one gains a match the undivided answer had skipped."""
    if name in _cases:
        return _cases[name]
    import vlg_matching_amd as V
    text = _text(name)
    rng = np.random.default_rng({"dna3000": 5, "abab": 6, "ints": 7}[name])
    if name == "ints":
        qs, fields = _random_int_queries(text, rng, 48, mmax=2, gapmax=30, gaplo=4)
        batches = [("int", qs, fields)]
    else:
        # (short sub-patterns and gaps of up to 30: matches are dense and wide, so that even ONE boundary cuts through a match of
        # many queries -- and moves every later match of the document behind it)
        qs = _random_queries(text, rng, 48, kmax=4, mmax=4 if name == "abab" else 2, gapmax=30, gaplo=4)
        qb = [_to_bench(q) for q in qs]
        batches = [("library", qs, [V.parse_query(q) for q in qs]), ("benchmark", qb, [V.parse_query(q, BENCH) for q in qb])]
    assert {len(f[0]) for f in batches[0][2]} == {1, 2, 3, 4}
    sets = _doc_sets(text, batches[0][2], rng)
    want = {}
    for kind, reps, fields in batches:
        memo = {}
        whole = [_brute_docs(text, f, [0], memo) for f in fields]
        assert whole == [_brute_window(text, f, 0, len(text)) for f in fields]
        for sname, starts in sets.items():
            w = [_brute_docs(text, f, starts, memo) for f in fields]
            if sname == "two":                                                   # the yardstick itself: one brute force per document
                assert w == [_brute_window(text, f, 0, starts[1]) + _brute_window(text, f, starts[1], len(text)) for f in fields]
            want[(kind, sname)] = w
            if sname == "one":
                assert w == whole
                continue
            nq = len(fields)
            assert sum(1 for x in w if x) > nq // 8, (name, kind, sname)
            assert sum(1 for x, y in zip(w, whole) if x != y) > nq // 8, (name, kind, sname)
            lost = any(any(t not in x for t in y) for x, y in zip(w, whole))
            gained = any(any(t not in y for t in x) for x, y in zip(w, whole))
            assert lost and gained, (name, kind, sname, lost, gained)
    _cases[name] = (text, batches, sets, want)
    return _cases[name]


def _make(V, kind, reps):
    if kind == "int":
        return V.index.Queries.from_int(reps)
    return V.index.Queries(reps, dialect=BENCH if kind == "benchmark" else V.capi.DIALECT_LIBRARY)


def _build(V, text):
    return V.VlgIndex.build_int(text) if isinstance(text, np.ndarray) else V.VlgIndex.build(text)


def _search_both(idx, batch, want, opts, ran=None):
    res = idx.search(batch, workspace=_workspace(opts))
    _check(res, want)
    _check(idx.search(batch, workspace=_workspace(dict(opts, tuples=0))), want, tuples=False)
    if ran:
        assert sum(res.summary[f] for f in ran) > 0, (opts, res.summary)
    return res


# ---- brute force ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TEXTS)
def test_documents_against_brute_force(V, name):
    """Counts, first positions, tuples, n_matches and checksum, with and without tuples: plain, rrr, text-order and d = 1 indexes
    under the default options, every row of workspace options on the plain index (the rows that name a filter kind with the proof
    that it ran), and "fuse_jump" = 0."""
    text, batches, sets, want = _case(name)                                  # (asserts non-vacuity before the GPU is touched)
    plain = _build(V, text)
    variants_ = [plain, plain.compress(), plain.resample(text_order=True, dens=7), plain.resample(text_order=False, dens=1)]
    for kind, reps, fields in batches:
        batch = _make(V, kind, reps)
        for sname, starts in sets.items():
            docs = V.Documents.from_starts(starts, len(text))
            assert docs.count() == len(starts)
            batch.set_documents(docs)
            w = want[(kind, sname)]
            for idx in variants_:
                _search_both(idx, batch, w, {})
            _search_both(plain, batch, w, {"fuse_jump": 0})
            for opts, ran in OPTION_ROWS[1:]:
                _search_both(plain, batch, w, opts, ran)
        batch.set_documents(None)


@pytest.mark.parametrize("name", TEXTS)
def test_documents_equal_the_windowed_batch(V, name):
    """the same device, one batch entry per (query, document): the per-query concatenation is identical, tuples included"""
    text, batches, sets, want = _case(name)
    idx = _build(V, text)
    for kind, reps, fields in batches:
        for sname in ("two", "65", "random"):
            starts = sets[sname]
            bounds = starts + [len(text)]
            pairs = [(j, b, e) for j in range(len(reps)) for b, e in zip(bounds[:-1], bounds[1:])]
            wb = _make(V, kind, [reps[j] for j, _, _ in pairs])
            wb.set_windows([b for _, b, _ in pairs], [e for _, _, e in pairs])
            win = idx.search(wb)
            batch = _make(V, kind, reps)
            batch.set_documents(V.Documents.from_starts(starts, len(text)))
            doc = idx.search(batch)
            d = len(starts)
            for j in range(len(reps)):
                cat = [t for i in range(j * d, (j + 1) * d) for t in win.tuples(i).tolist()]
                assert doc.tuples(j).tolist() == cat, (kind, sname, j)
            assert doc.summary["n_matches"] == win.summary["n_matches"] and doc.summary["checksum"] == win.summary["checksum"]


# ---- boundaries inside the kernel's steps ----------------------------------------------------------------------------------------
def _step_case(V):
    """"ab" stands at 2 i on the periodic text, so element e of its list sits at 2 e and a start at 2 e cuts the list in front of
    element e: inside a 128-key pair (e = 30, 100), between two 64-slot steps (64, 128), at the run border of the loaded library
    (VLG_LINK_RUN, and one element to either side), at a segment border (the last element of one query's list is followed by the
    first of the next query's).  A query of one sub-pattern, queries whose level-0 lists follow each other (segment borders inside a
    step: 3000 is no multiple of 64), and a benchmark-dialect query with |s_0| = 4 > |s_1| = 1."""
    R = V.capi.build_constants()["VLG_LINK_RUN"]
    text = b"ab" * 3000
    es = sorted({1, 30, 64, 100, 128, R - 1, R, R + 1, 2 * R, 2999} & set(range(1, 3000)))
    starts = sorted({0} | {2 * e for e in es} | {2 * 30 + 1, 2 * R + 1, 5997})
    lib_qs = ["ab", "ab.{0,2}?ab", "ab.{1,5}?b.{0,3}?a", "a", "ba.{0,4}?ab", "abab.{0,9}?ba"]
    bench_qs = ["abab.{0,3}b", "ab", "ab.{0,2}ab"]
    return text, starts, lib_qs, bench_qs


def test_boundaries_inside_the_steps_of_the_link_pass(V):
    text, starts, lib_qs, bench_qs = _step_case(V)
    memo = {}
    lf = [V.parse_query(q) for q in lib_qs]
    bf = [V.parse_query(q, BENCH) for q in bench_qs]
    wl = [_brute_docs(text, f, starts, memo) for f in lf]
    wb = [_brute_docs(text, f, starts, memo) for f in bf]
    # the benchmark query: somewhere a match ends within |s_0| of a boundary and the next document's first match begins ON the boundary
    # -- the restart key computed globally (end + 4) would skip it
    first = {t[0] for t in wb[0]}
    assert any(b in first and any(t[-1] < b < t[-1] + 4 for t in wb[0]) for b in starts[1:])
    whole = [_brute_docs(text, f, [0], memo) for f in lf + bf]
    # (a sub-pattern of one symbol crosses nothing: "a" alone has the answer of the undivided text)
    assert all((x != y) == (q != "a") for q, x, y in zip(lib_qs + bench_qs, wl + wb, whole)) and all(wl) and all(wb)
    idx = V.VlgIndex.build(text)
    docs = V.Documents.from_starts(starts, len(text))
    for reps, want, dialect in ((lib_qs, wl, V.capi.DIALECT_LIBRARY), (bench_qs, wb, BENCH)):
        batch = V.index.Queries(reps, dialect=dialect)
        batch.set_documents(docs)
        for opts in ({"filter": 0}, {}, {"filter": 0, "fuse_jump": 0}, {"fuse_jump": 0}):
            res = _search_both(idx, batch, want, opts)
        assert res.summary["join_slots"] > 2048                              # lists longer than one link run of the default build


def test_small_variant_runs_the_step_cases():
    """VLG_LINK_RUN = 192: the same cases in a child pytest that loads the `small` build -- runs of three steps, so the boundaries at
    R - 1, R, R + 1 fall at a run border that ends inside a pair, and the periodic lists cross 31 run borders"""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_LINK_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_documents.py", "-k", "inside_the_steps or abab"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= 3, tail


# ---- classes and budgets -------------------------------------------------------------------------------------------------------
def _class_expected(text, regexp, ks, starts):
    subs, lo, hi, end = B.parse(regexp)
    lists = [A.approx_occurrences(text, s, k) for s, k in zip(subs, ks)]
    return _doc_matches(lists, [len(s) for s in subs], lo, hi, end, starts, len(text))


def _check_tuples(res, want):
    for i, w in enumerate(want):
        assert res.tuples(i).tolist() == w, i
    flat = [t for w in want for t in w]
    assert res.summary["n_matches"] == len(flat) and res.summary["checksum"] == sum(t[0] for t in flat) % (1 << 64)


CLASS_REGEXPS = ["A[CG]T", "[AC][GT].{0,6}?T[AT]", "AC.{2,9}?[ACG]T.{0,4}?G", "[^A]C[^G]", "G[AT]TA.{0,12}?[CT]A", "T.{1,7}?[AG][AG]"]


def _class_cases():
    """-> (text, [(budgets, starts, expected per query)]): CPU only.  Not vacuous: at least half of the queries have a match, and
    differ from their answer on the undivided text (one query at least where a single boundary is all there is)."""
    text = dna_text(3000, 31).tobytes()
    rng = np.random.default_rng(3)
    nsub = sum(len(B.parse(r)[0]) for r in CLASS_REGEXPS)
    sets = {"two": [0, 1501], "every7": list(range(0, 3000, 7)), "random": sorted({0} | {int(x) for x in rng.integers(1, 3000, 75)})}
    out = []
    for budgets in ([0] * nsub, [int(x) for x in rng.integers(0, 3, nsub)]):
        per, s = [], 0
        for r in CLASS_REGEXPS:
            k = len(B.parse(r)[0])
            per.append(budgets[s:s + k])
            s += k
        whole = [_class_expected(text, r, ks, [0]) for r, ks in zip(CLASS_REGEXPS, per)]
        for sname, starts in sets.items():
            want = [_class_expected(text, r, ks, starts) for r, ks in zip(CLASS_REGEXPS, per)]
            differ = sum(1 for x, y in zip(want, whole) if x != y)
            assert sum(1 for w in want if w) >= 3 and differ >= (1 if sname == "two" else 3), (sname, differ)
            out.append((budgets, starts, want))
    assert max(out[-1][0]) == 2
    return text, out


def test_classes_and_budgets(V):
    """a[bc]d-style batches and budgets k <= 2, per document by tests/vlg_class_brute.py / vlg_approx_brute.py"""
    text, cases = _class_cases()
    idx = V.VlgIndex.build(text)
    for budgets, starts, want in cases:
        q = V.Queries.from_classes(CLASS_REGEXPS)
        q.set_mismatches(budgets)
        q.set_documents(V.Documents.from_starts(starts, len(text)))
        _check_tuples(idx.search(q), want)
        _check_tuples(idx.search(q, workspace=_workspace({"fuse_jump": 0})), want)


def _separator_case():
    rng = np.random.default_rng(8)
    text = bytes(rng.choice(np.frombuffer(b"aabbc\n", dtype=np.uint8), 2000))
    starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10 and i + 1 < len(text)]
    regexps = ["[^a]b", "a[^a][^a]", "[^a].{0,3}?[^a]b", "[^b][^a].{1,4}?[^a]", "b[^a]"]
    want = [_class_expected(text, r, [0] * len(B.parse(r)[0]), starts) for r in regexps]
    whole = [_class_expected(text, r, [0] * len(B.parse(r)[0]), [0]) for r in regexps]
    # ("b[^a]" crosses no boundary: only its LAST position accepts the newline, and the newline closes the document)
    assert all(want) and [x != y for x, y in zip(want, whole)] == [True, True, True, True, False]
    m_last = [len(B.parse(r)[0][-1]) for r in regexps]
    assert any(text[t[-1] + m - 1] == 10 for w, m in zip(want, m_last) for t in w)      # some match ends ON its newline
    return text, starts, regexps, want


def test_separator_closes_its_document(V):
    """from_separator(text, b"\\n") with [^a] classes that accept the separator: a line's match may end ON its newline, never behind it"""
    text, starts, regexps, want = _separator_case()
    docs = V.Documents.from_separator(text, b"\n")
    assert docs.count() == len(starts) > 100
    q = V.Queries.from_classes(regexps)
    q.set_documents(docs)
    _check_tuples(V.VlgIndex.build(text).search(q), want)
    d, off = docs.locate(np.arange(len(text)))
    assert d.tolist() == [int(np.searchsorted(starts, i, side="right")) - 1 for i in range(len(text))]


# ---- a single document is a no-op; set / get; refusals -----------------------------------------------------------------------------
def test_a_single_document_changes_nothing(V):
    text, batches, sets, want = _case("dna3000")
    idx = _build(V, text)
    for kind, reps, fields in batches:
        ws = _workspace({})
        old = idx.search(_make(V, kind, reps), workspace=ws)
        batch = _make(V, kind, reps)
        batch.set_documents(V.Documents.from_starts([0], len(text)))
        new = idx.search(batch, workspace=ws)
        assert new.summary == old.summary
        for x, y in zip(new.fetch(), old.fetch()):
            assert x.tolist() == y.tolist()
        batch.set_documents(None)                                            # ... and a batch whose documents were removed is a fresh batch
        again = idx.search(batch, workspace=ws)
        assert again.summary == old.summary


def test_set_get_and_the_exclusion_of_windows(V):
    text = dna_text(3000, 31).tobytes()
    qs = ["AC", "A.{0,5}?C"]
    docs = V.Documents.from_starts([0, 100, 2000], len(text))
    batch = V.index.Queries(qs)
    assert batch.documents() is None
    batch.set_documents(docs)
    assert batch.documents() is docs
    h = C.c_void_p()
    V.capi.check(V.lib().vlg_queries_get_documents(batch._h, C.byref(h)))
    assert h.value == docs._h.value
    with pytest.raises(V.VlgError) as err:                                   # documents first: windows are refused, the batch unchanged
        batch.set_windows(1, 9)
    assert err.value.status == V.capi.E_UNSUPPORTED and batch.windows() is None and batch.documents() is docs
    batch.set_documents(None)
    assert batch.documents() is None
    batch.set_windows(1, 9)                                                  # windows first: documents are refused, the batch unchanged
    with pytest.raises(V.VlgError) as err:
        batch.set_documents(docs)
    assert err.value.status == V.capi.E_UNSUPPORTED and batch.documents() is None
    assert [a.tolist() for a in batch.windows()] == [[1, 1], [9, 9]]
    with pytest.raises(TypeError):
        batch.set_documents([0, 5])


def test_locate_batch(V):
    n = 700
    starts = [0, 1, 2, 63, 64, 65, 300, 699]
    docs = V.Documents.from_starts(starts, n)
    pos = np.arange(n + 3, dtype=np.uint64)
    d, off = docs.locate(pos)
    for x in range(n):
        j = max(i for i, s in enumerate(starts) if s <= x)
        assert (int(d[x]), int(off[x])) == (j, x - starts[j]), x
    assert d[n:].tolist() == [U64] * 3 and off[n:].tolist() == [U64] * 3     # n_text and beyond
    assert docs.locate(n - 1) == (7, 0) and docs.locate(n) == (U64, U64) and docs.locate(64) == (4, 0)
    many = V.Documents.from_starts(list(range(0, 5000, 3)), 5000)            # more than one block of fences
    d, off = many.locate(np.arange(5000))
    assert d.tolist() == [x // 3 for x in range(5000)] and off.tolist() == [x % 3 for x in range(5000)]


def test_refusals_at_search_time(V):
    """an n_text that is not the index's, a collective workspace, the lazy index: refused, and nothing has been launched"""
    text = dna_text(3000, 31).tobytes()
    idx, lazy = V.VlgIndex.build(text), V.WtsaIndex(text)
    batch = V.index.Queries(["AC", "A.{0,5}?C"])
    batch.set_documents(V.Documents.from_starts([0, 50], len(text) + 1))
    ws = _workspace({})
    before = ws.kernel_stats()
    with pytest.raises(V.VlgError) as err:
        idx.search(batch, workspace=ws)
    assert err.value.status == V.capi.E_INVALID and ws.kernel_stats() == before
    batch.set_documents(V.Documents.from_starts([0, 50], len(text)))
    calls = []
    xws = _workspace({})
    xws.set_exchange(2, 0, lambda *a: calls.append(a) or 0)
    before = xws.kernel_stats()
    with pytest.raises(V.VlgError) as err:
        idx.search(batch, workspace=xws)
    assert err.value.status == V.capi.E_UNSUPPORTED and not calls
    assert xws.kernel_stats() == before and all(v["launches"] == 0 for v in before.values())
    h = C.c_void_p()
    before = ws.kernel_stats()
    assert V.lib().vlg_wtsa_search_batch(lazy._h, batch._h, 0, ws._h, C.byref(h)) == V.capi.E_UNSUPPORTED and not h.value
    z = np.zeros(2, np.uint64)
    assert V.lib().vlg_wtsa_search_window_batch(lazy._h, batch._h, z.ctypes.data, None, 0, ws._h, C.byref(h)) == V.capi.E_UNSUPPORTED and not h.value
    assert ws.kernel_stats() == before
    _check(idx.search(batch), [_brute_docs(text, V.parse_query(q), [0, 50], {}) for q in ["AC", "A.{0,5}?C"]])
