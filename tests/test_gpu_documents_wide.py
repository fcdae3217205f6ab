"""Document-bounded search on the 64-bit position kernels (VLG_FORCE_POS64 with vlg_queries_set_documents): "1" runs
run_batch<uint64_t> -- join_init_docs_kernel, join_link_docs_kernel, join_jump_docs_kernel, restart_key and doc_window on 8-byte
positions, and the pair search that loads a window when it turns to it, which the default build compiles for this combination
alone -- and "2" the 32-bit document kernels behind the wide locate (33-bit SA indices, the widths of a text of 2^32 + 1 symbols).
The yardstick is tests/vlg_brute.py per document through the builders of test_gpu_documents.py; equality is exact.  The
dense-partner cases add what those builders lack: partner lists several times as dense as the list that asks, so that a 128-key
pair is spread over all cooperative windows of the pair search and handed to the far search, with documents on.  Every case is
built and shown non-vacuous on the CPU (test_wide_cases_are_not_vacuous runs without a GPU) before a kernel is launched."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_doc_listing import _check as _check_listing
from test_gpu_documents import (BENCH, CLASS_REGEXPS, _brute_docs, _case, _check_tuples, _class_cases, _make, _search_both, _separator_case,
                                _step_case)
from test_gpu_search_window import OPTION_ROWS, _workspace
from vlg_matching_amd import variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE = ["1", "2"]


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _wide_index(V, text):
    """(the caller has set VLG_FORCE_POS64: index.hip reads it at build time, search.hip at search time)"""
    assert os.environ.get("VLG_FORCE_POS64") in FORCE
    idx = V.VlgIndex.build(text)
    assert idx.info()["pos_bytes"] == 8
    return idx


def _took_the_wide_path(V, res, force):
    """"1": the result's pieces are 8 bytes wide, so the narrow fetch is refused; "2": positions behind the wide locate are 4 bytes
    wide, and the narrow fetch hands out the values of fetch()"""
    assert res.summary["n_matches"] > 0
    if force == "1":
        with pytest.raises(V.VlgError):
            res.fetch32()
    else:
        f32, t32 = res.fetch32()
        _, _, first, tup = res.fetch()
        assert f32.dtype == np.uint32 and f32.tolist() == first.tolist() and t32.tolist() == tup.tolist()


def _search_wide(V, idx, batch, want, opts, force, ran=None):
    res = _search_both(idx, batch, want, opts, ran)
    _took_the_wide_path(V, res, force)
    return res


def _link_ran(idx, batch, opts=None):
    """the batch has a query of two sub-patterns or more: the link pass was launched"""
    ws = _workspace(opts or {})
    idx.search(batch, workspace=ws)
    assert ws.kernel_stats()["join_link"]["launches"] > 0


# ---- 1. the document cases of test_gpu_documents.py on wide positions ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("force", FORCE)
@pytest.mark.parametrize("name", ["dna3000", "abab"])
def test_wide_documents_against_brute_force(V, monkeypatch, name, force):
    """Counts, first positions, tuples, n_matches, checksum and n_tuple_values, with and without tuples, in both dialects and on every
    document set of _case(name): plain, rrr, text-order and d = 1 indexes under the default options; on the plain index every row of
    workspace options (the rows that name a filter kind with the proof that it ran) and "fuse_jump" = 0.  The three derived indexes
    are searched on the sets two, every7 and random only: with all eight a case took 6 to 7 s on the MI355X; the plain index and
    every option row run on all of them."""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text, batches, sets, want = _case(name)                                  # (asserts non-vacuity before the GPU is touched)
    assert set(sets) == {"one", "two", "64", "65", "every7", "on_occurrence", "random", "one_symbol"}
    plain = _wide_index(V, text)
    variants_ = [plain, plain.compress(), plain.resample(text_order=True, dens=7), plain.resample(text_order=False, dens=1)]
    assert all(i.info()["pos_bytes"] == 8 for i in variants_)
    for kind, reps, fields in batches:
        assert any(len(f[0]) >= 2 for f in fields)
        batch = _make(V, kind, reps)
        for sname, starts in sets.items():
            batch.set_documents(V.Documents.from_starts(starts, len(text)))
            w = want[(kind, sname)]
            for idx in variants_ if sname in ("two", "every7", "random") else variants_[:1]:
                _search_wide(V, idx, batch, w, {}, force)
            _search_wide(V, plain, batch, w, {"fuse_jump": 0}, force)
            for opts, ran in OPTION_ROWS[1:]:
                _search_wide(V, plain, batch, w, opts, force, ran)
            _link_ran(plain, batch, {"fuse_jump": 0})
        batch.set_documents(None)


@pytest.mark.gpu
@pytest.mark.parametrize("force", FORCE)
def test_wide_boundaries_inside_the_steps(V, monkeypatch, force):
    """the boundaries of _step_case -- inside a 128-key pair, between two steps, at a run border of the loaded library and one element to
    either side, at a segment border -- with the assertions of test_boundaries_inside_the_steps_of_the_link_pass"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
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
    idx = _wide_index(V, text)
    docs = V.Documents.from_starts(starts, len(text))
    for reps, want, dialect in ((lib_qs, wl, V.capi.DIALECT_LIBRARY), (bench_qs, wb, BENCH)):
        batch = V.index.Queries(reps, dialect=dialect)
        batch.set_documents(docs)
        for opts in ({"filter": 0}, {}, {"filter": 0, "fuse_jump": 0}, {"fuse_jump": 0}):
            res = _search_wide(V, idx, batch, want, opts, force)
            _link_ran(idx, batch, opts)
        assert res.summary["join_slots"] > 2048                              # lists longer than one link run of the default build


@pytest.mark.gpu
def test_wide_small_variant_runs_the_step_cases():
    """VLG_LINK_RUN = 192: the step cases and the dense-partner cases, in both force modes, in a child pytest that loads the `small`
    build -- runs of three steps, so the boundaries at R - 1, R, R + 1 fall at a run border that ends inside a pair, and the dense
    lists cross hundreds of run borders"""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_LINK_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_documents_wide.py", "-k",
                                "wide_boundaries_inside_the_steps or wide_dense_partners"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= len(FORCE) * (1 + len(DENSE_D)), tail


@pytest.mark.gpu
@pytest.mark.parametrize("force", FORCE)
def test_wide_classes_budgets_and_separator(V, monkeypatch, force):
    """a[bc]d-style batches with budgets k <= 2 and the separator case, as written and with "fuse_jump" = 0: class batches keep 32-bit
    lists (so nothing is claimed of their fetch32), their walks run on the wide index"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text, cases = _class_cases()
    idx = _wide_index(V, text)
    for budgets, starts, want in cases:
        q = V.Queries.from_classes(CLASS_REGEXPS)
        q.set_mismatches(budgets)
        q.set_documents(V.Documents.from_starts(starts, len(text)))
        _check_tuples(idx.search(q), want)
        _check_tuples(idx.search(q, workspace=_workspace({"fuse_jump": 0})), want)
        _link_ran(idx, q)
    text, starts, regexps, want = _separator_case()
    docs = V.Documents.from_separator(text, b"\n")
    assert docs.count() == len(starts) > 100
    q = V.Queries.from_classes(regexps)
    q.set_documents(docs)
    idx = _wide_index(V, text)
    _check_tuples(idx.search(q), want)
    _check_tuples(idx.search(q, workspace=_workspace({"fuse_jump": 0})), want)
    _link_ran(idx, q)


# ---- 2. dense partners -------------------------------------------------------------------------------------------------------------
DENSE_D = (3, 8, 40)
DENSE_PERIODS = 3000
# the stride of the `step` set: the brute force of a whole case stays under about two seconds, a document can hold a whole period, and
# every lcm(stride, d) symbols a boundary stands on an "a".  (d = 3: a stride of 7 puts two "a" into the document in front of such a
# boundary and the benchmark query, which matches every other "a", takes the first one -- no match ends next to the boundary; with
# a stride of 5 one does in every third document.  For the same reason the stride holds an odd number of periods: 13 = 8 + 5, 77 = 40 + 37.)
DENSE_STRIDE = {3: 5, 8: 13, 40: 77}
DENSE_OPTIONS = [{}, {"filter": 0}, {"filter": 0, "fuse_jump": 0}]
_dense = {}


def _dense_queries(d):
    """-> (library regexps, benchmark regexps, the indices of the a..b-shaped ones in either list).  "ab.{0,2}b" ends on the b at
    p + 2 of the period that begins at p, and the next "a" stands at p + d: its restart key p + 4 steps over that "a" for d = 3 only.
    "ab.{d-3,d-1}b" is the same query with the gap moved to the period's last b, p + d - 1 (for d = 3 it IS "ab.{0,2}b"): with
    end_len = |s_0| = 2 its restart key p + d + 1 lies behind the "a" at p + d whatever d is, so a boundary on that "a" must cap it."""
    lib = ["a.{0,2}?b", "a.{0,%d}?bb.{0,%d}?a" % (d, d), "b.{0,2}?a", "a", "b"]
    bench = ["ab.{0,2}b"] + (["ab.{%d,%d}b" % (d - 3, d - 1)] if d != 3 else [])
    return lib, bench


def _dense_sets(d, rng):
    n = d * DENSE_PERIODS

    def some_on_an_a(starts):
        """every fourth start moves back to the "a" of its period, every fourth to the b behind it (between the two symbols of the
        shortest match there is); the others stay where they fell"""
        starts = sorted(starts)
        return sorted({0} | {s - s % d + (i % 4) // 2 if i % 2 == 0 else s for i, s in enumerate(starts)})

    return {"one": [0],
            "sparse": some_on_an_a(int(x) for x in rng.integers(1, n, 12)),
            "random": some_on_an_a(int(x) for x in rng.integers(1, n, n // 40)),
            "step": list(range(0, n, DENSE_STRIDE[d]))}


def _dense_case(d):
    """-> (text, [(dialect, regexps, fields)], {set: starts}, {(dialect, set): expected per query}).  CPU only; computed once.  For
    every document set but the single document: the a..b-shaped queries have 500 matches or more each, differ from their answer on
    the undivided text and one loses a match; and for the benchmark query whose restart key can step over an "a" (the last one of
    _dense_queries), some document's first match begins ON a boundary that lies within end_len of the end of the match before --
    the restart key computed without the boundary would skip it."""
    if d in _dense:
        return _dense[d]
    import vlg_matching_amd as V
    text = (b"a" + b"b" * (d - 1)) * DENSE_PERIODS
    lib, bench = _dense_queries(d)
    batches = [("library", lib, [V.parse_query(q) for q in lib]), ("benchmark", bench, [V.parse_query(q, BENCH) for q in bench])]
    assert [len(f[0]) for f in batches[0][2]] == [2, 3, 2, 1, 1] and all(f[0] == [b"ab", b"b"] and f[3] == 2 for f in batches[1][2])
    sets = _dense_sets(d, np.random.default_rng(100 + d))
    assert len(sets["sparse"]) in (12, 13) and len(sets["random"]) > len(text) // 50
    want = {}
    for kind, reps, fields in batches:
        memo = {}
        whole = [_brute_docs(text, f, [0], memo) for f in fields]
        shaped = [0, 1] if kind == "library" else list(range(len(reps)))
        if kind == "library":
            assert [len(x) for x in whole[:2]] == [DENSE_PERIODS, DENSE_PERIODS // 2]
        else:                                                               # (the restart key steps over every other "a")
            assert len(whole[-1]) == DENSE_PERIODS // 2
        for sname, starts in sets.items():
            w = [_brute_docs(text, f, starts, memo) for f in fields]
            want[(kind, sname)] = w
            if sname == "one":
                assert w == whole
                continue
            for j in shaped:
                assert len(w[j]) >= 500, (d, kind, sname, reps[j], len(w[j]))
                assert w[j] != whole[j], (d, kind, sname, reps[j])
                assert any(t not in w[j] for t in whole[j]), (d, kind, sname, reps[j])
            if kind == "benchmark":
                end_len = fields[-1][3]
                first = {t[0] for t in w[-1]}
                ends = {t[-1] for t in w[-1]}
                assert any(b in first and any(b - e in ends for e in range(1, end_len)) for b in starts[1:]), (d, sname)
    _dense[d] = (text, batches, sets, want)
    return _dense[d]


def test_wide_cases_are_not_vacuous():
    """no GPU: the dense-partner cases hold what _dense_case asserts of them, and the partner lists have the densities that spread a
    128-key pair over the cooperative windows (d - 1 elements per key)"""
    for d in DENSE_D:
        text, batches, sets, want = _dense_case(d)
        assert len(text) == d * DENSE_PERIODS and text.count(b"a") == DENSE_PERIODS and text.count(b"b") == (d - 1) * DENSE_PERIODS
        assert set(sets) == {"one", "sparse", "random", "step"}
        for kind, reps, fields in batches:
            for sname in sets:
                assert len(want[(kind, sname)]) == len(reps)


@pytest.mark.gpu
@pytest.mark.parametrize("force", FORCE)
@pytest.mark.parametrize("d", DENSE_D)
def test_wide_dense_partners(V, monkeypatch, d, force):
    """"a" every d symbols, "b" d - 1 times as dense: consecutive keys of a pair advance d - 1 elements in the partner list, so d = 3
    spreads a pair over all four cooperative windows, d = 8 takes most of one through them into the far search, d = 40 nearly every
    key through the far search; the reverse densities, single lists, and a benchmark query whose restart key is capped at a boundary"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text, batches, sets, want = _dense_case(d)
    idx = _wide_index(V, text)
    for kind, reps, fields in batches:
        batch = _make(V, kind, reps)
        for sname, starts in sets.items():
            batch.set_documents(V.Documents.from_starts(starts, len(text)))
            for opts in DENSE_OPTIONS:
                _search_wide(V, idx, batch, want[(kind, sname)], opts, force)
                _link_ran(idx, batch, opts)
        batch.set_documents(None)


# ---- 4. the consumers of such a result ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("force", FORCE)
@pytest.mark.parametrize("case", ["dna3000", "dense8"])
def test_wide_result_lists_its_documents(V, monkeypatch, case, force):
    """vlg_result_list_documents on a document-bounded result of vlg_search_batch ("1": 8-byte pieces): df and the (document, count,
    first match) runs against numpy on its fetch(), and every match lies wholly inside the document the listing names for it"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text, batches, sets, want = _case(case) if case == "dna3000" else _dense_case(8)
    kind, reps, fields = batches[0]
    starts = sets["random"]
    docs = V.Documents.from_starts(starts, len(text))
    batch = _make(V, kind, reps)
    batch.set_documents(docs)
    res = _search_wide(V, _wide_index(V, text), batch, want[(kind, "random")], {}, force)
    _check_listing(V, res, starts, len(text), (case, force), docs)
    listing = res.list_documents(docs)
    counts, off, first, tup = res.fetch()
    assert listing.df.tolist() == [len({int(np.searchsorted(starts, t[0], "right")) - 1 for t in w}) for w in want[(kind, "random")]]
    doc = np.repeat(listing.docs.astype(np.int64), listing.counts.astype(np.int64))      # the runs cover the matches in order
    assert len(doc) == len(first) > 500
    bounds = np.asarray(starts + [len(text)], np.uint64)
    k = np.repeat([len(f[0]) for f in fields], counts.astype(np.int64))
    m_last = np.repeat([len(f[0][-1]) for f in fields], counts.astype(np.int64)).astype(np.uint64)
    last = tup[np.cumsum(k) - 1]
    assert (bounds[doc] <= first).all() and (last + m_last <= bounds[doc + 1]).all()
