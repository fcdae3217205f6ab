"""The lookups the passes over a result share (csrc/result_passes.hpp; doc_rank_dev and DocWave of join_device.hpp), pinned at their
edges through every consumer at once: nB = 66 and 65 (one fence; a ragged last block of two entries, of one), a first document of one
symbol, a match at position 0, a key at n_text - 1 in the last document, empty queries around the matching ones, a result in several
pieces.  The yardstick is brute force on the CPU and np.searchsorted over the starts on result.fetch()."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_doc_listing import _runs, _same
from test_gpu_documents import _brute_docs
from test_gpu_match_texts import _last_positions, _rule
from test_gpu_wtsa_window import _brute_window
from test_gpu_wtsa_window import _check as _check_result
from util import dna_text
from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000
EMPTY = "\xfe"
# Of its workspace a batch keeps 16 MiB and the lists off the join (search.hip: run_batch, plan_super_chunk), and a match of a query
# of one sub-pattern costs the join 30 bytes (kJoinBytesPerSlot + kJoinBytesPerSlot0): under 24 MiB more than 279 620 such matches
# cannot be joined in one chunk.
WORKSPACE = 24 << 20
ONE_CHUNK = (WORKSPACE - (16 << 20)) // 30


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _case():
    """-> (text, regexps): empty queries in front of, between and behind the matching ones; a query that matches at position 0, inside
    the first document and across its end; queries whose only sub-pattern ends at n_text, at n_text - 1, - 3 and - 5"""
    text = dna_text(N, 23, probs=(0.7, 0.1, 0.1, 0.1)).tobytes()
    s = lambda b: b.decode("latin-1")
    edge = [s(text[:1]), s(text[:4]), EMPTY, s(text[-1:]), s(text[-3:]), EMPTY, EMPTY, s(text[-5:])]
    gapped = ["A.{0,6}?C", "C.{1,9}?G.{0,4}?T", "AA.{2,30}?AA", "T.{0,3}?A.{0,3}?C.{0,3}?G"]
    bulk = []
    for i in range(170):                                                     # what forces the second piece: 170 x about 2100 matches
        bulk += ["A"] + ([EMPTY] if i % 7 == 0 else []) + ([EMPTY, EMPTY] if i % 31 == 0 else [])
    return text, [EMPTY, EMPTY] + edge + gapped + bulk[:len(bulk) // 2] + gapped[::-1] + bulk[len(bulk) // 2:] + edge[::-1] + [EMPTY]


def _starts(text, n_docs):
    """n_docs documents: the first of one symbol, the last of three, the others cut at random"""
    rng = np.random.default_rng(n_docs)
    inner = rng.choice(np.arange(2, N - 3), n_docs - 3, replace=False)
    return sorted({0, 1, N - 3} | {int(x) for x in inner})


def _symbols(t, b, e):
    """the concatenation of t[b[i]:e[i]]"""
    lens = e - b
    out_off = np.concatenate([[0], np.cumsum(lens)])
    return t[np.repeat(b - out_off[:-1], lens) + np.arange(out_off[-1])], out_off


@pytest.mark.parametrize("n_docs", [65, 64])
def test_every_consumer_at_the_edges(V, n_docs):
    from vlg_matching_amd.index import Workspace
    text, qs = _case()
    t = np.frombuffer(text, np.uint8)
    starts = _starts(text, n_docs)
    assert len(starts) == n_docs and starts[1] == 1 and (len(starts) + 1) >> 6 == 1 and (len(starts) + 1) & 63 == (2 if n_docs == 65 else 1)
    fields = {q: V.parse_query(q.encode("latin-1")) for q in set(qs)}
    whole = {q: _brute_window(text, f, 0, N) for q, f in fields.items()}
    memo = {}
    bounded = {q: _brute_docs(text, f, starts, memo) for q, f in fields.items()}
    # the edges are hit, on the CPU
    assert whole[qs[2]][0] == [0] and whole[qs[3]][0] == [0] and bounded[qs[2]][0] == [0] and [0] not in bounded[qs[3]]
    assert whole[qs[5]][-1] == [N - 1] == bounded[qs[5]][-1] and whole[qs[6]][-1] == [N - 3] == bounded[qs[6]][-1]
    assert whole[qs[9]][-1] == [N - 5] and [N - 5] not in bounded[qs[9]]
    counts = [len(whole[q]) for q in qs]
    assert counts[0] == counts[1] == counts[-1] == 0 and sum(1 for c in counts if c == 0) > 30
    assert sum(c for q, c in zip(qs, counts) if len(fields[q][0]) == 1) > ONE_CHUNK
    assert sum(1 for q in set(qs) if whole[q] != bounded[q]) >= 6

    idx = V.VlgIndex.build(text)
    docs = V.Documents.from_starts(starts, N)
    batch = V.Queries(qs)
    res = idx.search(batch, workspace=Workspace(WORKSPACE))
    assert res.summary["n_chunks"] >= 2                                      # several pieces
    _check_result(res, [whole[q] for q in qs])
    _, off, first, _ = res.fetch()
    doc = np.searchsorted(np.asarray(starts, np.uint64), first, "right") - 1
    assert doc.min() == 0 and doc.max() == n_docs - 1 and int(first.max()) == N - 1

    # Documents.locate of every first position
    d, o = docs.locate(first)
    assert d.tolist() == doc.tolist() and o.tolist() == (first.astype(np.int64) - np.asarray(starts, np.int64)[doc]).tolist()

    # the listing, with pairs and df only
    want = _runs(first, off, starts)
    assert int(want[3].sum()) == len(first)
    _same(res.list_documents(docs), want, "pairs")
    _same(res.list_documents(docs, pairs=False), want, "df")

    # the match texts inside the documents: flanks 0 and to the bound
    ta = idx.text_access(64)
    q_of, p0, pl = _last_positions(res, batch.ks)
    mlast = np.asarray([len(fields[q][0][-1]) for q in qs], np.int64)
    ce = pl + mlast[q_of]
    for flank in (0, None):
        b, e, B0, B1 = _rule(p0, ce, N, starts, flank)
        assert flank == 0 or ((b == B0).all() and (e == np.maximum(B1, ce)).all() and (ce > B1).any())
        sym_want, off_want = _symbols(t, b, e)
        mt = res.extract_matches(batch, ta, flank=flank, documents=docs)
        m_off, m_beg, m_sym = mt.fetch()
        assert mt.n_matches == len(p0) and mt.n_symbols == len(sym_want), flank
        assert m_off.tolist() == off_want.tolist() and m_beg.tolist() == b.tolist(), flank
        assert np.array_equal(m_sym, sym_want), flank

    # a document-bounded search of the same queries, in several pieces too, and its own listing
    batch.set_documents(docs)
    res = idx.search(batch, workspace=Workspace(WORKSPACE))
    assert res.summary["n_chunks"] >= 2
    _check_result(res, [bounded[q] for q in qs])
    _, off, first, _ = res.fetch()
    _same(res.list_documents(docs), _runs(first, off, starts), "bounded")


def _child(env_extra):
    env = dict(os.environ, **env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_result_passes.py", "-k", "every_consumer"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= 2, tail


def test_small_variant_runs_the_edges():
    """VLG_DOCLIST_RUN = 192: the same cases in a child pytest that loads the `small` build"""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_DOCLIST_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    _child({"VLG_HIP_LIBRARY": lib})


def test_stored_document_ids_see_the_same_edges():
    """VLG_DOCLIST_STORE_IDS=1: the scatter pass reads the documents the head pass stored (a child process: the switch is read once)"""
    _child({"VLG_DOCLIST_STORE_IDS": "1"})
