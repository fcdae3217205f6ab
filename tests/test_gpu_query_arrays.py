"""Query batches built by the caller (vlg_queries_create / Queries.from_arrays) through both search paths -- the FM-index path
(vlg_search_batch) and the paper's lazy index (vlg_wtsa_search_batch) -- against the brute-force statement of the search
(tests/vlg_brute.py).  These are the shapes the regexp parser cannot produce: start-to-start bounds below the previous sub-pattern's
length down to lo = 0, hi up to 2^63 - 1, an end_len that is no sub-pattern's length, k up to 64 with a different gap everywhere."""
import functools

import numpy as np
import pytest

from util import array_queries, dna_text, skewed_text
from vlg_brute import lazy_matches, occurrences

pytestmark = pytest.mark.gpu
TEXTS = {"dna": lambda: dna_text(4000, 41).tobytes(), "zipf": lambda: skewed_text(4000, 42).tobytes(), "300a": lambda: b"a" * 300,
         "abab": lambda: b"ab" * 600 + b"aab" * 100}
MODES = ("fm", "fm_filter0", "fm_filter1", "fm_first_positions", "wtsa_wave", "wtsa_lane", "wtsa_first_positions")


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


@functools.lru_cache(maxsize=None)
def _case(name):
    """text, the batch's fields, and what every query must return (computed once, shared by all modes, never changed)"""
    text = TEXTS[name]()
    batch = array_queries(text, 43 + len(name))
    want = tuple(tuple(map(tuple, lazy_matches([occurrences(text, s) for s in subs], lo, hi, end_len))) for subs, lo, hi, end_len in batch)
    return text, batch, want


def _search(V, monkeypatch, mode, text, q):
    ws = V.index.Workspace()
    if mode.startswith("fm"):
        if mode in ("fm_filter0", "fm_filter1"):
            ws.set_option("filter", int(mode[-1]))
            ws.set_option("filter_min", 0)
            ws.set_option("filter_stream_min", 0)
        if mode == "fm_first_positions":
            ws.set_option("tuples", 0)
        return V.VlgIndex.build(text).search(q, workspace=ws)
    if mode == "wtsa_lane":
        monkeypatch.setenv("VLG_WTSA_LANE_PER_QUERY", "1")
    else:
        monkeypatch.delenv("VLG_WTSA_LANE_PER_QUERY", raising=False)
    if mode == "wtsa_first_positions":
        ws.set_option("tuples", 0)
    return V.WtsaIndex(text).search(q, workspace=ws)


def _check(res, want, ks, with_tuples):
    counts = res.counts
    assert [int(c) for c in counts] == [len(w) for w in want]
    n_matches = sum(len(w) for w in want)
    assert res.summary["n_matches"] == n_matches
    assert res.summary["checksum"] == sum(t[0] for w in want for t in w) % (1 << 64)
    assert res.summary["n_tuple_values"] == (sum(len(w) * k for w, k in zip(want, ks)) if with_tuples else 0)
    for i, w in enumerate(want):
        assert res.positions(i).tolist() == [t[0] for t in w], i
        if with_tuples:
            assert res.tuples(i).tolist() == [list(t) for t in w], i


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_caller_built_batches_equal_brute_force(V, torch_cuda, monkeypatch, name, mode):
    text, batch, want = _case(name)
    assert sum(len(w) for w in want) > 300 and sum(1 for w, b in zip(want, batch) if w and len(b[0]) >= 31) >= 3     # not vacuous, deep ones too
    q = V.index.Queries.from_arrays([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], [b[3] for b in batch])
    assert q.ks.tolist() == [len(b[0]) for b in batch]
    res = _search(V, monkeypatch, mode, text, q)
    _check(res, want, [len(b[0]) for b in batch], with_tuples=not mode.endswith("first_positions"))


@pytest.mark.parametrize("name", ["dna", "abab"])
def test_from_arrays_of_parsed_fields_equals_the_parsed_batch(V, torch_cuda, name):
    """vlg_parse_query's fields handed to vlg_queries_create give the batch vlg_queries_parse builds: same results, both paths"""
    text = TEXTS[name]()
    rng = np.random.default_rng(7)
    qs = []
    for _ in range(120):
        k = int(rng.choice([1, 2, 3, 4, 9, 33]))
        subs = [text[s:s + int(rng.integers(1, 4))].decode() for s in rng.integers(0, len(text) - 3, k)]
        q = subs[0]
        for s in subs[1:]:
            a = int(rng.integers(0, 20))
            q += ".{%d,%d}?%s" % (a, a + int(rng.integers(0, 50)), s)
        qs.append(q)
    qs += ["\xfe.{0,5}?" + text[:1].decode(), text[:2].decode() + ".{0,4611686018427387903}?" + text[5:7].decode()]
    fields = [V.parse_query(q) for q in qs]
    built = V.index.Queries.from_arrays([f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields], [f[3] for f in fields])
    for idx in (V.VlgIndex.build(text), V.WtsaIndex(text)):
        a, b = idx.search(qs), idx.search(built)
        assert a.summary["n_matches"] == b.summary["n_matches"] > 100 and a.summary["checksum"] == b.summary["checksum"]
        for x, y in zip(a.fetch(), b.fetch()):
            assert x.tolist() == y.tolist()
