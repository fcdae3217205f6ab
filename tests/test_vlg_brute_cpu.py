"""The brute-force statement of the search (tests/vlg_brute.py) pinned before anything on the device is measured with it: against the
oracle's merge join, the reference's recorded answers, and the reference's own vlg_iterator."""
import json
import os
import re

import numpy as np
import pytest

from util import I63, array_queries, dna_text, skewed_text
from vlg_brute import lazy_matches, lazy_matches_by_sweeps, occurrences

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vlg_known_answers.json")))
TEXTS = {"dna": dna_text(1500, 21).tobytes(), "zipf": skewed_text(1500, 22).tobytes(), "100a": b"a" * 100, "abab": b"ab" * 150 + b"aab" * 40}


def test_occurrences_byte_and_integer():
    assert occurrences(b"abracadabra", b"a").tolist() == [0, 3, 5, 7, 10]
    assert occurrences(b"aaaa", b"aa").tolist() == [0, 1, 2] and occurrences(b"aaaa", b"aaaaa").tolist() == []
    assert occurrences(b"abc", b"abc").tolist() == [0] and occurrences(b"", b"a").tolist() == []
    t = np.array([0, 2 ** 31, 0, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    assert occurrences(t, np.array([0, 2 ** 31], dtype=np.uint32)).tolist() == [0, 2]
    assert occurrences(t, np.array([2 ** 32 - 1], dtype=np.uint32)).tolist() == [4]
    assert occurrences(t, np.array([7], dtype=np.uint32)).tolist() == []


def test_lazy_matches_by_hand():
    a = [0, 1, 2, 3, 4, 5]
    assert lazy_matches([a], [], [], 2) == [[0], [2], [4]]
    assert lazy_matches([a, a], [0], [0], 1) == [[i, i] for i in a]                         # two sub-patterns at the same position
    assert lazy_matches([a, a, a], [1, 1], [1, 1], 1) == [[0, 1, 2], [3, 4, 5]]
    assert lazy_matches([a, a], [1], [3], 1, cap=2) == lazy_matches_by_sweeps([a, a], [1], [3], 1, cap=2) == [[0, 1], [2, 3]]
    assert lazy_matches([a, []], [0], [9], 1) == [] and lazy_matches([[], a], [0], [9], 1) == []
    # the least tuple is not the greedy one: 10 is the first partner of 0, but only 12 has a partner in the third list
    assert lazy_matches([[0], [10, 12], [22]], [5, 10], [20, 10], 1) == lazy_matches_by_sweeps([[0], [10, 12], [22]], [5, 10], [20, 10], 1) == [[0, 12, 22]]
    # ... and a first element without any chain is passed over
    assert lazy_matches([[0, 3], [10, 14], [25]], [5, 11], [12, 11], 1) == [[3, 14, 25]]
    # bounds near 2^63, positions near 2^62: no wrapping
    big = 1 << 62
    assert lazy_matches([[5, big], [6, big + 1]], [1], [I63], I63) == [[5, 6]]
    assert lazy_matches([[5, big], [6, big + 1]], [I63], [I63], 1) == []
    assert lazy_matches([[5], [5 + I63]], [I63], [I63], 1) == [[5, 5 + I63]]


def _random_lists(rng, k, span, dense):
    base = np.unique(rng.integers(0, span, int(rng.integers(1, dense))))
    lists = []
    for _ in range(k):
        if rng.integers(0, 3) == 0:
            lists.append(base)                                                              # duplicates across lists
        else:
            lists.append(np.unique(rng.integers(0, span, int(rng.integers(1, dense)))))
    return lists


def test_lazy_matches_equals_the_merge_join_on_random_lists(oracle):
    """Random lists (shared elements across lists included), k up to 64, lo = 0, overlapping windows, lo == hi, hi = 2^63 - 1, all end_len
    kinds: the definition and the oracle's monotone pointers yield the same tuples.  (Positions stay below 2^62: the join adds in 64 bits.)"""
    rng = np.random.default_rng(5)
    total = 0
    for case in range(1500):
        k = int((1, 2, 2, 3, 3, 4, 8, 9, 31, 32, 33, 40, 64)[case % 13])
        span = int(rng.choice([30, 200, 3000]))
        lists = _random_lists(rng, k, span, int(rng.choice([6, 40, 300])))
        lo, hi = [], []
        for _ in range(k - 1):
            kind = int(rng.integers(0, 5))
            a = 0 if kind == 0 else int(rng.integers(0, 12))
            b = a if kind == 1 else I63 if kind == 2 else a + int(rng.integers(0, 40))
            if kind == 4 and case % 50 == 0:
                a = b = I63
            lo.append(a)
            hi.append(b)
        end_len = int(rng.choice([1, 2, 3, 1000, I63]))
        m, want = oracle.join(lists, lo, hi, end_len, cap=max(len(lists[0]), 1))
        got = lazy_matches(lists, lo, hi, end_len)
        assert got == want.tolist(), (case, k, lo, hi, end_len)
        assert lazy_matches_by_sweeps(lists, lo, hi, end_len) == got, (case, k, lo, hi, end_len)      # candidate by candidate: the same
        assert len(got) == m
        for cap in (1, 2):
            assert lazy_matches(lists, lo, hi, end_len, cap=cap) == got[:cap]
        total += len(got)
    assert total > 3000


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_lazy_matches_equals_the_merge_join_on_caller_built_queries(oracle, name):
    """the query kinds of test_gpu_query_arrays.py, on smaller texts"""
    text = TEXTS[name]
    total = 0
    for subs, lo, hi, end_len in array_queries(text, 31, n=80):
        lists = [occurrences(text, s) for s in subs]
        want = oracle.join(lists, lo, hi, end_len, cap=len(text))[1].tolist() if all(len(l) for l in lists) else []
        assert lazy_matches(lists, lo, hi, end_len) == want, (subs, lo, hi, end_len)
        assert lazy_matches_by_sweeps(lists, lo, hi, end_len) == want, (subs, lo, hi, end_len)
        total += len(want)
    assert total > 100


def _parse_int_query(q):
    """'5 6 .{0,3}? 7' -> (sub-patterns, lo, hi): gaps count symbols (vlg_index.hpp:95)"""
    parts = re.split(r"\.\{(\d+),(\d+)\}\?", q)
    subs = [np.array([int(t) for t in p.split()], dtype=np.uint64) for p in parts[0::3]]
    lo = [int(a) + len(subs[i]) for i, a in enumerate(parts[1::3])]
    hi = [int(b) + len(subs[i]) for i, b in enumerate(parts[2::3])]
    return subs, lo, hi


def test_lazy_matches_equals_the_references_recorded_answers(oracle):
    n = 0
    for case in GOLD["cases"]:
        if "error" in case:
            continue
        subs, lo, hi, end_len = oracle.query_fields(oracle.parse(case["query"]))
        text = case["text"].encode()
        assert lazy_matches([occurrences(text, s) for s in subs], lo, hi, end_len) == case["tuples"], case
        n += 1
    for case in GOLD["int_cases"]:
        subs, lo, hi = _parse_int_query(case["query"])
        text = np.array(case["int_text"], dtype=np.uint64)
        assert lazy_matches([occurrences(text, s) for s in subs], lo, hi, len(subs[-1])) == case["tuples"], case
        n += 1
    assert n >= 15


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_lazy_matches_equals_the_references_iterator(oracle, refmod, name):
    """vlg_iterator restated over the reference's own wt_range_walker (oracle/_ref) on the reference's own tree, for the queries its
    parser can express (lo >= |s_{i-1}|, end_len = |s_last|) with k up to 64 -- except one sub-pattern of one symbol, where the iterator
    itself skips matches (test_oracle.py::test_vlg_iterator_skips_the_odd_twin_of_adjacent_single_symbol_matches)."""
    text = TEXTS[name]
    idx = oracle.Index.from_text(text)
    w = refmod.RefWtInt(oracle.suffix_array(np.frombuffer(text + b"\0", dtype=np.uint8)))
    total = 0
    for subs, lo, hi, _ in array_queries(text, 32, n=60):
        if len(subs) == 1 and len(subs[0]) == 1:
            continue
        lo = [a + len(s) for a, s in zip(lo, subs)]                     # as the parser stores them: at least the previous length
        hi = [min(b + len(s), I63) for b, s in zip(hi, subs)]
        ranges = [(lambda c: (c[1], c[2]) if c[0] else (1, 0))(idx.backward_search(s)) for s in subs]
        want = w.vlg_iterate(ranges, lo, hi, len(subs[-1])).tolist()
        assert lazy_matches([occurrences(text, s) for s in subs], lo, hi, len(subs[-1])) == want, (subs, lo, hi)
        total += len(want)
    assert total > 50
