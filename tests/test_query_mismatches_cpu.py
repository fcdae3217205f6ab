"""Mismatch budgets per sub-pattern, host side (no GPU): the brute-force statements of tests/vlg_approx_brute.py agree with a plain
loop over positions, and vlg_queries_set_mismatches / _get_mismatches are declared, exported, bound and refuse a NULL batch on the host.
(A batch needs a device to exist, so the round trips and the refusals on real batches are in tests/test_gpu_query_mismatches.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vlg_approx_brute as A
import vlg_class_brute as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    if not os.path.exists(v.library_path()):
        v.build_library()
    return v


def _by_loop(text, rows, k):
    """the definition, position by position: v occurs when 0 <= v, v + m <= n and at most k of the m positions are not accepted"""
    n, m = len(text), len(rows)
    out = []
    for v in range(0, n - m + 1):
        miss = 0
        for t in range(m):
            if not rows[t][text[v + t]]:
                miss += 1
        if miss <= k:
            out.append(v)
    return out


def test_two_statements_of_approximate_occurrences_agree():
    rng = np.random.default_rng(6)
    nonempty = 0
    for trial in range(80):
        sigma = int(rng.integers(1, 6))
        text = (97 + rng.integers(0, sigma, size=int(rng.integers(1, 120)))).astype(np.uint8).tobytes()
        m = int(rng.integers(1, 6))
        rows = np.zeros((m, 256), dtype=bool)
        for t in range(m):
            rows[t, 97 + rng.choice(7, size=int(rng.integers(1, 4)), replace=False)] = True       # (some members are not in the text)
        for k in (0, 1, 2, m, m + 3):
            got = A.approx_occurrences(text, rows, k)
            assert got.dtype == np.uint64 and got.tolist() == _by_loop(text, rows, k), (trial, k)
            if k == 0:
                assert got.tolist() == B.class_occurrences(text, rows).tolist(), trial
            if k >= m:
                assert got.tolist() == list(range(0, max(0, len(text) - m + 1))), (trial, k)          # every position may differ
            nonempty += len(got) > 0
            widths = A.frontier_widths(text, rows, k)
            assert len(widths) == m
            for j in range(1, m + 1):
                strings = {text[v:v + j] for v in _by_loop(text, rows[m - j:], k)}
                assert widths[j - 1] == len(strings), (trial, k, j)
    assert nonempty > 100
    # by hand
    assert A.approx_occurrences(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 0).tolist() == [0]
    assert A.approx_occurrences(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 1).tolist() == [0, 3]
    assert A.approx_occurrences(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 2).tolist() == [0, 3]
    assert A.approx_occurrences(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 3).tolist() == [0, 1, 2, 3]
    assert A.approx_occurrences(b"ab", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 3).tolist() == []           # m > n
    assert A.misses(b"aaaa", [B.row(b"b"), B.row(b"a")]).tolist() == [1, 1, 1]
    assert A.frontier_widths(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"c")], 1) == [4, 2, 2]           # a b c d | bc bd | abc abd


def test_header_library_and_binding_stay_in_step(V):
    src = open(os.path.join(ROOT, "include", "vlg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"vlg_status\s+vlg_queries_set_mismatches\s*\(\s*vlg_queries\s*\*\s*q\s*,\s*const\s+uint8_t\s*\*\s*h_k\s*\)\s*;", code)
    assert re.search(r"vlg_status\s+vlg_queries_get_mismatches\s*\(\s*const\s+vlg_queries\s*\*\s*q\s*,\s*int\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*h_k\s*\)\s*;", code)
    L = C.CDLL(V.library_path())
    bound = {s[0]: s for s in V.capi.SYMBOLS}
    for name, nargs in (("vlg_queries_set_mismatches", 2), ("vlg_queries_get_mismatches", 3)):
        assert hasattr(L, name), "library does not export " + name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == nargs


def test_null_batch_is_refused_without_a_device(V):
    L = V.lib()
    k = (C.c_uint8 * 3)(1, 2, 3)
    has = C.c_int(7)
    assert L.vlg_queries_set_mismatches(None, k) == V.capi.E_INVALID
    assert L.vlg_queries_set_mismatches(None, None) == V.capi.E_INVALID
    assert L.vlg_queries_get_mismatches(None, C.byref(has), k) == V.capi.E_INVALID
    assert L.vlg_queries_get_mismatches(None, None, None) == V.capi.E_INVALID
    assert has.value == 7 and list(k) == [1, 2, 3]                          # (nothing was written)
    assert b"null" in L.vlg_last_error()
