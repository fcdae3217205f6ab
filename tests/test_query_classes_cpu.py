"""Character classes in sub-patterns, host side (no GPU): the brute-force statements of tests/vlg_class_brute.py agree with each
other, and vlg_parse_class_query agrees with the restated grammar and -- on strings without classes -- with vlg_parse_query."""
import os

import numpy as np
import pytest

import vlg_class_brute as B


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    if not os.path.exists(v.library_path()):
        v.build_library()
    return v


def test_two_statements_of_class_occurrences_agree():
    rng = np.random.default_rng(5)
    nonempty = 0
    for trial in range(60):
        sigma = int(rng.integers(1, 6))
        text = (97 + rng.integers(0, sigma, size=int(rng.integers(1, 400)))).astype(np.uint8)
        m = int(rng.integers(1, 5))
        rows = np.zeros((m, 256), dtype=bool)
        for t in range(m):
            rows[t, 97 + rng.choice(7, size=int(rng.integers(1, 5)), replace=False)] = True       # (some members are not in the text)
        a, b = B.class_occurrences(text, rows), B.class_occurrences_re(text.tobytes(), rows)
        assert a.tolist() == b.tolist(), trial
        assert len(B.distinct_member_strings(text.tobytes(), rows)) <= len(a)
        nonempty += len(a) > 0
    assert nonempty > 20
    # by hand
    assert B.class_occurrences(b"abcabd", [B.row(b"a"), B.row(b"b"), B.row(b"cd")]).tolist() == [0, 3]
    assert B.class_occurrences(b"aaaa", [B.row(b"a"), B.row(b"a")]).tolist() == [0, 1, 2]                     # overlapping starts
    assert B.class_occurrences(b"ab", [B.row(b"a"), B.row(b"b"), B.row(b"c")]).tolist() == []
    assert (B.rows_of(B.masks_of([B.row(b"a\xff"), B.row(b"\x01")])) == np.array([B.row(b"a\xff"), B.row(b"\x01")])).all()


CASES = ["a[bc]d", "[a-c]x.{1,2}?[^a]", r"\[a\]", r"[\]]", r"[a\-c]", "a.{1,2}?[.{]", "[]", "[^]", "[ab", "[z-a]", "a\\",
         "[a\x00]", "[\x00-c]", "[^\x01-\xff]", "[-a]", "[a-]", "[a-c-e]", r"[\^a]", r"a\.{1,2}?b", r"[a-\]]", "[ab].{0,3}?[cd][ef].{2,2}?g",
         "[a]", "x[a]y", "[a.{1,2}?b]", "a[b.{1,2}?c", "[ab].{2,1}?c", "[ab].{1,2}c", "[ab].{1,2}?", ".{1,2}?[ab]", "[\\", "[a\\"]


def _check_against_grammar(V, c):
    try:
        want = B.parse(c)
    except B.GrammarError as e:
        with pytest.raises(V.VlgError) as ee:
            V.parse_class_query(c)
        assert ee.value.status == e.status, (c, str(e))
        return False
    subs, lo, hi, end = V.parse_class_query(c)
    assert len(subs) == len(want[0]), c
    for got, w in zip(subs, want[0]):
        assert got.shape == (len(w), 32) and (B.rows_of(got) == np.array(w)).all(), c
    assert (lo, hi, end) == (want[1], want[2], want[3]), c
    return True


def test_parser_matches_the_restated_grammar(V):
    ok = sum(_check_against_grammar(V, c) for c in CASES)
    assert 10 <= ok <= len(CASES) - 10                                   # both outcomes are well represented
    # the verdicts the issue names, by hand
    for c, status in [("[]", 4), ("[^]", 4), ("[ab", 4), ("[z-a]", 4), ("a\\", 4), ("[a\x00]", 1)]:
        with pytest.raises(V.VlgError) as e:
            V.parse_class_query(c)
        assert e.value.status == status, c
    subs, lo, hi, end = V.parse_class_query("a.{1,2}?[.{]")
    assert [len(s) for s in subs] == [1, 1] and V.index.class_mask_members(subs[1][0]).tobytes() == b".{"
    subs, _, _, _ = V.parse_class_query("[^a]")
    assert V.index.class_mask_members(subs[0][0]).tolist() == [c for c in range(1, 256) if c != 97]


def test_at_most_64_subpatterns(V):
    q64 = ".{0,1}?".join(["[ab]"] * 64)
    subs, lo, hi, end = V.parse_class_query(q64)
    assert len(subs) == 64 and lo == [1] * 63 and hi == [2] * 63
    assert _check_against_grammar(V, q64)
    with pytest.raises(V.VlgError) as e:
        V.parse_class_query(q64 + ".{0,1}?[ab]")
    assert e.value.status == V.capi.E_INVALID
    assert not _check_against_grammar(V, q64 + ".{0,1}?[ab]")


def test_lengths_count_positions(V):
    subs, lo, hi, end = V.parse_class_query(r"[abc][de]\[.{2,5}?x[a-z][^q]y.{0,0}?[01]")
    assert [len(s) for s in subs] == [3, 4, 1]
    assert lo == [2 + 3, 0 + 4] and hi == [5 + 3, 0 + 4] and end == 1
    # the same shape in plain bytes has the same fields
    assert V.parse_query("abc.{2,5}?xyzw.{0,0}?0")[1:] == (lo, hi, end)


# the case list of test_capi_cpu.py::test_host_parser_matches_oracle_parser, restated: none of them holds '[' or '\'
LIBRARY_CASES = ["ab.{2,5}?cde.{0,7}?f", "a", "abc.{0,0}?abc", "a.{1,2}b", "a.{3,2}?b", "a.{x,2}?b", "a.{1,2", ".{1,2}?b", "a.{1,2}?",
                 "a.{ 1, 2}?b", "a.{+1,2}?b", "a.{1,2}?b.{3,4}c", "x.{0,18446744073709551616}?y", "x.{0,4611686018427387903}?y",
                 "ab.{2,5}cde.{0,7}f", "A.{0,100}C", "A.{0,100}?C", "q.{1}?r", "a.{1,2}?b.{5,6}?c.{7,8}?d",
                 "x.{0,18446744073709551615}?y", "x.{0,4611686018427387904}?y", "", "a.{-1,2}?b"]


def test_strings_without_classes_parse_as_the_library_dialect(V):
    parsed = 0
    for c in LIBRARY_CASES:
        assert "[" not in c and "\\" not in c
        try:
            want = V.parse_query(c, V.capi.DIALECT_LIBRARY)
        except V.VlgError as e:
            with pytest.raises(V.VlgError) as ee:
                V.parse_class_query(c)
            assert ee.value.status == e.status, c
            continue
        subs, lo, hi, end = V.parse_class_query(c)
        assert [bytes(int(V.index.class_mask_members(r)[0]) for r in s) for s in subs] == want[0], c
        assert all(len(V.index.class_mask_members(r)) == 1 for s in subs for r in s)
        assert (lo, hi, end) == want[1:], c
        parsed += 1
    assert 5 <= parsed < len(LIBRARY_CASES)


def test_count_only_and_small_buffer(V):
    import ctypes as C
    L = V.lib()
    p, n = V.capi.ParsedQuery(), C.c_uint64()
    raw = b"a[bc]d.{1,2}?[ef]"
    assert L.vlg_parse_class_query(raw, len(raw), C.byref(p), None, 0, C.byref(n)) == 0
    assert n.value == 4 and p.k == 2 and list(p.sub_off[:2]) == [0, 3] and list(p.sub_len[:2]) == [3, 1]
    buf = np.zeros((3, 32), np.uint8)
    assert L.vlg_parse_class_query(raw, len(raw), C.byref(p), buf.ctypes.data, 3, C.byref(n)) == V.capi.E_INVALID
