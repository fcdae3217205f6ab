"""The pivot filter's range-kind segments: index ranges per (pivot element, level) instead of activity bits (filter.hpp).

Every case goes through vlg_join_batch on caller-built lists and is compared three ways: tuple for tuple with the oracle's join, array
for array with the unfiltered join, and array for array and in join_slots with pivot_range_ratio = 0 (the same build keeping activity
bits: equal join_slots means the same survivors; so does summary["filter_survivors"], which unlike join_slots does not depend on how
the joins were cut into chunks).  summary["filter_range_segments"] shows that the ranges were what ran.  The last two
tests run this file again in a child process: without the speculative compaction, and on the `small` variant of the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"filter_min": 0, "filter_stream_min": 0, "filter_pivot": 1, "filter_pivot_ratio": 2}
ALWAYS = 1                      # pivot_range_ratio: the pivot list is the shortest, so every pivot-filtered query qualifies


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


@pytest.fixture(scope="module")
def G(V):
    return V.capi.build_constants()["VLG_PIVOT_GROUPS"]


def _join(torch, cases, opts, cap=None):
    from vlg_matching_amd.index import Workspace, join_batch
    ws = Workspace(cap) if cap else Workspace()
    for k, v in opts.items():
        ws.set_option(k, v)
    flat, list_off, join_list, lo, hi, end_len = [], [0], [0], [], [], []
    for lists, l, h, e in cases:
        for i, a in enumerate(lists):
            flat.append(np.asarray(a, np.uint64))
            list_off.append(list_off[-1] + len(a))
            lo.append(0 if i == 0 else l[i - 1])
            hi.append(0 if i == 0 else h[i - 1])
        join_list.append(len(list_off) - 1)
        end_len.append(e)
    d = torch.from_numpy(np.concatenate(flat).view(np.int64)).cuda()
    return join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws), ws


_oracle_cache = {}


def _check(torch, oracle, name, cases, opts=None, cap=None, ratio=ALWAYS):
    """the three comparisons; -> the result with ranges"""
    opts = dict(BASE, **(opts or {}))
    res, ws = _join(torch, cases, dict(opts, pivot_range_ratio=ratio), cap)
    assert res.summary["filter_range_segments"] > 0, res.summary
    assert ws.kernel_stats()["filter_pivot"]["launches"] > 0 and ws.kernel_stats()["filter_compact"]["launches"] > 0
    if name not in _oracle_cache:                                 # (a case list is joined by the oracle once, whatever runs it again)
        _oracle_cache[name] = [oracle.join(*c) for c in cases]
    total = 0
    for j, (m, want) in enumerate(_oracle_cache[name]):
        assert int(res.counts[j]) == m, (name, j)
        assert res.tuples(j).tolist() == want.tolist(), (name, j)
        total += m
    assert res.summary["n_matches"] == total
    plain, _ = _join(torch, cases, {"filter": 0})
    bits, _ = _join(torch, cases, dict(opts, pivot_range_ratio=0), cap)
    assert bits.summary["filter_range_segments"] == 0 and bits.summary["filter_bit_segments"] > 0, bits.summary
    for x, y, z in zip(res.fetch(), plain.fetch(), bits.fetch()):
        assert (x == y).all() and (x == z).all(), name
    # the survivors the joins read, list by list and whatever the chunks: the same number
    assert res.summary["filter_survivors"] == bits.summary["filter_survivors"], (name, res.summary, bits.summary)
    # join_slots = those survivors and the lists read as they are, each class of segments of a chunk starting on a multiple of 64: the
    # same survivors in the same chunks are the same number.  Without a cap both runs are one chunk; under a cap their filter state
    # differs and so may their cuts: the test that sets one (below) goes on to a cap at which both cut alike
    assert cap or res.summary["n_chunks"] == bits.summary["n_chunks"], (name, res.summary, bits.summary)
    if res.summary["n_chunks"] == bits.summary["n_chunks"]:
        assert res.summary["join_slots"] == bits.summary["join_slots"], (name, res.summary, bits.summary)
    return (res, bits) if cap else res


def _distinct(rng, n, span):
    return np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64)


LO, HI = 4, 24                  # the carry cases: pivot element x keeps the neighbours p with LO <= x - p <= HI
HOLE = (20000, 22000)           # ... and no neighbour lies in here


def _carry_case(G, empty_groups):
    """[neighbour, pivot], the pivot last, 3 * 64 * G + 1 pivot elements; the neighbour list holds the even numbers but for one hole.
    The elements of a stretch that is `on` stand 6 apart (their windows overlap), every fourth right behind its predecessor (its range
    adds nothing); the elements of an empty stretch have their windows in the hole.
    empty_groups False: on over the first group borders and the first wave border (64 G), then empty until 9 elements into the next
    group (whose first on-element is so not its first), then on again.
    empty_groups True: 20 elements on, then empty up to element 192 (the groups [64, 128) and [128, 192) are wholly empty), on again
    (one element when G = 1).
    The last element's window reaches past the end of the neighbour list."""
    n_p = 3 * 64 * G + 1
    n_n = 64 * n_p + 512
    nb = np.arange(n_n + (HOLE[1] - HOLE[0]) // 2, dtype=np.uint64) * 2
    nb = nb[(nb < HOLE[0]) | (nb >= HOLE[1])][:n_n]
    e0, e1 = (20, 192) if empty_groups else (64 * G + 11, 64 * G + 64 + 9)     # the empty stretch
    x = []
    for e in range(n_p - 1):
        if e < e0:
            x.append(1000 + 6 * e + (0 if e % 4 else -5))
        elif e < e1:
            x.append(HOLE[0] + HI + 100 + 4 * (e - e0))
        else:
            x.append(HOLE[1] + 50 + 6 * (e - e1) + (0 if e % 4 else -5))
    assert 1000 + 6 * e0 < HOLE[0] and HOLE[0] + HI + 100 + 4 * (e1 - e0) - LO < HOLE[1]
    x.append(int(nb[-1]) + LO + 10)
    pv = np.array(x, dtype=np.uint64)
    assert len(pv) == n_p and (np.diff(pv.astype(np.int64)) > 0).all() and len(nb) >= 64 * n_p and x[-2] + 100 < int(nb[-1])
    return ([nb, pv], [LO], [HI], 1)


def _carry_cases(G):
    return [_carry_case(G, False), _carry_case(G, True)]


def test_carry_over_groups_waves_and_empty_groups(torch_cuda, oracle, G):
    cases = _carry_cases(G)
    res = _check(torch_cuda, oracle, "carry%d" % G, cases)
    survivors, seen = 0, set()
    for nb, pv in (c[0] for c in cases):
        lo_i = np.searchsorted(nb.astype(np.int64), pv.astype(np.int64) - HI, "left")
        hi_i = np.searchsorted(nb.astype(np.int64), pv.astype(np.int64) - LO, "right")
        on = hi_i > lo_i
        grp = [on[g:g + 64] for g in range(0, len(pv) - 1, 64)]
        inner_empty = [i for i, g_ in enumerate(grp) if not g_.any() and on[:64 * i].any() and on[64 * i + 64:].any()]
        if len(inner_empty) >= 2:
            seen.add("a carry crosses two whole empty groups")
        if any(g_.any() and not g_[0] for g_ in grp):
            seen.add("a group's first on-element is not its first element")
        for border in (64, 64 * G):
            if on[border - 1] and on[border] and hi_i[border - 1] > lo_i[border]:
                seen.add("windows overlap across element %d" % border)
        if (on[1:] & on[:-1] & (hi_i[1:] == hi_i[:-1])).any():
            seen.add("a later range adds nothing")
        if pv[-1] - LO > nb[-1] >= pv[-1] - HI:
            seen.add("a window reaches past the end")
        keep = np.zeros(len(nb), bool)
        for a, b in zip(lo_i, hi_i):
            keep[a:b] = True
        survivors += int(keep.sum())
    assert len(seen) == 5 + (G > 1), seen
    assert survivors <= res.summary["join_slots"] < survivors + 2 * 128   # (k = 2: the ranges of the one level are exact; + alignment)


def _direction_cases(rng):
    cases = []

    def lists(k, p, n_p=150, n_o=4000, span=60000):
        return [_distinct(rng, n_p if i == p else n_o + 300 * i, span) for i in range(k)]
    for k, p in ((2, 1), (3, 0), (3, 1), (3, 2), (5, 2)):
        for _ in range(2):
            lo = [int(rng.integers(0, 6)) for _ in range(k - 1)]
            cases.append((lists(k, p), lo, [l + int(rng.integers(1, 60)) for l in lo], 1 + int(rng.integers(0, 3))))
    # a dead query: nothing of the first list lies near the pivot list
    far = _distinct(rng, 3000, 20000) + np.uint64(10 ** 6)
    cases.append(([far, _distinct(rng, 100, 20000), _distinct(rng, 3000, 20000)], [0, 0], [50, 50], 1))
    return cases


def test_every_direction_and_depth(torch_cuda, oracle):
    cases = _direction_cases(np.random.default_rng(4100))
    res = _check(torch_cuda, oracle, "directions", cases)
    assert int(res.counts[len(cases) - 1]) == 0
    assert sum(int(c) for c in res.counts) > 0


def test_mixed_batch_of_range_bit_and_streamed_queries(torch_cuda, oracle):
    rng = np.random.default_rng(4200)
    cases = []
    for i in range(6):
        cases.append(([_distinct(rng, 4000, 50000), _distinct(rng, 100, 50000), _distinct(rng, 3000, 50000), _distinct(rng, 500, 50000)],
                      [0, 1, 0], [30, 40, 60], 1))                                                             # pivot, ratio 35: ranges
        cases.append(([_distinct(rng, 3000, 50000), _distinct(rng, 500, 50000)], [2], [25], 1))                # pivot, ratio 6: bits
        cases.append(([_distinct(rng, 1000, 20000), _distinct(rng, 1000, 20000)], [0], [12], 1))               # streamed
    res = _check(torch_cuda, oracle, "mixed", cases, {"filter_pivot_ratio": 3}, ratio=16)
    s = res.summary
    assert s["filter_range_segments"] == 12 and s["filter_bit_segments"] == 6 and s["filter_stream_segments"] == 6, s


def _fence_cases():
    """[A, B, pivot]: pivot element j stands 3 behind B[at_j] and A[at_j] 5 before it, so exactly c elements of B (direct level) and
    of A (hull level) survive; the survivors' lists of the batch lie one behind the other, their borders inside blocks of 64."""
    cases = []
    for c in (63, 64, 65, 128, 1, 200):
        n = 64 * c + 77
        B = np.arange(n, dtype=np.uint64) * 10 + 100
        at = np.arange(c) * 64 + 5
        cases.append(([B - 5, B, B[at] + 3], [5, 3], [5, 3], 1))
    return cases


def test_fences_written_by_the_compaction(torch_cuda, oracle):
    cases = _fence_cases()
    res = _check(torch_cuda, oracle, "fences", cases)
    assert [int(c) for c in res.counts] == [63, 64, 65, 128, 1, 200]
    assert 0 <= res.summary["join_slots"] - 2 * (63 + 64 + 65 + 128 + 1 + 200) < 64 * 3


def test_chunks_read_and_compact_range_segments(torch_cuda, oracle, G):
    """many survivors under a small workspace cap: the join runs in several chunks over the survivors' lists.  (Every list of a
    vlg_join_batch call is its own, and the room for the survivors is as large as the lists: a group's survivors always fit it here.
    The group that overflows it is the next test's.)"""
    rng = np.random.default_rng(4300)
    cases = _carry_cases(G) + _fence_cases()
    for _ in range(24):                                               # wide windows: most of the long lists survive
        cases.append(([_distinct(rng, 9000, 40000), _distinct(rng, 130, 40000), _distinct(rng, 9000, 40000), _distinct(rng, 300, 40000)],
                      [0, 0, 0], [400, 400, 400], 1))
    for cap_mb in (40, 32, 28, 24, 22, 20, 19, 18):                   # the first cap that cuts both runs, and cuts them alike
        res, bits = _check(torch_cuda, oracle, "chunks", cases, cap=cap_mb << 20)
        print("cap %d MiB: chunks %d (ranges) %d (bits), join_slots %d %d" % (cap_mb, res.summary["n_chunks"], bits.summary["n_chunks"],
                                                                             res.summary["join_slots"], bits.summary["join_slots"]))
        if res.summary["n_chunks"] > 1 and res.summary["n_chunks"] == bits.summary["n_chunks"]:
            break
    assert res.summary["n_chunks"] > 1 and res.summary["n_chunks"] == bits.summary["n_chunks"], (res.summary, bits.summary)
    assert res.summary["join_slots"] == bits.summary["join_slots"]    # (asserted by _check already: said again where it matters)


def test_group_whose_survivors_overflow_the_room_behind_the_lists(V, oracle):
    """Forty queries of a search share one list of 1500 occurrences and a pivot list of twelve, under windows that keep nearly all of the
    1500: the survivors of the group, a list per query, are some 50 000, and the room behind the located lists (a few times their 1512
    elements) takes a tenth of that.  The speculative expansion of the whole group stops at the room's end (a group of ranges that would
    pass it writes nothing), summary["filter_overflows"] counts the group, and every join chunk expands the ranges of its own queries."""
    from vlg_matching_amd.index import Workspace
    n_a, n_p, n_q = 1500, 12, 40
    rng = np.random.default_rng(4500)
    slots = n_a + n_p + 64
    text = bytearray(rng.choice(np.frombuffer(b"ab", np.uint8), 4 * slots + 16).tobytes())
    at = rng.permutation(slots) * 4
    for p in at[:n_a]:
        text[p:p + 2] = b"\x81\x81"
    for p in at[n_a:n_a + n_p]:
        text[p:p + 2] = b"\xf0\xf0"
    text = bytes(text)
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text)
    qs = ["\x81\x81.{0,%d}?\xf0\xf0" % (3000 + 7 * i) for i in range(n_q)]
    want = [o.search(q).tolist() for q in qs]
    assert all(len(w) > 0 for w in want)                            # (matches do not overlap: about one per pivot element and query)
    speculative = os.environ.get("VLG_NO_SPECULATIVE_COMPACT") != "1"
    slots_seen = []
    for ratio in (ALWAYS, 0):
        ws = Workspace()
        for k_, v_ in dict(BASE, pivot_range_ratio=ratio).items():
            ws.set_option(k_, v_)
        res = idx.search(qs, workspace=ws)
        s = res.summary
        print("pivot_range_ratio %d:" % ratio, s)
        assert (s["filter_range_segments"], s["filter_bit_segments"]) == ((n_q, 0) if ratio else (0, n_q)), s
        assert s["filter_survivors"] > 20 * (n_a + n_p), s
        assert s["filter_overflows"] == (1 if speculative else 0) and s["n_chunks"] > 1, s
        assert ws.kernel_stats()["filter_compact"]["launches"] > 0
        for i, q in enumerate(qs):
            assert res.tuples(i).tolist() == want[i], (ratio, q)
        slots_seen.append((s["filter_survivors"], s["n_chunks"], s["join_slots"]))
    assert slots_seen[0] == slots_seen[1], slots_seen              # (the survivors alone cut these chunks: both runs cut alike)


def test_through_a_search_with_both_range_producers(V, oracle):
    """patterns of 63 .. 4097 occurrences beside a pivot pattern of a dozen: the bracket searches (pivot_rungs 0) and the ladder
    (pivot_rungs 2) both feed the ranges"""
    from vlg_matching_amd.index import Workspace
    lengths = [63, 64, 65, 1023, 1025, 4097]
    rng = np.random.default_rng(4400)
    slots = sum(lengths) + 64
    text = bytearray(rng.choice(np.frombuffer(b"ab", np.uint8), 4 * slots + 16).tobytes())
    at = rng.permutation(slots) * 4
    used = 0
    for i, L in enumerate(lengths):
        for p in at[used:used + L]:
            text[p:p + 2] = bytes([0x80 + i, 0x80 + i])
        used += L
    for p in at[used:used + 12]:
        text[p:p + 2] = b"\xf0\xf0"
    text = bytes(text)
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text)
    qs = []
    for i in range(len(lengths)):
        t = chr(0x80 + i) * 2
        qs += [t + ".{0,300}?\xf0\xf0", t + ".{0,64}?\xf0\xf0.{0,64}?" + t, t + ".{0,200}?" + t + ".{0,200}?\xf0\xf0"]
    want = [o.search(q).tolist() for q in qs]
    for rungs in (0, 2):
        ws = Workspace()
        for k_, v_ in dict(BASE, pivot_rungs=rungs, pivot_range_ratio=ALWAYS).items():
            ws.set_option(k_, v_)
        res = idx.search(qs, workspace=ws)
        ks = ws.kernel_stats()
        assert ks["filter_pivot"]["launches"] > 0 and (ks["filter_ladder"]["launches"] > 0) == (rungs == 2), ks
        assert res.summary["filter_range_segments"] > 0, res.summary
        for i, q in enumerate(qs):
            assert res.tuples(i).tolist() == want[i], (rungs, q)


CHILD_ENV = "VLG_PIVOT_RANGES_CHILD"


def _run_child(env_extra):
    """the tests above in one fresh process (the parent launches nothing on the GPU meanwhile)"""
    env = dict(os.environ, **env_extra)
    env[CHILD_ENV] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_pivot_ranges.py",
                                                                             "-k", "not child_process"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout.splitlines()[-1] and "skipped" not in out.stdout.splitlines()[-1], tail


def test_child_process_without_speculative_compaction():
    """VLG_NO_SPECULATIVE_COMPACT=1: every chunk expands the ranges of its own lists (JoinChunk::compact_survivors)"""
    assert CHILD_ENV not in os.environ
    _run_child({"VLG_NO_SPECULATIVE_COMPACT": "1", "VLG_HIP_LIBRARY": os.environ.get("VLG_HIP_LIBRARY", "")})


def test_child_process_on_the_small_variant():
    """VLG_PIVOT_GROUPS = 1 and VLG_COMPACT_RUNS = 1: a wave per group of pivot elements and per run"""
    assert CHILD_ENV not in os.environ
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    c = variants.constants("small")
    assert c["VLG_PIVOT_GROUPS"] == 1 and c["VLG_COMPACT_RUNS"] == 1
    _run_child({"VLG_HIP_LIBRARY": lib})
