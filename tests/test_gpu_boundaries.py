"""Oracle tests aimed at the borders where a kernel hands work from one wave, run or chunk to the next.

Every test reads the constants of the library it loaded (vlg_build_constants) and builds its input so that it lands on their borders,
shows through kernel_stats() or the input's own layout that the path it aims at ran, and compares tuple for tuple with the oracle.
They run on the default build and, through tests/test_gpu_variants.py, on every variant, where the constants are small enough that
the same inputs cross each border hundreds of times."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

kRun = 2048                    # list elements per run of the filter and the compaction (join_device.hpp: kRun, not a build constant)


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
def K(V):
    return V.capi.build_constants()


def _dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _join(torch, cases, opts):
    """vlg_join_batch over cases [(lists, lo, hi, end_len)] -> (result, workspace)"""
    from vlg_matching_amd.index import Workspace, join_batch
    ws = Workspace()
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
    d = _dev_u64(torch, np.concatenate(flat))
    res = join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws)
    return res, ws


def _assert_oracle(oracle, res, cases):
    total = 0
    for j, (lists, lo, hi, e) in enumerate(cases):
        m, want = oracle.join(lists, lo, hi, e)
        assert int(res.counts[j]) == m, j
        assert res.tuples(j).tolist() == want.tolist(), j
        total += m
    assert res.summary["n_matches"] == total
    return total


def _sorted_distinct(rng, n, span):
    return np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64)


def _slot_borders(lengths_by_class):
    """Slot numbers of the segment borders of the link pass (search.hip: classes from the most sub-patterns after them down, each
    class starting on a multiple of 64, its segments in query order)."""
    borders, acc = [], 0
    for lengths in lengths_by_class:
        acc = (acc + 63) // 64 * 64
        for n in lengths:
            acc += n
            borders.append(acc)
    return borders


@pytest.mark.parametrize("k", [2, 3])
def test_link_pass_segment_borders_on_run_and_step_borders(torch_cuda, V, oracle, K, k):
    """Segments whose borders fall at 64 j and VLG_LINK_RUN j, +-1, so that runs of the link pass start, end and change segment on
    and next to every border, runs end inside a two-step (128-key) pair, and one list spans many 1024-slot tiles.  k = 2: the link
    pass of the last class only; k = 3: a class whose next list has join state (next_feasible) in front of it."""
    R = K["VLG_LINK_RUN"]
    rng = np.random.default_rng(700 + k)
    n_runs = 120
    borders = {R * j + int(rng.integers(-1, 2)) for j in range(1, n_runs + 1)}
    borders |= {64 * j + int(rng.integers(-1, 2)) for j in range(1, n_runs * R // 64, 5)}
    borders = sorted(b for b in borders if b > 0)
    lengths = list(np.diff([0] + borders)) + [20 * 1024 + 1]                 # the last one spans 21 tiles
    cases = []
    for n in lengths:
        n = int(n)
        span = 3 * n + 16
        lists = [_sorted_distinct(rng, n, span) for _ in range(k - 1)] + [_sorted_distinct(rng, max(1, n // 2), span)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 9)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 4))))
    # every class with slots holds the lists 0 .. k-2 of the queries, in query order: the same lengths in each
    slot_b = _slot_borders([lengths] * (k - 1))
    near_run = sum(1 for b in slot_b if min(b % R, R - b % R) <= 1)
    near_step = sum(1 for b in slot_b if min(b % 64, 64 - b % 64) <= 1)
    assert near_run >= 100 and near_step >= 150, (near_run, near_step)
    assert slot_b[-1] >= (k - 1) * 100 * R                                  # >= 100 runs of the link pass per class
    res, ws = _join(torch_cuda, cases, {"filter": 0})
    assert ws.kernel_stats()["join_link"]["launches"] >= k - 1
    assert _assert_oracle(oracle, res, cases) > 0
    # the same through the window filter: the survivors' compacted lists, with fences of their own
    res_f, ws_f = _join(torch_cuda, cases, {"filter": 1, "filter_min": 0, "filter_stream_min": 0})
    assert ws_f.kernel_stats()["filter_compact"]["launches"] > 0
    _assert_oracle(oracle, res_f, cases)


def _resolve_texts(n):
    rng = np.random.default_rng(5)
    block = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 37).tobytes())
    periodic = bytearray(block * (n // 37 + 1))[:n]
    for p in rng.integers(0, n, n // 500):                                    # noise: a few periods differ
        periodic[p] = ord("n")
    return {"a_run": b"a" * n, "ab_run": b"ab" * (n // 2), "periodic": bytes(periodic)}


@pytest.mark.parametrize("name", ["a_run", "ab_run", "periodic"])
def test_resolve_chains_longer_than_a_round(V, oracle, K, name):
    """Texts made of long runs of adjacent occurrences: a walk of the trail-sharing sweep stops on the occurrence right behind it,
    so the trail records form chains as long as the gaps between SA samples.  The index samples every (2 VLG_RESOLVE_HOPS + 8)-th
    SA index, so chains outlast a resolve round of VLG_RESOLVE_HOPS hops (a second round must run), and the batch holds many times
    VLG_GROUP_CHUNK and VLG_RESOLVE_CHUNK records (chunk borders inside chains)."""
    from vlg_matching_amd.index import Workspace
    H, G, C = K["VLG_RESOLVE_HOPS"], K["VLG_GROUP_CHUNK"], K["VLG_RESOLVE_CHUNK"]
    dens = 2 * H + 8
    n = max(40000, 5 * dens, 8 * max(G, C)) * (4 if name == "periodic" else 1)
    text = _resolve_texts(n)[name]
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text, dens=dens)
    qs = {"a_run": ["a", "aa", "a.{0,3}?a"], "ab_run": ["ab", "b", "a.{1,1}?a", "ba.{0,4}?b"],
          "periodic": ["a", "c", "g.{0,40}?t", text[:5].decode()]}[name]
    ws = Workspace()
    for k_, v_ in {"sweep_min": 1, "sweep_tail": 16}.items():
        ws.set_option(k_, v_)
    res = idx.search(qs, workspace=ws)
    ks = ws.kernel_stats()
    total = 0
    for i, q in enumerate(qs):
        want = o.search(q)
        assert res.tuples(i).tolist() == want.tolist(), q
        total += len(want)
    assert total >= 8 * max(G, C)
    # one launch per resolve round: chains longer than a round's hops need at least a second one
    assert ks["locate_resolve"]["launches"] >= 2, ks["locate_resolve"]


@pytest.mark.parametrize("dense_min", [0, 1 << 20])
def test_compaction_survivors_in_one_run_the_last_run_and_none(torch_cuda, V, oracle, K, dense_min):
    """The compaction takes kRun (2048) list elements per run and VLG_COMPACT_RUNS runs per wave.  Each query's first list spans two
    waves' groups of runs and a partial last run; the second list is placed so that the survivors of the first lie in exactly one
    run of a group, only in the last partial run, in one run of each group, or nowhere.  dense_min 0 moves every run word by word
    (the dense path), 2^20 half a word per lane (the sparse path)."""
    CR = K["VLG_COMPACT_RUNS"]
    rng = np.random.default_rng(900 + (dense_min > 0))
    n_runs = 2 * CR + 1
    n0 = kRun * (n_runs - 1) + 777
    base = np.arange(n0, dtype=np.uint64) * 10
    first_group_run = min(3, CR - 1)
    layouts = {
        "one_run": [first_group_run],
        "last_partial_run": [n_runs - 1],
        "one_run_per_group": [first_group_run, CR + min(5, CR - 1)],
        "every_run": list(range(n_runs)),
        "none": [],
    }
    cases, expect = [], []
    for name, runs in layouts.items():
        for count in (1, 40, 700):                                           # survivors per chosen run: sparse and dense runs
            picks = []
            for r in runs:
                lo_i, hi_i = r * kRun, min(n0, (r + 1) * kRun)
                picks.append(rng.choice(np.arange(lo_i, hi_i), size=min(count, hi_i - lo_i), replace=False))
            sel = np.sort(np.concatenate(picks)) if picks else np.zeros(0, np.int64)
            second = base[sel] + 3 if len(sel) else np.array([base[-1] + 1000], np.uint64)   # "none": nothing in any window
            cases.append(([base, np.sort(second).astype(np.uint64)], [3], [3], 1))
            surv_runs = sorted(set((sel // kRun).tolist()))
            assert surv_runs == sorted(runs), (name, surv_runs)
            expect.append(len(sel))
    opts = {"filter": 1, "filter_min": 0, "filter_stream_min": 0, "compact_dense_min": dense_min}
    res, ws = _join(torch_cuda, cases, opts)
    assert ws.kernel_stats()["filter_compact"]["launches"] > 0
    _assert_oracle(oracle, res, cases)
    # the join saw no more than the lists' survivors (the filter keeps a superset of the exact ones, never fewer)
    assert sum(expect) <= res.summary["join_slots"] < len(cases) * n0
    res_plain, _ = _join(torch_cuda, cases, {"filter": 0})
    for x, y in zip(res.fetch(), res_plain.fetch()):
        assert (x == y).all()


def _fan_lengths(F):
    lengths, p = [], F
    while p <= 70000:
        lengths += [p - 1, p, p + 1]
        p *= F
    return lengths


def test_pivot_ladder_lists_of_fan_power_lengths(V, oracle, K):
    """The pivot filter descends the ladder of fan f = 2^VLG_RUNG_SHIFT over the sorted lists of a search: patterns with exactly
    f^j - 1, f^j and f^j + 1 occurrences (a level more or less, a last group cut by one) beside a pivot pattern of a dozen, at every
    alignment inside the shared array (the lists stand side by side in it)."""
    from vlg_matching_amd.index import Workspace
    F = 1 << K["VLG_RUNG_SHIFT"]
    lengths = _fan_lengths(F)
    assert len(lengths) <= 0x70
    rng = np.random.default_rng(1200 + F)
    slots = sum(lengths) + 64
    text = bytearray(rng.choice(np.frombuffer(b"ab", np.uint8), 4 * slots + 16).tobytes())
    at = rng.permutation(slots) * 4
    used = 0
    for i, L in enumerate(lengths):                                          # token i occurs exactly L times
        for p in at[used:used + L]:
            text[p:p + 2] = bytes([0x80 + i, 0x80 + i])
        used += L
    for p in at[used:used + 12]:
        text[p:p + 2] = b"\xf0\xf0"                                         # the pivot
    text = bytes(text)
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text)
    qs = []
    for i in range(len(lengths)):
        t = chr(0x80 + i) * 2
        qs += ["\xf0\xf0.{0,%d}?%s" % (4 * (i + 1), t), t + ".{0,300}?\xf0\xf0", t + ".{0,64}?\xf0\xf0.{0,64}?" + t]
    ws = Workspace()
    for k_, v_ in {"filter_min": 0, "filter_stream_min": 0, "filter_pivot": 1, "filter_pivot_ratio": 2, "pivot_rungs": 2}.items():
        ws.set_option(k_, v_)
    res = idx.search(qs, workspace=ws)
    ks = ws.kernel_stats()
    assert ks["filter_pivot"]["launches"] > 0 and ks["filter_ladder"]["launches"] > 0, ks
    for i, q in enumerate(qs):
        assert res.tuples(i).tolist() == o.search(q).tolist(), q


def test_pivot_filter_on_caller_lists_of_fan_power_lengths(torch_cuda, V, oracle, K):
    """The pivot filter's bracket searches (vlg_join_batch builds no ladder) on lists of the same lengths, VLG_PIVOT_GROUPS groups
    of 64 pivot elements per wave, lists ahead of and behind the pivot."""
    F = 1 << K["VLG_RUNG_SHIFT"]
    rng = np.random.default_rng(1300 + F)
    cases = []
    for L in _fan_lengths(F):
        span = 4 * L + 64
        long1 = _sorted_distinct(rng, L, span)
        pivot = _sorted_distinct(rng, min(span, 64 * K["VLG_PIVOT_GROUPS"] + 1), span)
        lo = int(rng.integers(0, 4))
        hi = lo + int(rng.integers(0, 40))
        cases.append(([pivot, long1], [lo], [hi], 1))
        cases.append(([long1, pivot], [lo], [hi], 2))
        cases.append(([long1, pivot, _sorted_distinct(rng, L, span)], [lo, 0], [hi, 30], 1))
    res, ws = _join(torch_cuda, cases, {"filter_min": 0, "filter_stream_min": 0, "filter_pivot": 1, "filter_pivot_ratio": 2})
    assert ws.kernel_stats()["filter_pivot"]["launches"] > 0
    _assert_oracle(oracle, res, cases)
