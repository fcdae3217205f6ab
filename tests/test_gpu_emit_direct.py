"""First positions written by the emit pass of the chain itself (join_device.hpp: chain_emit_kernel<.., kDirect>; workspace option
"emit_direct", with "tuples" = 0): no mlist[], no gather pass.

Every case goes through vlg_join_batch on caller-made lists.  "emit_direct" = 1 is compared with "emit_direct" = 0 (emit into mlist[],
then gather) and with the oracle's merge join: counts, offsets, first positions and checksum; and "tuples" = 1 with "emit_direct" = 1,
which must take the gather pass, with the oracle's tuples; the workspace's kernel statistics say which path ran (launches of the class
"gather").  The cases sit on what the direct emit adds to the emit pass: the rank of a
match inside its tile's record (lanes hold the ranks lane, 64 + lane, ...), the match number of a record's first match, the query's
offset into the result, the first list's place in P, and the workgroup's checksum when some of its four waves have no record."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 1024                 # slots per chain tile (join_device.hpp: kTile)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


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
    d = torch.from_numpy(np.ascontiguousarray(np.concatenate(flat), dtype=np.uint64).view(np.int64)).cuda()
    res = join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws)
    return res, ws.kernel_stats()["gather"]["launches"]


def _check(torch, oracle, cases, opts=None, cap=None):
    want = [oracle.join(*c) for c in cases]
    counts = [m for m, _ in want]
    first = [int(v) for _, t in want for v in t[:, 0].tolist()]
    chk = sum(first) % (1 << 64)
    base = {"filter": 0}
    base.update(opts or {})
    runs = {}
    for name, o in (("direct", {"tuples": 0, "emit_direct": 1}), ("gather", {"tuples": 0, "emit_direct": 0}),
                    ("tuples", {"tuples": 1, "emit_direct": 1})):
        res, gathers = _join(torch, cases, dict(base, **o), cap)
        # the path taken, not only its results: no gather pass behind the direct emit, one per chunk with matches otherwise
        assert (gathers == 0) == (name == "direct") and gathers <= res.summary["n_chunks"], (name, gathers)
        c, off, f, _ = res.fetch()
        assert c.tolist() == counts, name
        assert off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), name
        assert f.tolist() == first, name
        assert res.summary["n_matches"] == sum(counts) and res.summary["checksum"] == chk, name
        assert res.summary["n_tuple_values"] == (sum(m * len(cs[0]) for m, cs in zip(counts, cases)) if name == "tuples" else 0), name
        if name == "tuples":
            for j, (m, t) in enumerate(want):
                assert res.tuples(j).tolist() == t.tolist(), j
        runs[name] = res
    assert runs["direct"].summary["n_chunks"] == runs["gather"].summary["n_chunks"]
    return want, runs["direct"]


def _tile_query(n, hits, offset=0):
    """A first list of n elements four apart of which the elements `hits` have their partner one position on: with end_len = 1 every
    one of them is a match, and the chain goes from hit to hit."""
    x = np.arange(n, dtype=np.uint64) * np.uint64(4) + np.uint64(100 + offset)
    y = x[np.asarray(hits, dtype=np.int64)] + np.uint64(1)
    return ([x, y], [1], [1], 1)


def _rank_border_cases(offset=0):
    """Every first list is a whole number of tiles long and all queries have k = 2, so the first lists lie tile by tile in the slots.
    Chains of exactly 1, 63, 64, 65 and 1024 matches inside one tile; a query without a match between two with matches; a single
    match; a chain that enters a tile on its last slot and leaves it at once."""
    cases = [_tile_query(TILE, range(c), offset) for c in (1, 63, 64, 65, TILE)]
    cases.append(_tile_query(TILE, [TILE - 1], offset))                        # the single match on the last slot of its tile
    dead = _tile_query(TILE, [5], offset)
    dead[0][1] = dead[0][1] + np.uint64(1)                                     # the partner is out of the gap: no match
    cases.append(dead)
    cases.append(_tile_query(2 * TILE, [3, TILE - 1, TILE + 6], offset))       # ... 2 -> last slot of the tile -> the next tile
    cases.append(_tile_query(TILE, range(0, TILE, 3), offset))
    return cases


def test_ranks_inside_a_tile(torch_cuda, oracle):
    cases = _rank_border_cases()
    want, res = _check(torch_cuda, oracle, cases)
    assert [m for m, _ in want] == [1, 63, 64, 65, TILE, 1, 0, 3, (TILE + 2) // 3]
    assert res.summary["n_chunks"] == 1


def _mixed_cases(offset=0):
    """Many queries in one chunk, k = 1, 2 and 3 side by side: first lists that start anywhere in P and in the slots, results that
    start anywhere in the result; a first list of about 5000 elements whose chain crosses four tiles behind an odd number of slots."""
    rng = np.random.default_rng(20261021)
    cases = []
    for i in range(40):
        k = int(rng.integers(1, 4))
        n = int(rng.integers(1, 700))
        lists = [np.sort(rng.choice(4 * n + 16, size=n, replace=False)).astype(np.uint64) + np.uint64(offset) for _ in range(k)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 9)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 6))))
        if i == 20:
            cases.append(_tile_query(5000, range(0, 5000, 2), offset))
            cases.append(_tile_query(777, [], offset))                         # no partner at all
    return cases


def test_many_queries_in_one_chunk(torch_cuda, oracle):
    cases = _mixed_cases()
    want, res = _check(torch_cuda, oracle, cases)
    assert res.summary["n_chunks"] == 1 and want[21][0] == 2500 and want[22][0] == 0
    assert sum(1 for m, _ in want if m) >= 30


def test_through_the_window_filter(torch_cuda, oracle):
    _check(torch_cuda, oracle, _mixed_cases() + _rank_border_cases(), {"filter": 1, "filter_min": 0, "filter_stream_min": 0})


def test_single_list_queries(torch_cuda, oracle):
    """class 0 alone: every element is feasible, the jumps come from the separate jump pass"""
    rng = np.random.default_rng(5)
    cases = [([np.sort(rng.choice(9 * n, size=n, replace=False)).astype(np.uint64)], [], [], int(e))
             for n, e in ((1, 1), (64, 3), (1023, 2), (1024, 9), (1025, 1), (3000, 40), (130, 1))]
    want, _ = _check(torch_cuda, oracle, cases)
    assert want[0][0] == 1 and want[4][0] > 500


def test_wide_positions(torch_cuda, oracle):
    """values above 2^32: the 64-bit instantiations"""
    off = (1 << 33) + 4321
    want, _ = _check(torch_cuda, oracle, _rank_border_cases(off) + _mixed_cases(off))
    assert min(int(t[0, 0]) for m, t in want if m) > 1 << 32


def test_several_join_chunks(torch_cuda, oracle):
    """a small workspace: several join chunks, each with its own piece of the result"""
    rng = np.random.default_rng(77)
    cases = []
    for _ in range(60):
        k = int(rng.integers(1, 4))
        lists = [np.sort(rng.choice(400000, size=int(n), replace=False)).astype(np.uint64) for n in rng.integers(1000, 30000, k)]
        lo = [int(rng.integers(0, 151)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 301)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 9))))
    want, res = _check(torch_cuda, oracle, cases, cap=40 << 20)
    assert res.summary["n_chunks"] > 1 and sum(m for m, _ in want) > 0
