"""The chain's tile pass as a two-level backward scan (join_device.hpp: chain_tiles_scan; workspace option "tile_scan") and the walk of
heavy queries by waves with a look-ahead over tile heads (chain_walk_kernel; workspace option "walk_wave").

The scan's arithmetic is restated on the CPU (`scan`, below) and held against plain chain following on random tiles, without a GPU.

Every GPU case goes through vlg_join_batch on caller-made lists and is compared with the oracle's merge join: counts, first positions,
tuples and checksum.  Each runs with "tile_scan" and "walk_wave" at 1 and at 0 (all four pairs), with and without tuples, and with
"fuse_jump" 1 and 0; "filter" is 0 throughout.  A case passes only if its batch ran in one chunk and produced matches.

Where the cases sit: a tile is 1024 slots = 32 blocks of 32; a wave walks a query whose level-0 segment overlaps at least 64 tiles
(kWalkWaveTiles) and fetches the first 16 words of the next 4 tiles with every round.  In a batch of single-list queries the level-0
slots begin at slot 0 and the segments follow each other in query order, which is what places the borders below."""
import numpy as np
import pytest

SIZES = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097]   # those of test_gpu_fused_jump.py
TILE = 1024
WALK_WAVE_TILES = 64
# (tile_scan, walk_wave, fuse_jump, tuples)
MODES = [(s, w, f, t) for s, w in ((1, 1), (0, 0), (1, 0), (0, 1)) for f in (1, 0) for t in (1, 0)]


# ---- the CPU model of the two phases ----------------------------------------------------------------------------------------------

def scan(j, base, K=1024, B=32, NONE=0xFFFFFFFF):      # j: settled jump words of the tile's slots (int64), base: its first slot
    nxt = np.where((j != NONE) & (j < base + K), j - base, -1)
    last, cnt, out = np.arange(K), np.ones(K, np.int64), nxt.copy()
    for b in range(K // B):                             # phase 1: every block on its own, from its last slot to its first
        for s in range(b * B + B - 1, b * B - 1, -1):
            t = nxt[s]
            if 0 <= t < b * B + B:
                last[s], cnt[s], out[s] = last[t], cnt[t] + 1, out[t]
    for b in range(K // B - 1, -1, -1):                 # phase 2: blocks from the last to the first, one look-up per slot
        for s in range(b * B, b * B + B):
            t = out[s]
            if t >= 0:                                  # (t lies in a later block: final)
                last[s], cnt[s], out[s] = last[t], cnt[s] + cnt[t], -1
    return j[last], cnt                                 # xh[base + s] = (exit, chain elements inside the tile)


def _follow(j, base, K=1024, NONE=0xFFFFFFFF):
    """plain chain following, slot by slot"""
    ext, cnt = np.empty(K, np.int64), np.empty(K, np.int64)
    for s in range(K):
        c, n = s, 1
        while j[c] != NONE and j[c] < base + K:
            c, n = int(j[c] - base), n + 1
        ext[s], cnt[s] = j[c], n
    return ext, cnt


def _random_tile(rng, base, lo, hi, none_share, K=1024, NONE=0xFFFFFFFF):
    """jump words of a tile: slot s -> base + s + (a length in [lo, hi]), kNone with the given share"""
    j = base + np.arange(K, dtype=np.int64) + rng.integers(lo, hi + 1, K)
    j[rng.random(K) < none_share] = NONE
    return j


def test_model_of_the_scan_agrees_with_chain_following():
    rng = np.random.default_rng(20261021)
    shapes = [(1, 1), (1, 3), (31, 65), (1, 65), (1, 2000), (900, 2000)]
    n = 0
    for lo, hi in shapes:
        for none_share in (0.0, 0.02, 0.1, 0.25, 0.5):
            for _ in range(10):
                base = int(rng.integers(0, 1 << 20)) * 1024
                j = _random_tile(rng, base, lo, hi, none_share)
                got, want = scan(j, base), _follow(j, base)
                assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), (lo, hi, none_share)
                n += 1
    assert n == 300
    # every slot hops to the next: the largest count the state word holds
    j = np.arange(1, 1025, dtype=np.int64)
    ext, cnt = scan(j, 0)
    assert cnt.tolist() == list(range(1024, 0, -1)) and set(ext.tolist()) == {1024}


# ---- GPU cases ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _join(torch, cases, opts):
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
    return join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws)


_want = {}


def _oracle(oracle, name, cases):
    """The oracle's answers of a named set of cases, computed once and shared by the modes."""
    if name not in _want:
        _want[name] = [oracle.join(*c) for c in cases]
    return _want[name]


def _check(torch, oracle, name, cases, mode, floor):
    scan_on, wave, fuse, tuples = mode
    want = _oracle(oracle, name, cases)
    res = _join(torch, cases, {"filter": 0, "tile_scan": scan_on, "walk_wave": wave, "fuse_jump": fuse, "tuples": tuples})
    total, chk = 0, 0
    for j, (m, t) in enumerate(want):
        assert int(res.counts[j]) == m, (name, j)
        assert res.positions(j).tolist() == t[:, 0].tolist(), (name, j)
        if tuples:
            assert res.tuples(j).tolist() == t.tolist(), (name, j)
        total += m
        chk = (chk + int(t[:, 0].sum())) % (1 << 64) if m else chk
    assert res.summary["n_matches"] == total and res.summary["checksum"] == chk, name
    assert res.summary["n_tuple_values"] == (sum(m * len(c[0]) for (m, _), c in zip(want, cases)) if tuples else 0), name
    assert res.summary["n_chunks"] == 1, name
    assert total >= floor, (name, total)
    return res, total


def _run(n, offset=0):
    return np.arange(n, dtype=np.uint64) + np.uint64(offset)


def _distinct(rng, n, span):
    return np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64)


def _every_slot_hops_cases():
    """k = 1, consecutive positions, end_len 1: every slot hops to the next one, 1024 chain elements in a full tile; every block border
    and every tile border is crossed.  The four lists follow each other, so the later ones begin inside a block."""
    return [([_run(n)], [], [], 1) for n in (1023, 1024, 1025, 3 * 1024 + 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_slot_hops_to_the_next(torch_cuda, oracle, mode):
    cases = _every_slot_hops_cases()
    _, total = _check(torch_cuda, oracle, "hops", cases, mode, 1023 + 1024 + 1025 + 3 * 1024 + 5)
    assert total == 1023 + 1024 + 1025 + 3 * 1024 + 5


END_LENS = [31, 32, 33, 63, 64, 1023, 1024, 1025, 2 * 1024 + 1]
LONG = 68 * TILE                                        # a heavy list: 68 tiles, or 69 where it does not begin on a tile border


def _long_jump_cases():
    """k = 1, consecutive positions: every jump is end_len slots long.  From the first list's slot 0 (slot 0 of a tile) the chain lands on
    the last slot of a block, the first slot of the next block, the tile's last slot, the next tile's first slot, or beyond the next
    tile; the lists are heavy, so the last three also make the look-ahead meet an exit that skips a tile."""
    return [([_run(LONG, 7 * i)], [], [], e) for i, e in enumerate(END_LENS)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_jumps_of_block_and_tile_length(torch_cuda, oracle, mode):
    cases = _long_jump_cases()
    want = _oracle(oracle, "long", cases)
    assert [m for m, _ in want] == [-(-LONG // e) for e in END_LENS]
    _check(torch_cuda, oracle, "long", cases, mode, sum(-(-LONG // e) for e in END_LENS))


def _border_cases(k, sizes=SIZES, seed=0):
    """One join per first-list length, all in one chunk: segment borders fall inside blocks and tiles.  Short windows and a short
    end_len: the chains hop a few elements.  The last list of several is half as long as the others, so many level-0 slots are
    infeasible."""
    rng = np.random.default_rng(2100 + k + seed)
    cases = []
    for n in sizes:
        span = 3 * n + 16
        lists = [_distinct(rng, n, span) for _ in range(k - 1)] + [_distinct(rng, n if k == 1 else max(1, n // 2), span)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 9)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 12))))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_many_short_queries_in_one_chunk(torch_cuda, oracle, k, mode):
    cases = _border_cases(k)
    assert [len(c[0][0]) for c in cases] == SIZES
    _check(torch_cuda, oracle, "short%d" % k, cases, mode, 1000)


def _mixed_k_cases():
    """k = 1, 2 and 3 in one batch: the level-0 range begins with the class of the three-list queries, not on a tile border, and the
    slots between two classes belong to no pass."""
    rng = np.random.default_rng(2107)
    cases = []
    for k, n in ((1, 700), (2, 1500), (3, 900), (1, 100), (3, 2100), (2, 40), (1, 3000), (2, 1025), (3, 33)):
        lists = [_distinct(rng, n, 4 * n) for _ in range(k)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(2, 12)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 9))))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_mixed_k_in_one_chunk(torch_cuda, oracle, mode):
    cases = _mixed_k_cases()
    want = _oracle(oracle, "mixed", cases)
    assert all(m > 0 for m, _ in want)
    _check(torch_cuda, oracle, "mixed", cases, mode, 2000)


def _sparse_last_cases(k):
    """k = 2 and 3 with a sparse last list: most level-0 slots are infeasible, raw targets move to the next feasible slot or leave their
    segment, and chains end in the middle of a tile (and of a look-ahead: the first query is heavy)."""
    rng = np.random.default_rng(2110 + k)
    cases = []
    for n, share in ((LONG, 0.3), (5000, 0.05), (3000, 0.5), (LONG + 100, 0.02), (1500, 0.1)):
        a = _run(n) * np.uint64(3)
        keep = np.sort(rng.choice(n, size=max(1, int(n * share)), replace=False))
        # partners for the kept elements only, in runs so that whole blocks are infeasible between them
        keep = np.unique(np.concatenate([keep[:len(keep) // 2], np.arange(n // 3, n // 3 + len(keep) // 2)]))
        lists = [a] + [a + np.uint64(1)] * (k - 2) + [a[keep] + np.uint64(k - 1)]
        one = [1] * (k - 1)
        cases.append((lists, one, one, int(rng.integers(1, 40))))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [2, 3])
def test_sparse_last_list(torch_cuda, oracle, k, mode):
    cases = _sparse_last_cases(k)
    want = _oracle(oracle, "sparse%d" % k, cases)
    assert all(m > 0 for m, _ in want)
    _check(torch_cuda, oracle, "sparse%d" % k, cases, mode, 3000)


def _heavy_cases():
    """Single-list queries, so the level-0 slots begin at slot 0 and the segments follow each other: segments of 63, exactly 64 and 65
    tiles (the second begins on a tile border, the third has one slot more), light queries between the heavy ones, and heavy ones that
    begin inside a tile.  end_len 1: dense chains, every entry is the first word of a head.  end_len 17 and 100: most entries lie
    behind the 16 head slots.  end_len 5: entries among the heads.  Every heavy segment ends inside the look-ahead window of its last
    rounds, and the next segment's words lie behind it."""
    shapes = [(63 * TILE, 1), (64 * TILE, 1), (64 * TILE + 1, 1), (5, 1), (1023, 2), (LONG, 17), (300, 3), (LONG, 100), (LONG, 5),
              (64 * TILE - 1022, 1), (77, 1)]
    return [([_run(n, 11 * i)], [], [], e) for i, (n, e) in enumerate(shapes)]


def _segment_tiles(cases):
    """tiles every first list's segment overlaps, for single-list queries (see the module's docstring)"""
    out, at = [], 0
    for lists, _, _, _ in cases:
        n = len(lists[0])
        out.append((at + n - 1) // TILE - at // TILE + 1)
        at += n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_heavy_queries_beside_light_ones(torch_cuda, oracle, mode):
    cases = _heavy_cases()
    tiles = _segment_tiles(cases)
    assert tiles[:3] == [WALK_WAVE_TILES - 1, WALK_WAVE_TILES, WALK_WAVE_TILES + 1]
    assert tiles[9] == WALK_WAVE_TILES and sum(1 for t in tiles if t >= WALK_WAVE_TILES) == 6
    want = _oracle(oracle, "heavy", cases)
    assert [m for m, _ in want] == [-(-len(c[0][0]) // c[3]) for c in cases]
    _check(torch_cuda, oracle, "heavy", cases, mode, 190000)


def _heavy_join_cases():
    """k = 2 and 3 with heavy first lists of random positions: the entries fall where the data puts them, a few slots into a tile."""
    return _border_cases(2, [LONG, 100, LONG + 513], seed=50) + _border_cases(3, [LONG + 1, 2000], seed=60)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_heavy_joins_of_two_and_three_lists(torch_cuda, oracle, mode):
    cases = _heavy_join_cases()
    _check(torch_cuda, oracle, "heavy_join", cases, mode, 5000)
