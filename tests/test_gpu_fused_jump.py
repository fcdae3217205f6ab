"""The level-0 jump found inside the link pass (join_device.hpp: join_link_kernel<.., kJump>) and settled by the tile pass.

Every case goes through vlg_join_batch on caller-made lists and is compared with the oracle's merge join: counts, first positions,
tuples and checksum.  Each runs with the workspace option "fuse_jump" 1 (the fused pass) and 0 (the separate jump pass, whose settled
output passes through the same settling unchanged), with and without tuples.  The cases sit on the borders of the fused pass: its
64- and 128-key steps, its 256-element staged stretch, the runs of VLG_LINK_RUN slots, the 1024-slot chain tiles, the segment
borders inside each of them, and the summary levels of the feasibility bitset."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
MODES = [(f, t) for f in (1, 0) for t in (1, 0)]          # (fuse_jump, tuples)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


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
    d = _dev_u64(torch, np.concatenate(flat))
    return join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws)


_want = {}


def _oracle(oracle, name, cases):
    """The oracle's answers of a named set of cases, computed once and shared by the modes."""
    if name not in _want:
        _want[name] = [oracle.join(*c) for c in cases]
    return _want[name]


def _check(torch, oracle, name, cases, fuse, tuples, opts=None, cap=None):
    want = _oracle(oracle, name, cases)
    o = {"filter": 0}
    o.update(opts or {})
    o.update({"fuse_jump": fuse, "tuples": tuples})
    res = _join(torch, cases, o, cap)
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
    return res, total


def _distinct(rng, n, span):
    return np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64)


def _border_cases(k, offset=0, sizes=SIZES):
    """One join per first-list length, all in one chunk: the segments of a class follow each other in query order, so their borders
    fall inside 64-key steps, 128-key pairs, runs and chain tiles.  Short windows and short end_len: the chains hop a few elements."""
    rng = np.random.default_rng(1600 + k)
    cases = []
    for n in sizes:
        span = 3 * n + 16
        lists = [_distinct(rng, n, span) + np.uint64(offset) for _ in range(k - 1)] + [_distinct(rng, max(1, n // 2), span) + np.uint64(offset)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 9)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 12))))
    return cases


@pytest.mark.parametrize("fuse,tuples", MODES)
@pytest.mark.parametrize("k", [2, 3])
def test_borders_of_steps_blocks_runs_and_tiles(torch_cuda, oracle, k, fuse, tuples):
    cases = _border_cases(k)
    assert [len(c[0][0]) for c in cases] == SIZES
    res, total = _check(torch_cuda, oracle, "borders%d" % k, cases, fuse, tuples)
    assert res.summary["n_chunks"] == 1 and total > 1000


@pytest.mark.parametrize("fuse,tuples", MODES)
@pytest.mark.parametrize("k", [2, 3])
def test_borders_through_the_window_filter(torch_cuda, oracle, k, fuse, tuples):
    """filter on: the joins run on the survivors' private lists behind the shared ones, with fences of their own"""
    _check(torch_cuda, oracle, "borders%d" % k, _border_cases(k), fuse, tuples, {"filter": 1, "filter_min": 0, "filter_stream_min": 0})


def _far_cases(offset=0):
    """A dense first list whose chain ends lie `g` elements ahead: every element has its partner, exactly g positions on (k = 3:
    through a middle list one position on), so end + end_len is element g + 1 (g + 2) behind the element -- beyond the 256 staged
    elements, beyond 1024, beyond the 4096 elements of the far search's first round, and behind the list (jump = none)."""
    cases = []
    for n, g in ((6000, 300), (6000, 1500), (12000, 5000), (3000, 4000)):
        a = np.arange(n, dtype=np.uint64) + np.uint64(offset)
        cases.append(([a, a + np.uint64(g)], [g], [g], 1))
        cases.append(([a, a + np.uint64(1), a + np.uint64(1 + g)], [1, g], [1, g], 1))
    return cases


@pytest.mark.parametrize("fuse,tuples", MODES)
def test_answer_beyond_the_staged_stretch(torch_cuda, oracle, fuse, tuples):
    cases = _far_cases()
    want = _oracle(oracle, "far", cases)
    # a chain of hops g + 1 (g + 2) elements long; one match where the answer lies behind the list
    assert [m for m, _ in want] == [20, 20, 4, 4, 3, 3, 1, 1]
    _check(torch_cuda, oracle, "far", cases, fuse, tuples)


def _neighbour_cases(k):
    """Two joins side by side in a class.  The tail of the first one's list 0 has no partner (infeasible), the head of the second
    one's list 0 is feasible: the raw target of the first join's last match lies in its infeasible tail, and the next feasible slot
    behind it belongs to the neighbour."""
    a = np.arange(0, 3000, 10, dtype=np.uint64)                       # 300 elements; partners for the first 100
    b = np.arange(5, 2005, 10, dtype=np.uint64)                       # 200 elements, all with a partner
    mid = [] if k == 2 else [1]
    first = [a] + [a + np.uint64(1)] * (k - 2) + [a[:100] + np.uint64(k - 1)]
    second = [b] + [b + np.uint64(1)] * (k - 2) + [b + np.uint64(k - 1)]
    return [(first, mid + [1], mid + [1], 1), (second, mid + [1], mid + [1], 1)]


@pytest.mark.parametrize("fuse,tuples", MODES)
@pytest.mark.parametrize("k", [2, 3])
def test_settling_does_not_cross_a_segment(torch_cuda, oracle, k, fuse, tuples):
    cases = _neighbour_cases(k)
    want = _oracle(oracle, "neighbours%d" % k, cases)
    assert [m for m, _ in want] == [100, 200]
    _check(torch_cuda, oracle, "neighbours%d" % k, cases, fuse, tuples)


def _sparse_cases(k):
    """More than 3 x 64 x 64 infeasible level-0 slots in a row between a raw target and the next feasible slot: whatever the
    alignment, whole words of the first and the second summary level are zero there, and next_feasible climbs them."""
    n = 14000
    a = np.arange(0, 10 * n, 10, dtype=np.uint64)
    live = np.concatenate([a[:10], a[-10:]])
    lists = [a] + [a + np.uint64(1)] * (k - 2) + [live + np.uint64(k - 1)]
    one = [1] * (k - 1)
    return [(lists, one, one, 1)]


@pytest.mark.parametrize("fuse,tuples", MODES)
@pytest.mark.parametrize("k", [2, 3])
def test_sparse_feasibility_climbs_the_summary_levels(torch_cuda, oracle, k, fuse, tuples):
    cases = _sparse_cases(k)
    assert _oracle(oracle, "sparse%d" % k, cases)[0][0] == 20
    _check(torch_cuda, oracle, "sparse%d" % k, cases, fuse, tuples)


def _mixed_k_join_cases():
    """Joins of 1, 2, 3 and 5 lists (two of them dead) whose first lists land in the classes 0, 1, 2 and 4 of one chunk, with lengths on
    both sides of the class alignment (64 slots) and of the chain tile (1024 slots), and lists shorter than kMinPiece (128)."""
    rng = np.random.default_rng(20261018)
    lens = [[65], [63, 10], [64, 1, 7], [1, 130, 2, 1025, 3], [50, 0], [0], [1023, 1024, 1]]
    span, cases = 6000, []
    for ln in lens:
        lists = [np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64) for n in ln]
        lo = [int(rng.integers(0, 20)) for _ in ln[1:]]
        hi = [l + int(rng.integers(1500, 3000)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 9))))
    # one match made by hand, from the single element of the five-list join's first list
    lists, lo, hi, _ = cases[3]
    p = 100
    for i, a in enumerate(lists):
        p += lo[i - 1] if i else 0
        others = rng.choice(span, size=len(a) + 1, replace=False)
        lists[i] = np.sort(np.append(others[others != p][:len(a) - 1], p)).astype(np.uint64)
    # ... and longer joins of every k beside them, so that every class holds first lists and other levels side by side
    rng = np.random.default_rng(1605)
    for k, n in ((1, 700), (2, 1500), (3, 900), (5, 1100), (1, 100), (3, 100), (2, 40)):
        lists = [_distinct(rng, n, 4 * n) for _ in range(k)]
        lo = [int(rng.integers(0, 3)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(2, 12)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 9))))
    return cases


@pytest.mark.parametrize("fuse,tuples", MODES)
def test_mixed_k_in_one_chunk(torch_cuda, oracle, fuse, tuples):
    cases = _mixed_k_join_cases()
    want = _oracle(oracle, "mixed", cases)
    assert want[4][0] == 0 and want[5][0] == 0 and sum(1 for m, _ in want if m) >= 9
    res, _ = _check(torch_cuda, oracle, "mixed", cases, fuse, tuples)
    assert res.summary["n_chunks"] == 1


@pytest.mark.parametrize("fuse,tuples", MODES)
def test_wide_positions(torch_cuda, oracle, fuse, tuples):
    """values above 2^32: the 64-bit instantiations"""
    off = (1 << 33) + 12345
    sizes = [65, 129, 513, 1025, 2049]
    cases = _border_cases(2, off, sizes) + _border_cases(3, off, sizes) + _far_cases(off)[2:]
    assert min(int(c[0][0][0]) for c in cases) > 1 << 32
    _, total = _check(torch_cuda, oracle, "wide", cases, fuse, tuples)
    assert total > 500


def _chunk_cases():
    rng = np.random.default_rng(77)
    cases = []
    for _ in range(60):
        k = int(rng.integers(1, 4))
        lists = [_distinct(rng, int(n), 400000) for n in rng.integers(1000, 30000, k)]
        lo = [int(rng.integers(0, 151)) for _ in range(k - 1)]
        hi = [l + int(rng.integers(0, 301)) for l in lo]
        cases.append((lists, lo, hi, int(rng.integers(1, 9))))
    return cases


@pytest.mark.parametrize("fuse,tuples", MODES)
def test_several_join_chunks(torch_cuda, oracle, fuse, tuples):
    """a small workspace: the joins are cut into several chunks, each with its own slots, classes and tiles"""
    res, total = _check(torch_cuda, oracle, "chunks", _chunk_cases(), fuse, tuples, cap=40 << 20)
    assert res.summary["n_chunks"] > 1 and total > 0


def test_small_variant_runs_these_cases():
    """VLG_LINK_RUN = 192: runs end inside a 128-key pair and inside the staged stretch.  The cases above once more, in a child pytest
    that loads the `small` build."""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; print(json.dumps(capi.build_constants()['VLG_LINK_RUN']))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "192", out.stdout + out.stderr
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_fused_jump.py", "-k", "not small_variant"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) >= 48, tail                 # every case above, in every mode
