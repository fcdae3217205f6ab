"""The one-pass class of the list sort (csrc/list_sort.hpp: kOnePassMax, workspace option "sort_one_pass", vlg_sort_lists_u32 mode 3).

A long list (more than kSortTile keys) of at most VLG_ONE_PASS_MAX keys takes one ranking pass over its top 8 position bits, into the
second buffer, and its windows read it there; a longer list takes two passes over its top 16 bits and comes back first.  The lists,
tiles, chunks and windows of the two classes are numbered apart, so the cases put lists of both classes, short lists, 1-key and
empty lists next to each other in every order, and batches in which one class is empty.  numpy's sort is the truth; mode 1 (the
classes), mode 2 (four full passes) and mode 3 (mode 1 with every long list taking two passes) must agree key for key, and the number
of lists flagged as clustered must be what a numpy model of the plan kernel's rule says -- zero for every case built of spread lists,
so that no case passes by quietly taking the four full passes."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from util import skewed_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                      # kSortTile
WIN_MAX_LEN = 1 << 25            # kWinMaxLen


@pytest.fixture(scope="module")
def V():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import vlg_matching_amd as v
    v.lib()
    return v


@functools.lru_cache(maxsize=None)
def _shape():
    """(kWinSpan, kWinReach, kOnePassMax of the loaded library, the bound the cases are built around)"""
    from vlg_matching_amd import capi
    k = capi.build_constants()
    span = TILE // k["VLG_WINDOWS_PER_TILE"]
    reach = k["VLG_WINDOW_THREADS"] * k["VLG_WINDOW_ITEMS"] - span
    return span, reach, k["VLG_ONE_PASS_MAX"], k["VLG_ONE_PASS_MAX"] or 256 * (reach // 2)


def _windows_on():
    from vlg_matching_amd import capi
    return os.environ["VLG_WINDOW_SORT"][:1] != "0" if "VLG_WINDOW_SORT" in os.environ else capi.build_constants()["VLG_WINDOW_SORT"] != 0


def model_flagged(keys, bits, one_pass_class):
    """The plan kernel's rule for one list: at a border x = j * kWinSpan of the list ordered by its group bits (the top 8 position bits of
    a one-pass list, the top 16 of any other), the list is flagged if and only if the group of the key at x begins more than kWinReach
    keys before x; so is a list of more than kWinMaxLen keys.  Short lists, and all lists below 17 position bits, have no windows."""
    span, reach, one_max, _ = _shape()
    n = len(keys)
    if n <= TILE or bits < 17 or not _windows_on():
        return False
    if n > WIN_MAX_LEN:
        return True
    gbits = 8 if one_pass_class and n <= one_max else 16
    g = np.sort(keys.astype(np.uint64) >> np.uint64(bits - gbits))
    x = np.arange(span, n, span)
    return bool(((x - np.searchsorted(g, g[x], side="left")) > reach).any())


def model_clustered(lists, bits, mode):
    return 0 if mode == 2 else sum(model_flagged(x, bits, mode == 1) for x in lists)


def _spread(rng, n, bits=30):
    return rng.choice(1 << bits, n, replace=False).astype(np.uint32)


def _padded(lists):
    """a 1-key list and an empty list between every two lists"""
    out = []
    for i, x in enumerate(lists):
        out += [x, np.array([i], np.uint32), np.zeros(0, np.uint32)]
    return out[:-2]


def _staircase(rng, run, bits=30):
    """A one-pass list whose group 100 (of its top 8 bits) is nothing but a run of `run` consecutive positions, placed at the window
    border x = 3 kWinSpan by the number of spread keys in the groups below it (20000 more lie above).  run = kWinReach: the group fills
    [x - kWinReach, x), it ends on the border and the key at x opens the next group; kWinReach + 1: [x - kWinReach, x], the key at x is
    the group's last and the group begins exactly kWinReach before it -- the longest within reach; kWinReach + 2: [x - kWinReach - 1, x],
    one key too many."""
    span, reach, _, _ = _shape()
    w = 1 << (bits - 8)
    x = 3 * span
    below = rng.choice(100 * w, x - reach - (1 if run > reach + 1 else 0), replace=False)
    above = 101 * w + rng.choice((1 << bits) - 101 * w, 20000, replace=False)
    return rng.permutation(np.concatenate([below, 100 * w + 1000 + np.arange(run), above])).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _cases():
    """{name: (lists, position bits, built of spread lists only)}, built once; the sorted truth is added by _truth()"""
    span, reach, _, M = _shape()
    rng = np.random.default_rng(2024)
    c = {}
    borders = [_spread(rng, n) for n in (TILE, TILE + 1, M - 1, M, M + 1, 2 * M)]
    c["borders"] = (borders, 30, True)
    c["borders_reversed"] = (borders[::-1], 30, True)
    c["borders_padded"] = (_padded(borders), 30, True)
    c["borders_reversed_padded"] = (_padded(borders[::-1]), 30, True)
    # one class empty: its sub-range of tiles, chunks and windows has no member; whole tiles and one key more
    c["one_pass_only"] = ([_spread(rng, n) for n in (2 * TILE, 2 * TILE + 1, min(50000, M))], 30, True)
    c["two_pass_only"] = ([_spread(rng, n) for n in (M + 1, M + M // 2 + 7)], 30, True)
    # 17 bits, the fewest the windows run on: every position of the text in one list of kOnePassMax keys, groups of 512 at the default
    c["17bit"] = ([rng.permutation(np.arange(min(M, 1 << 17), dtype=np.uint32)), _spread(rng, 9000, 17)], 17, True)
    hi = [np.unique(np.concatenate([rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint64), [2 ** 32 - 2, 0]])).astype(np.uint32) for n in (70000, 300000)]
    c["32bit"] = ([rng.permutation(h) for h in hi], 32, True)
    # clustered one-pass lists
    island = np.unique(np.concatenate([_spread(rng, 60000), 777_000_000 + np.arange(reach + 2048, dtype=np.uint32)]))
    island = rng.permutation(island)
    c["island"] = ([island], 30, False)
    c["island_between"] = ([_spread(rng, M + 5000), island, _spread(rng, 30000)], 30, False)
    c["equal_keys"] = ([np.full(5000, 123_456_789, np.uint32), _spread(rng, 6000)], 30, False)
    for d in (0, 1, 2):
        c["run_reach_plus_%d" % d] = ([_staircase(rng, reach + d), _spread(rng, 10000)], 30, False)
    return c


@functools.lru_cache(maxsize=None)
def _truth(name):
    lists, bits, spread = _cases()[name]
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return np.concatenate(lists).astype(np.uint32), off, np.concatenate([np.sort(x) for x in lists])


CASES = ["borders", "borders_reversed", "borders_padded", "borders_reversed_padded", "one_pass_only", "two_pass_only", "17bit", "32bit",
         "island", "island_between", "equal_keys", "run_reach_plus_0", "run_reach_plus_1", "run_reach_plus_2"]


def test_the_case_table_is_complete():
    assert sorted(CASES) == sorted(_cases())


@pytest.mark.parametrize("name", CASES)
def test_one_pass_lists_sort_like_numpy_in_every_mode(V, name):
    import torch
    span, reach, one_max, M = _shape()
    lists, bits, spread = _cases()[name]
    flat, off, want = _truth(name)
    assert len(flat) < 2_000_000
    if spread:                                       # the guard: nothing here may be flagged, with the class or without it
        for x in lists:
            assert not model_flagged(x, bits, True) and not model_flagged(x, bits, False), (name, len(x))
    if name.startswith("island"):
        assert model_flagged(lists[name == "island_between"], bits, True)
    if name == "run_reach_plus_0" or name == "run_reach_plus_1":
        assert not model_flagged(lists[0], bits, True), name
    if name == "run_reach_plus_2" and one_max:
        assert model_flagged(lists[0], bits, True)
    L = V.lib()
    for mode in (1, 2, 3):
        d = torch.from_numpy(flat.view(np.int32).copy()).cuda()
        nc = C.c_uint64(99)
        V.capi.check(L.vlg_sort_lists_u32(d.data_ptr(), off.ctypes.data, len(lists), bits, mode, C.byref(nc), None))
        got = d.cpu().numpy().view(np.uint32)
        assert (got == want).all(), (name, mode, int(np.argmax(got != want)))
        expect = model_clustered(lists, bits, mode)
        print("%s mode %d: n_clustered %d, model %d" % (name, mode, nc.value, expect))
        assert nc.value == expect, (name, mode, nc.value, expect)
        if spread:
            assert nc.value == 0, (name, mode)


def test_mode_4_is_refused(V):
    off = np.array([0, 1], dtype=np.uint64)
    with pytest.raises(V.VlgError):
        V.capi.check(V.lib().vlg_sort_lists_u32(None, off.ctypes.data, 1, 30, 4, None, None))


# ---- through the search path ------------------------------------------------------------------------------------------------------
# The parity tests' Zipf text (util.skewed_text), 400 000 symbols where they take 40 000: the windows need 17 position bits, and at this
# length the commonest symbols' lists lie on both sides of the small variant's bound (8192) AND of the default one (131072).
def _search_both_ways(V):
    from vlg_matching_amd import capi
    from vlg_matching_amd.index import Workspace
    text = skewed_text(400000, 3)
    one_max = capi.build_constants()["VLG_ONE_PASS_MAX"]
    sym = [int(s) for s in np.argsort(-np.bincount(text, minlength=256))[:12]]
    occ = np.bincount(text, minlength=256)
    lens = [int(occ[s]) for s in sym]
    assert any(TILE < n <= one_max for n in lens) and any(n > one_max for n in lens), (one_max, lens)
    ch = [chr(s) for s in sym]
    qs = ["%s.{0,6}?%s.{1,9}?%s" % (ch[i], ch[(i + 3) % 12], ch[(i + 7) % 12]) for i in range(12)] + ["%s.{0,3}?%s" % (a, b) for a, b in zip(ch, ch[1:])] + ch
    idx = V.VlgIndex.build(text.tobytes())
    res = []
    for on in (0, 1):
        ws = Workspace()
        ws.set_option("sort_one_pass", on)
        res.append(idx.search(qs, workspace=ws))
    off, on = res
    assert on.summary["n_matches"] > 100000
    for k in ("n_matches", "checksum", "located_occurrences"):
        assert on.summary[k] == off.summary[k], k
    for x, y in zip(on.fetch(), off.fetch()):
        assert (x == y).all()
    # the one-symbol queries: every occurrence, ascending -- the sorted lists themselves
    counts, offsets, first, _ = on.fetch()
    for j, s in enumerate(sym):
        q = len(qs) - 12 + j
        assert (first[int(offsets[q]):int(offsets[q + 1])] == np.flatnonzero(text == s)).all(), chr(s)


def test_search_is_the_same_with_and_without_one_pass_lists(V):
    assert os.environ.get("VLG_CHECK_SORT") == "1"
    _search_both_ways(V)


def test_search_on_the_small_variant(V):
    """The same batch on the library compiled with VLG_ONE_PASS_MAX = 8192 (variants.py: "small"), in a process of its own."""
    from vlg_matching_amd import variants
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = ("import sys; sys.path.insert(0, %r); import torch; assert torch.cuda.is_available(); import vlg_matching_amd as v; v.lib(); "
            "assert v.capi.build_constants()['VLG_ONE_PASS_MAX'] == %d; import test_gpu_sort_one_pass as t; t._search_both_ways(v); print('ok')"
            % (os.path.join(ROOT, "tests"), variants.constants("small")["VLG_ONE_PASS_MAX"]))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=ROOT,
                         env=dict(os.environ, VLG_HIP_LIBRARY=lib, VLG_CHECK_SORT="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout + out.stderr)[-3000:]
