"""The cooperative searches of the link pass (join_device.hpp: wave_lower_bound, wave_lower_bound2 with its early window load,
wave_far_lower_bound) at the borders of their windows, far rounds and lists.

Every case goes through vlg_join_batch on caller-made lists and is compared with the oracle's merge join: counts, first positions,
tuples and checksum.  Each runs without the window filter and through it (the survivors' private lists), with "fuse_jump" 1 and 0,
with and without tuples, for k = 2 and 3, with 32-bit positions, with positions beyond 2^32 (the 64-bit instantiations) and with
positions that end just below 2^32 (the 32-bit search refuses the keys whose window begins beyond the positions' range).

A pair of steps holds 128 ascending keys, lane i the keys i and 64 + i; the windows are 64 consecutive elements of the next list from
the previous answer on, VLG_COOP_WINDOWS2 (4) of them, each loaded while the one before it is ranked, and the far search takes the
keys they did not reach: 64 blocks of 64 per round, four rounds, then a gallop.  The staircases put the answers of consecutive keys d
elements apart, so the windows of a pair hold keys of neither register, of one, or of both, the last window loaded lies before, on and
behind the list's end, and runs and steps end inside a pair; the split pairs leave one register, or half of one, to the far search;
the far cases put the answer in each stage of it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from vlg_matching_amd import variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(flt, f, t) for flt in (0, 1) for f in (1, 0) for t in (1, 0)]          # (filter, fuse_jump, tuples)
DS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]
NS = [128, 129, 191, 192, 193, 257]
LO = 7                                                      # lower gap bound of the searched gap: the key of x is x + LO
WIDE = (1 << 33) + 12345
RANGES = ["narrow", "wide", "edge"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


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
    d = torch.from_numpy(np.ascontiguousarray(np.concatenate(flat), dtype=np.uint64).view(np.int64)).cuda()
    return join_batch(d.data_ptr(), list_off, join_list, lo, hi, end_len, ws)


_want = {}


def _check(torch, oracle, name, cases, flt, fuse, tuples):
    if name not in _want:                                   # the oracle's answers, computed once and shared by the modes
        _want[name] = [oracle.join(*c) for c in cases]
    want = _want[name]
    opts = {"filter": flt, "fuse_jump": fuse, "tuples": tuples}
    if flt:
        opts.update({"filter_min": 0, "filter_stream_min": 0})
    res = _join(torch, cases, opts)
    total, chk = 0, 0
    for j, (m, t) in enumerate(want):
        assert int(res.counts[j]) == m, (name, j)
        assert res.positions(j).tolist() == t[:, 0].tolist(), (name, j)
        if tuples:
            assert res.tuples(j).tolist() == t.tolist(), (name, j)
        total += m
        chk = (chk + int(t[:, 0].sum())) % (1 << 64) if m else chk
    assert res.summary["n_matches"] == total and res.summary["checksum"] == chk, name
    return want, total


def _case(x, y, k, hi_extra=1):
    """The join of the keys x against the list y under the gap [LO, LO + hi_extra]; k = 3: through a middle list one position on, so
    that the searched gap is the last one (kLast) and the first gap is searched by the pass of the other class."""
    x = np.asarray(x, np.uint64)
    y = np.asarray(y, np.uint64)
    if k == 2:
        return ([x, y], [LO], [LO + hi_extra], 1)
    return ([x, x + np.uint64(1), y + np.uint64(1)], [1, LO], [1, LO + hi_extra], 1)


def _staircase(n, d, k):
    """n keys d + 1 apart; between the keys (x + LO) of two neighbours lie d elements of the next list, so the lower bounds of
    consecutive keys are d elements apart.  Of the d + 1 values from one key to the next the odd steps leave out the key itself (its
    answer is the element one above it, no match unless the gap reaches it) and the even steps the value behind the previous key.
    Five elements below every key and 70 above them all, so no length is a multiple of 64 by design and d = 0 has a list at all."""
    x = 100 + np.arange(n, dtype=np.int64) * (d + 1)
    key = x + LO
    parts = [np.arange(key[0] - 5, key[0], dtype=np.int64)]
    for i in range(1, n):
        v = np.arange(key[i - 1] + 1, key[i] + 1, dtype=np.int64)            # d + 1 values, the key last
        parts.append(v[:-1] if i % 2 else v[1:])
    parts.append(key[-1] + 3 + 2 * np.arange(70, dtype=np.int64))
    return _case(x, np.concatenate(parts), k)


def _window_last(k):
    """Windows of a dense list that start at its first element: keys equal to a window's last element and one above it (the answer
    is the first element of the next window), in both registers of a pair."""
    y = 1000 + 2 * np.arange(1500, dtype=np.int64)
    idx = np.array([0, 63, 127, 191, 255, 319, 383, 447, 511, 575, 639], dtype=np.int64)
    keys = np.unique(np.concatenate([y[idx], y[idx] + 1, y[5:700:6] - 1]))
    assert len(keys) >= 130
    return _case(keys - LO, y, k)


def _split(k, near, dist, ny=20000):
    """128 keys (and 192: a single step behind the pair): the first `near` land in the first window, the others `dist` elements on."""
    y = 500 + 3 * np.arange(ny, dtype=np.int64)
    out = []
    for n in (128, 192):
        at = np.concatenate([np.arange(near), dist + 2 * np.arange(n - near)])
        keys = np.where(at < ny, y[np.minimum(at, ny - 1)], y[-1] + 1 + at)              # behind the list: no element at or after the key
        out.append(_case(keys - LO, y, k))
    return out


def _far_cases(k):
    w = 64 * variants.DEFAULTS["VLG_COOP_WINDOWS2"]
    cases = []
    cases += _split(k, 64, w + 6 * 64)              # register 1 alone goes far
    cases += _split(k, 32, w + 6 * 64)              # half of register 0 and register 1
    cases += _split(k, 64, w + 1)                   # just beyond the windows
    cases += _split(k, 64, w + 4096 + 70)           # the second far round
    cases += _split(k, 64, w + 4 * 4096 + 70)       # behind the far rounds: the gallop
    cases += _split(k, 64, 30000)                   # behind the list's end: no link
    cases += _split(k, 1, 19990, ny=19999)          # ... and the last elements of a list whose length is no multiple of 64
    return cases


_cases = {}


def _all_cases(k):
    if k not in _cases:
        _cases[k] = [_staircase(n, d, k) for d in DS for n in NS] + [_window_last(k)] + _far_cases(k)
    return _cases[k]


def _in_range(cases, rng):
    """narrow: as made (32-bit positions).  wide: beyond 2^32.  edge: every join moved so that its largest key is 2^32 - 3 -- the
    windows of its last keys begin beyond 2^32 - 1 -- and the elements that no longer fit 32 bits dropped."""
    if rng == "narrow":
        return cases
    out = []
    for lists, lo, hi, e in cases:
        off = WIDE if rng == "wide" else (1 << 32) - 3 - int(lists[0][-1])
        moved = [a + np.uint64(off) for a in lists]
        if rng == "edge":
            moved = [a[a < np.uint64(1 << 32)] for a in moved]
        out.append((moved, lo, hi, e))
    return out


@pytest.mark.parametrize("flt,fuse,tuples", MODES)
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("rng", RANGES)
def test_staircases_split_pairs_and_far_answers(torch_cuda, oracle, rng, k, flt, fuse, tuples):
    cases = _in_range(_all_cases(k), rng)
    top = max(int(a[-1]) for c in cases for a in c[0] if len(a))
    assert (top >> 32 == 0) == (rng != "wide") and (rng != "edge" or top == (1 << 32) - 1)
    # a staircase is as long as its d and n make it (n d + 75 elements, 66 124 for the largest pair); every other list stays at 2 x 10^4
    assert len(cases) == len(DS) * len(NS) + 15
    assert max(len(a) for c in cases[:len(DS) * len(NS)] for a in c[0]) <= max(DS) * max(NS) + 75
    assert max(len(a) for c in cases[len(DS) * len(NS):] for a in c[0]) <= 20001
    want, total = _check(torch_cuda, oracle, "%s%d" % (rng, k), cases, flt, fuse, tuples)
    assert total > 5000
    # the cases do what they are there for: keys that link and keys that do not in one staircase; a far answer behind the list
    m = [w[0] for w in want]
    assert 0 < m[len(NS) + 1] < NS[1] and 0 < m[-3] <= 64 and 0 < m[-4] <= 64


def test_small_variant_runs_these_cases():
    """VLG_LINK_RUN = 192 and VLG_COOP_WINDOWS2 = 1: runs end inside a pair and every pair whose keys spread over more than one window
    goes far.  The cases above once more, in a child pytest that loads the `small` build."""
    lib = variants.library("small")
    assert os.path.exists(lib), "variant small is not built (run __graft_entry__.build())"
    code = "import json; from vlg_matching_amd import capi; c = capi.build_constants(); print(json.dumps([c['VLG_LINK_RUN'], c['VLG_COOP_WINDOWS2']]))"
    env = dict(os.environ, VLG_HIP_LIBRARY=lib)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    out = subprocess.run(cmd + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "[192, 1]", out.stdout + out.stderr
    out = subprocess.run(cmd + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_gpu_link_windows.py", "-k", "not small_variant"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((out.stdout + out.stderr).strip().splitlines()[-30:])
    assert out.returncode == 0, "child run failed:\n" + tail
    last = out.stdout.strip().splitlines()[-1]
    assert re.search(r"\b(failed|error|errors|skipped)\b", last) is None, tail
    m = re.search(r"(\d+) passed", last)
    assert m and int(m.group(1)) == len(RANGES) * 2 * len(MODES), tail            # every case above, in every mode
