"""The build-time constants of csrc/ reject the values their kernels do not support (static_assert), checked by compiling one
translation unit per group of tunables with -fsyntax-only for gfx950; no device needed."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlg_matching_amd", "csrc")

# (translation unit, macro, an illegal value, what the static_assert says)
ILLEGAL = [
    ("search.hip", "VLG_LINK_RUN", 100, "VLG_LINK_RUN: a multiple of 64"),
    ("search.hip", "VLG_COOP_WINDOWS2", 0, "VLG_COOP_WINDOWS2: at least one"),
    ("search.hip", "VLG_RUNG_SHIFT", 1, "VLG_RUNG_SHIFT: 2 .. 8"),
    ("search.hip", "VLG_PIVOT_GROUPS", 0, "VLG_PIVOT_GROUPS: at least one"),
    ("search.hip", "VLG_PIVOT_TURNS", 0, "VLG_PIVOT_TURNS: at least one"),
    ("search.hip", "VLG_COMPACT_RUNS", 65, "VLG_COMPACT_RUNS: 1 .. 64"),
    ("search.hip", "VLG_SPARSE_TURN", 0, "VLG_SPARSE_TURN: 1 .. 32"),
    ("search.hip", "VLG_BUCKET_SORT", 2, "VLG_BUCKET_SORT: 0 or 1"),
    ("search.hip", "VLG_WINDOW_SORT", 2, "VLG_WINDOW_SORT: 0 or 1"),
    ("search.hip", "VLG_WINDOW_RANK_LOOP", 2, "VLG_WINDOW_RANK_LOOP: 0 or 1"),
    ("search.hip", "VLG_WINDOWS_PER_TILE", 0, "VLG_WINDOWS_PER_TILE: at least one"),
    ("search.hip", "VLG_SORT_CLASSES", 4, "three or five classes"),
    ("search.hip", "VLG_FETCH_THREADS", 0, "VLG_FETCH_THREADS: at least one"),
    ("kernels.hip", "VLG_RESOLVE_HOPS", 0, "VLG_RESOLVE_HOPS: at least one hop"),
    ("kernels.hip", "VLG_RESOLVE_CHUNK", 100, "VLG_RESOLVE_CHUNK: whole turns"),
    ("kernels.hip", "VLG_GROUP_CHUNK", 16384, "VLG_GROUP_CHUNK: s_rec + s_idx + s_bin must fit"),
    ("kernels.hip", "VLG_STAGE_LISTS", 2, "VLG_STAGE_LISTS: 0 or 1"),
    ("kernels.hip", "VLG_SWEEP_PAIRS", 2, "VLG_SWEEP_PAIRS: 0 or 1"),
]


def _hipcc():
    h = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(h):
        pytest.skip("hipcc not installed")
    return h


def _syntax_errors(tu, defs):
    cmd = [_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-ferror-limit=0"] + defs + [tu]
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    return out.returncode, out.stderr


@pytest.mark.parametrize("tu", sorted({t for t, _, _, _ in ILLEGAL}))
def test_every_tunable_rejects_an_illegal_value(tu):
    """All illegal values of one translation unit at once: each must fail its own static_assert (the compiler reports them all)."""
    cases = [c for c in ILLEGAL if c[0] == tu]
    rc, err = _syntax_errors(tu, ["-D%s=%d" % (m, v) for _, m, v, _ in cases])
    assert rc != 0
    failed = re.findall(r"static assertion failed[^\n]*", err)
    for _, macro, value, says in cases:
        assert any(says in line for line in failed), (macro, value, "\n".join(failed))


@pytest.mark.parametrize("tu", ["search.hip", "kernels.hip"])
def test_the_defaults_pass_the_static_asserts(tu):
    rc, err = _syntax_errors(tu, [])
    assert rc == 0, err[-3000:]
