"""Document listing (vlg_result_list_documents, vlg_doc_listing_*) without a device: header, library and binding stay in step, NULL
handles are refused on the host, the arithmetic of csrc/doc_list_math.hpp agrees with naive loops in a stand-alone program (also under
ASan + UBSan), and an emulation of the head pass -- 64 lanes per step, runs of 192 and 2048 matches, the document of the match in
front of lane 0 and the query of the step carried from step to step -- gives the naive listing when heads fall on lane 0, on lane 63 and
on the first match of a run.  What needs a result needs a device: tests/test_gpu_doc_listing.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("vlg_result_list_documents", 4), ("vlg_doc_listing_info", 3), ("vlg_doc_listing_fetch", 6), ("vlg_doc_listing_destroy", 1))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as V
    return V


def test_header_library_and_binding_stay_in_step(V):
    src = open(os.path.join(ROOT, "include", "vlg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(V.library_path())
    bound = {s[0]: s for s in V.capi.SYMBOLS}
    for name, nargs in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(L, name), "library does not export " + name
        assert name in bound and len(bound[name][2]) == nargs
        assert "void* stream" not in m.group(1) and "vlg_workspace" not in m.group(1)      # null stream, no workspace
    assert re.search(r"enum\s*\{\s*VLG_DOCLIST_DF\s*=\s*0\s*,\s*VLG_DOCLIST_PAIRS\s*=\s*1\s*\}", code)
    assert (V.capi.DOCLIST_DF, V.capi.DOCLIST_PAIRS) == (0, 1)
    # the contract is written down where a caller looks for it, with what it replaces
    block = src[src.index("Document listing:"):src.index("typedef struct vlg_doc_listing")]
    for word in ("vlg_result_fetch", "vlg_documents_locate_batch", "run-length", "first_match", "null stream", "VLG_E_UNSUPPORTED", "*out untouched",
                 "query border"):
        assert word in block, word
    assert V.capi.build_constants()["VLG_DOCLIST_RUN"] == 2048 or os.environ.get("VLG_HIP_LIBRARY")


def test_null_handles_are_refused_on_the_host(V):
    L = V.lib()
    out = C.c_void_p(7)
    for what in (0, 1, 2, -1):
        assert L.vlg_result_list_documents(None, None, what, C.byref(out)) == V.capi.E_INVALID
        assert out.value == 7                                               # (nothing was written)
    assert L.vlg_result_list_documents(None, None, 0, None) == V.capi.E_INVALID
    assert b"null" in L.vlg_last_error()
    n = C.c_uint64(9)
    assert L.vlg_doc_listing_info(None, C.byref(n), C.byref(n)) == V.capi.E_INVALID and n.value == 9
    assert L.vlg_doc_listing_fetch(None, None, None, None, None, None) == V.capi.E_INVALID
    L.vlg_doc_listing_destroy(None)


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "doc_list_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_listing_arithmetic_against_naive_loops(tmp_path):
    _build_and_run(tmp_path, "doc_list_check", [])


def test_listing_arithmetic_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "doc_list_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_run_length_rejects_an_illegal_value():
    """VLG_DOCLIST_RUN: a multiple of 64 (a step writes its word of head bits whole), as tests/test_build_constants_cpu.py asks of
    the other tunables"""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-ferror-limit=0", "-DVLG_DOCLIST_RUN=96", "search.hip"],
                         cwd=os.path.join(ROOT, "vlg_matching_amd", "csrc"), capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert any("VLG_DOCLIST_RUN: a multiple of 64" in line for line in re.findall(r"static assertion failed[^\n]*", out.stderr)), out.stderr[-2000:]


# ---- the head pass, lane by lane---------------------------------------------------------------------------------------------------
def naive_listing(pos, off, starts):
    """-> (df, docs, counts, first_match): per query the maximal runs of equal documents"""
    doc = np.searchsorted(np.asarray(starts, np.uint64), np.asarray(pos, np.uint64), "right") - 1
    df, docs, counts, first = [], [], [], []
    for q in range(len(off) - 1):
        a, b = int(off[q]), int(off[q + 1])
        n = 0
        for i in range(a, b):
            if i > a and docs[-1] == doc[i]:
                counts[-1] += 1
            else:
                docs.append(int(doc[i])); counts.append(1); first.append(i); n += 1
        df.append(n)
    return df, docs, counts, first


def emulate(pos, off, starts, R):
    """The head pass as the kernel runs it (one piece): per run the query of its first match by a search over the offsets and the
    document of the match in front of it by one extra lookup; per step of 64 lanes the documents, the query borders found 64 offsets
    at a time, the predecessor's document from the neighbouring lane (lane 0: carried), one word of head bits.  Then the scan, the
    ranks at the query borders and the scatter.  -> (df, docs, counts, first_match, heads as (run, step, lane))"""
    pos, off, B = np.asarray(pos, np.uint64), [int(x) for x in off], np.asarray(starts, np.uint64)
    m, nq = len(pos), len(off) - 1
    lookup = lambda x: int(np.searchsorted(B, x, "right")) - 1
    n_runs = -(-m // R)
    bits, run_heads, where = {}, [0] * (n_runs + 1), []
    for run in range(n_runs):
        rb, re_ = run * R, min(m, run * R + R)
        q = int(np.searchsorted(off, rb + 1, "left")) - 1                   # off[q] <= rb < off[q + 1]
        assert off[q] <= rb < off[q + 1]
        q_end, first0 = off[q + 1], off[q] == rb
        carry = lookup(pos[rb - 1]) if rb else None
        for s in range(rb, re_, 64):
            lanes = min(64, re_ - s)
            d = [lookup(pos[s + l]) for l in range(lanes)]
            firsts = 1 if (s == rb and first0) else 0
            step_end = s + lanes
            while q_end < step_end:
                assert q_end >= s
                window = off[q + 1:q + 65]                                  # 64 offsets a round, as 64 lanes load them
                inside = [v for v in window if v < step_end]
                assert inside
                for v in inside:
                    firsts |= 1 << (v - s)
                q += len(inside)
                q_end = off[q + 1]
            word = 0
            for l in range(lanes):
                prev = carry if l == 0 else d[l - 1]
                if (firsts >> l) & 1 or d[l] != prev:
                    word |= 1 << l
                    where.append(((s - rb) // 64, l, s + l == rb))
            bits[s // 64] = word
            run_heads[run] += bin(word).count("1")
            carry = d[-1]                                                   # (lane 63; a short step is the run's last)
    rank = np.concatenate([[0], np.cumsum(run_heads)]).tolist()

    def rank_of(g):
        if g >= m:
            return rank[n_runs]
        r = rank[g // R] + sum(bin(bits[w]).count("1") for w in range((g // R) * R // 64, g // 64))
        return r + bin(bits[g // 64] & ((1 << (g % 64)) - 1)).count("1")
    pair_off = [rank_of(off[q]) for q in range(nq + 1)]
    docs, first = [None] * rank[n_runs], [None] * rank[n_runs]
    for g in range(m):
        if (bits[g // 64] >> (g % 64)) & 1:
            docs[rank_of(g)], first[rank_of(g)] = lookup(pos[g]), g
    counts = []
    for q in range(nq):
        for p in range(pair_off[q], pair_off[q + 1]):
            counts.append((first[p + 1] if p + 1 < pair_off[q + 1] else off[q + 1]) - first[p])
    return [pair_off[q + 1] - pair_off[q] for q in range(nq)], docs, counts, first, where


def _sets(R, m):
    """document sets over positions 0, 2, 4, ...: match e stands at 2 e, so a start at 2 e makes match e a head"""
    n = 2 * m
    s = {
        "lane0": list(range(0, n, 128)), "lane1": [0] + list(range(130, n, 128)), "lane63": [0] + list(range(126, n, 128)),
        "run_first": [0, 2 * R, 4 * R], "run_second": [0, 2 * R + 2], "run_last": [0, 2 * R - 2],
        "spanning": [0, 2 * (R + R // 2)], "every": list(range(0, n, 2)), "single": [0],
    }
    return s


@pytest.mark.parametrize("R", [192, 2048])
def test_the_carry_of_the_head_pass(R):
    m = 2 * R + R // 2 + 37                                                 # three runs, the last one short, its last step short
    pos = np.arange(m, dtype=np.uint64) * 2
    # one query; queries that end on a step, on a run, one behind it; empty queries at the front, several in a row, at the end
    offsets = {
        "one": [0, m],
        "borders": [0, 0, 64, 64, 64, 65, 127, 128, R - 1, R, R + 1, 2 * R, 2 * R, 2 * R + 64, m, m, m],
        "ones": list(range(0, 200)) + [m],                                  # 199 queries of one match: more than 64 borders in a row
    }
    lanes_seen, run_first_seen = set(), False
    for oname, off in offsets.items():
        for sname, starts in _sets(R, m).items():
            want = naive_listing(pos, off, starts)
            got = emulate(pos, off, starts, R)
            assert tuple(got[:4]) == want, (oname, sname)
            if oname == "one":                                              # the heads fall where the set aims them
                lanes = {l for _, l, _ in got[4][1:]}
                if sname in ("lane0", "lane1", "lane63"):
                    assert lanes == {int(sname[4:])}, (sname, lanes)
                if sname == "run_first":
                    assert [w for w in got[4] if w[2]] == [(0, 0, True)] * 3
                if sname == "run_second":
                    assert got[4][1][:2] == (0, 1)
                if sname == "run_last":
                    assert got[4][1][:2] == ((R - 1) // 64, (R - 1) % 64)
                if sname == "spanning":
                    assert len(got[4]) == 2 and not got[4][1][2]
                lanes_seen |= lanes
                run_first_seen |= any(w[2] for w in got[4][1:])
    assert {0, 1, 63} <= lanes_seen and run_first_seen


def test_the_carry_with_positions_that_ascend_only_inside_a_query():
    """random queries over random documents: the document of a step is bracketed by its smallest and largest key"""
    rng = np.random.default_rng(4)
    for R in (192, 2048):
        for _ in range(6):
            counts = rng.choice([0, 0, 1, 2, 63, 64, 65, 300, 700], 14)
            pos = np.concatenate([np.sort(rng.integers(0, 9000, c)) for c in counts] + [np.zeros(0, np.int64)]).astype(np.uint64)
            off = np.concatenate([[0], np.cumsum(counts)]).tolist()
            if not len(pos):
                continue
            starts = sorted({0} | {int(x) for x in rng.integers(1, 9000, int(rng.choice([1, 30, 2000])))})
            assert tuple(emulate(pos, off, starts, R)[:4]) == naive_listing(pos, off, starts)
