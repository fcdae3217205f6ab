"""Match texts (vlg_result_extract_matches, vlg_match_texts_*) without a device: header, library and binding stay in step for the four
entry points, NULL handles are refused on the host before any device is asked for, and the rule of csrc/match_span.hpp agrees with
naive loops in a stand-alone program (also under ASan + UBSan; nothing is sanitized inside python).  What needs a result needs a
device: tests/test_gpu_match_texts.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("vlg_result_extract_matches", 10), ("vlg_match_texts_info", 4), ("vlg_match_texts_fetch", 4), ("vlg_match_texts_destroy", 1))
U64_MAX = (1 << 64) - 1


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
    args = bound["vlg_result_extract_matches"][2]
    assert all(a is C.c_uint64 for a in args[4:9])                              # flanks, slice and cap are 64 bits wide
    assert bound["vlg_match_texts_info"][2][3]._type_ is C.c_uint32
    # the contract is written down where a caller looks for it, with what it replaces
    block = src[src.index("Match texts:"):src.index("typedef struct vlg_match_texts")]
    for word in ("vlg_result_fetch", "vlg_extract_batch", "never cut", "UINT64_MAX", "null stream", "max_symbols", "VLG_E_WORKSPACE", "VLG_E_UNSUPPORTED",
                 "*out untouched", "\"tuples\" = 0", "ORIGINAL", "tuple value - b", "first position"):
        assert word in block, word
    assert hasattr(V, "MatchTexts") and hasattr(V.SearchResult, "extract_matches")


def test_null_handles_are_refused_on_the_host(V):
    L = V.lib()
    out = C.c_void_p(7)
    for begin, end in ((0, U64_MAX), (0, 0), (5, 2)):
        assert L.vlg_result_extract_matches(None, None, None, None, 0, 0, begin, end, 0, C.byref(out)) == V.capi.E_INVALID
        assert out.value == 7                                                   # (nothing was written)
    assert L.vlg_result_extract_matches(None, None, None, None, U64_MAX, U64_MAX, 0, U64_MAX, 1, None) == V.capi.E_INVALID
    assert b"null" in L.vlg_last_error()
    n, sb = C.c_uint64(9), C.c_uint32(9)
    assert L.vlg_match_texts_info(None, C.byref(n), C.byref(n), C.byref(sb)) == V.capi.E_INVALID and n.value == 9 and sb.value == 9
    assert L.vlg_match_texts_fetch(None, None, None, None) == V.capi.E_INVALID
    L.vlg_match_texts_destroy(None)


def test_the_python_arguments_are_checked_before_the_library_is_asked(V):
    r = V.SearchResult.__new__(V.SearchResult)
    r._h = None
    for kw in ({"flank": -1}, {"flank": (0, -2)}, {"matches": (-1, 3)}, {"matches": (0, -3)}, {"max_symbols": -1}):
        with pytest.raises(ValueError):
            r.extract_matches(None, None, **kw)


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "match_span_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_span_rule_against_naive_loops(tmp_path):
    _build_and_run(tmp_path, "match_span_check", [])


def test_span_rule_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "match_span_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
