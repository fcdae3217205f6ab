"""Documents (vlg_documents, vlg_queries_set_documents) without a device: the argument checks of vlg_documents_create come before a
device is asked for (a bad argument is VLG_E_INVALID on a machine without a GPU too, a good one fails loudly there with
VLG_E_NO_DEVICE), NULL handles are refused on the host, header, library and binding stay in step, and the boundary arithmetic of
csrc/doc_cut.hpp -- nb, the straddle test, the capped window, the capped restart -- agrees with naive loops in a stand-alone program,
also under ASan + UBSan.  What needs a batch (set / get, windows against documents) needs a device to make one: tests/test_gpu_documents.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as V
    return V


def _create(V, starts, n_docs, n_text):
    h = C.c_void_p(0xDEAD)
    a = np.ascontiguousarray(starts, dtype=np.uint64) if starts is not None else None
    st = V.lib().vlg_documents_create(a.ctypes.data if a is not None else None, n_docs, n_text, C.byref(h))
    return st, h


@pytest.mark.parametrize("starts,n_docs,n_text,word", [
    (None, 1, 10, b"null"),                     # NULL starts
    ([0], 0, 10, b"at least one"),              # no document
    ([1, 5], 2, 10, b"starts at 0"),            # the first start is not 0
    ([0, 5, 5], 3, 10, b"start 2"),             # not strictly ascending
    ([0, 5, 4], 3, 10, b"start 2"),
    ([0, 10], 2, 10, b"start 1"),               # a start at n_text
    ([0, 11], 2, 10, b"start 1"),
    ([0], 1, 0, b"start 0"),                    # an empty text has no document
])
def test_create_checks_its_arguments_before_it_asks_for_a_device(V, starts, n_docs, n_text, word):
    st, h = _create(V, starts, n_docs, n_text)
    assert st == V.capi.E_INVALID
    assert h.value is None                                                  # *out = NULL
    assert word in V.lib().vlg_last_error(), V.lib().vlg_last_error()
    assert V.lib().vlg_documents_create(None, 1, 10, None) == V.capi.E_INVALID


def test_create_fails_loudly_without_a_device(V):
    n = C.c_int(0)
    have = V.lib().vlg_device_count(C.byref(n)) == V.capi.OK and n.value > 0
    st, h = _create(V, [0, 4, 9], 3, 10)
    if have:
        assert st == V.capi.OK and h.value
        assert V.lib().vlg_documents_count(h) == 3 and V.lib().vlg_documents_text_length(h) == 10
        V.lib().vlg_documents_destroy(h)
    else:
        assert st == V.capi.E_NO_DEVICE and h.value is None
        assert b"device" in V.lib().vlg_last_error()
        with pytest.raises(V.VlgError):
            V.Documents.from_starts([0, 4, 9], 10)
    # the Python class refuses what the library refuses, and a few things on its own
    with pytest.raises(V.VlgError):
        V.Documents.from_starts([0, 5, 5], 10)
    with pytest.raises(ValueError):
        V.Documents.from_starts([0, -1], 10)
    with pytest.raises(ValueError):
        V.Documents.from_starts([[0, 1]], 10)


def test_null_handles_are_refused_on_the_host(V):
    L = V.lib()
    out = C.c_void_p(7)
    assert L.vlg_queries_set_documents(None, None) == V.capi.E_INVALID
    assert L.vlg_queries_get_documents(None, C.byref(out)) == V.capi.E_INVALID
    assert out.value == 7                                                   # (nothing was written)
    assert L.vlg_documents_locate_batch(None, None, 0, None, None) == V.capi.E_INVALID
    assert b"null" in L.vlg_last_error()
    assert L.vlg_documents_count(None) == 0 and L.vlg_documents_text_length(None) == 0
    L.vlg_documents_destroy(None)


def test_header_library_and_binding_stay_in_step(V):
    src = open(os.path.join(ROOT, "include", "vlg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(V.library_path())
    bound = {s[0]: s for s in V.capi.SYMBOLS}
    for name, nargs in (("vlg_documents_create", 4), ("vlg_documents_destroy", 1), ("vlg_documents_count", 1), ("vlg_documents_text_length", 1),
                        ("vlg_documents_locate_batch", 5), ("vlg_queries_set_documents", 2), ("vlg_queries_get_documents", 2)):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(L, name), "library does not export " + name
        assert name in bound and len(bound[name][2]) == nargs
    # the contract is written down where a caller looks for it
    for word in ("doc(v) == doc(v + m - 1)", "bit-identical", "fuse_jump", "VLG_E_UNSUPPORTED", "vlg_join_batch"):
        assert word in src[src.index("Documents: the indexed text"):src.index("typedef struct vlg_documents")]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + extra + ["-I", os.path.join(ROOT, "vlg_matching_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "doc_cut_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")


def test_boundary_arithmetic_against_naive_loops(tmp_path):
    _build_and_run(tmp_path, "doc_cut_check", [])


def test_boundary_arithmetic_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    _build_and_run(tmp_path, "doc_cut_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
