"""Nothing forgotten later: every prototype of include/vlg_hip.h that takes a `void* stream` or a `vlg_workspace*` has a row in the
table of tests/test_gpu_streams.py, is one of its searches, or is excluded there with a reason.  A new entry point fails this test
until it gets a row.  Needs no GPU."""
import os
import re

import test_gpu_streams as T

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlg_hip.h")


def _prototypes():
    """{name: parameter list} of every function the header declares"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = {}
    for m in re.finditer(r"\b(vlg_\w+)\s*\(([^;{}()]*)\)\s*;", src):
        out[m.group(1)] = " ".join(m.group(2).split())
    return out


def _stream_taking(protos):
    return {n for n, p in protos.items() if re.search(r"\bvoid\s*\*\s*stream\b", p) or re.search(r"\bvlg_workspace\s*\*", p)}


def test_the_parser_reads_the_header():
    protos = _prototypes()
    assert len(protos) > 100 and "vlg_last_error" in protos and "vlg_build_constants" in protos
    assert "void* stream" in protos["vlg_psi_batch"] and "vlg_workspace* ws" in protos["vlg_search_batch"]
    assert "vlg_exchange_fn" not in protos                              # (a callback type, not an entry point)


def test_every_stream_taking_entry_point_has_a_row_or_a_reason():
    taking = _stream_taking(_prototypes())
    rows = {r.entry for r in T.ROWS}
    searches, excluded = set(T.SEARCH_ENTRIES), set(T.EXCLUDED)
    assert not (rows & searches) and not (rows & excluded) and not (searches & excluded)
    covered = rows | searches | excluded
    assert taking - covered == set(), "entry points that take a stream or a workspace and have no row: %s" % sorted(taking - covered)
    assert covered - taking == set(), "rows or exclusions for what the header does not declare with a stream: %s" % sorted(covered - taking)
    for name, reason in T.EXCLUDED.items():
        assert len(reason.split()) >= 2, name
        assert name == "vlg_index_broadcast" or name.startswith("vlg_comm_") or name.startswith("vlg_workspace_"), name


def test_every_row_states_what_the_header_states():
    """a row's `sync` is the header's word: the comment in front of the prototype says "synchronises" or "asynchronous" """
    src = open(HEADER).read()
    for r in T.ROWS:
        at = src.index(" " + r.entry + "(")
        comment = src.rfind("/*", 0, at)
        # the comment block that precedes the prototype (prototypes that share one comment lie between it and the next comment)
        text = src[comment:at]
        says_sync = re.search(r"[Ss]ynchronises\s+`stream`", text) is not None
        says_async = re.search(r"[Aa]synchronous\s+on\s+`stream`", text) is not None
        assert says_sync != says_async, "%s: the header must say whether it synchronises `stream`" % r.entry
        assert says_sync == r.sync, r.entry
