"""Host parser of csa_wt<wt_int<>, d, ., sa_order_sa_sampling<>, isa_sampling<>, int_alphabet<>> files (vlg_sdsl_int_file_*, through
vlg_matching_amd.index.read_sdsl_int_file) on files this test assembles member by member (tests/sdsl_int.py): continuous and sparse
alphabets, a wt_int<rrr_vector<63>> tree, and every refusal.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdsl_int as S  # noqa: E402


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def naive(text):
    tz = [int(x) for x in text] + [0]
    n = len(tz)
    sa = sorted(range(n), key=lambda i: tz[i:])
    bwt = [tz[i - 1] if i else 0 for i in sa]
    return n, sa, bwt


TEXTS = {
    "continuous": np.random.default_rng(1).permutation(np.repeat(np.arange(1, 201), 3)),      # every symbol 1..200: m_char is empty
    "sparse": np.random.default_rng(2).choice([3, 7, 7, 19, 1000, 70000, 2 ** 31 + 5], 700),     # 32 levels
    "survey": [5, 6, 7, 5, 6, 7, 1000, 5],
    "one": [42],
    "empty": [],
}


def _file(tmp_path, name, dens=32, isa_dens=64, rrr=False, **over):
    n, sa, bwt = naive(TEXTS[name])
    m = S.members(n, bwt, sa, dens, isa_dens)
    args = dict(n=n, tree_bits_2d=m["tree"], C=m["C"], comp2char=m["comp2char"], samples=m["samples"], isa=m["isa"], rrr=rrr)
    args.update(over)
    path = tmp_path / ("%s_%d%s.sdsl" % (name, dens, "_rrr" if rrr else ""))
    data = S.write_file(path, **args)
    return path, data, n, sa, m


@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("rrr", [False, True])
def test_parser_reads_assembled_files(V, tmp_path, name, rrr):
    for dens in (32, 3):
        path, _, n, sa, m = _file(tmp_path, name, dens=dens, rrr=rrr)
        got = V.index.read_sdsl_int_file(path, dens=dens, rrr=rrr)
        assert got["n"] == n and got["sigma"] == len(m["comp2char"]) and got["max_level"] == m["levels"] and got["dens"] == dens
        assert got["comp2char"].tolist() == list(m["comp2char"]) and got["C"].tolist() == list(m["C"])
        assert got["tree_bits"] == n * m["levels"]
        assert (S.words_to_bits(got["tree_words"], got["tree_bits"]) == m["tree"].reshape(-1)).all()
        assert got["samples"].tolist() == [sa[j] for j in range(0, n, dens)]
    if name == "continuous" and not rrr:
        assert S.read_file(path)["m_char"]["size"] == 0
    if name == "sparse":
        assert m["levels"] == 32


def _status(V, path, dens=32, rrr=False):
    f = C.c_void_p()
    st = V.lib().vlg_sdsl_int_file_open(str(path).encode(), dens, 1 if rrr else 0, C.byref(f))
    if st == 0:
        V.lib().vlg_sdsl_int_file_close(f)
    return st, (V.lib().vlg_last_error() or b"").decode()


def test_refusals(V, tmp_path):
    E_INVALID, E_UNSUPPORTED = V.capi.E_INVALID, V.capi.E_UNSUPPORTED
    path, data, n, sa, m = _file(tmp_path, "sparse")
    assert _status(V, path)[0] == 0
    bad = tmp_path / "bad.sdsl"

    def check(blob, want=E_INVALID, dens=32, rrr=False, text=None):
        bad.write_bytes(blob)
        st, msg = _status(V, bad, dens, rrr)
        assert st == want, (st, msg)
        if text:
            assert text in msg, msg
        assert _status(V, path)[0] == 0                                # a normal parse still succeeds afterwards

    for cut in (0, 7, 16, 40, len(data) // 2, len(data) - 9, len(data) - 1):
        check(data[:cut])
    check(data + b"\0", text="trailing")
    bad.write_bytes(data)
    assert _status(V, bad, dens=16)[0] == E_INVALID                       # ceil(n / 16) samples != ceil(n / 32)
    assert "density" in _status(V, bad, dens=16)[1]
    # sample count other than ceil(n / d)
    check(S.write_file(bad, n, m["tree"], m["C"], m["comp2char"], m["samples"][:-1], m["isa"]), text="density")
    # wt.size != C[sigma]
    C2 = list(m["C"])
    C2[-1] += 1
    check(S.write_file(bad, n, m["tree"], C2, m["comp2char"], m["samples"], m["isa"]))
    # C not increasing
    C3 = list(m["C"])
    C3[2] = C3[1]
    check(S.write_file(bad, n, m["tree"], C3, m["comp2char"], m["samples"], m["isa"]), text="increase")
    # max_level inconsistent with the largest symbol
    check(S.write_file(bad, n, m["tree"], m["C"], m["comp2char"], m["samples"], m["isa"], max_level=31), text="max_level")
    # an ISA vector whose length fits no density
    check(S.write_file(bad, n, m["tree"], m["C"], m["comp2char"], m["samples"], [0] * (n + 1)), text="ISA")
    # a symbol >= 2^32
    c2c = list(m["comp2char"])
    c2c[-1] = 2 ** 33 + 1
    tree = np.concatenate([np.zeros((2, n), np.uint8), m["tree"]])
    bad.write_bytes(b"")
    blob = S.write_file(bad, n, tree, m["C"], c2c, m["samples"], m["isa"])
    check(blob, want=E_UNSUPPORTED, text="2^32")
    # not an integer-index file at all, and the rrr reader on a plain file
    check(b"not an index at all" * 10)
    check(data, rrr=True)


def test_parser_refuses_a_byte_index_file(V, refmod, tmp_path):
    """a csa_wt<wt_huff<>> file written by the reference's own code is not read as an integer index"""
    from util import bwt_from_sa
    text = b"abracadabrasimsalabim"
    tz = np.frombuffer(text + b"\0", dtype=np.uint8)
    sa = refmod.suffix_array(tz)
    R = refmod.RefIndex(bwt_from_sa(tz, sa), sa, 0)
    path = tmp_path / "byte.sdsl"
    R.write_csa_image(path, sa)
    assert V.index.read_sdsl_file(path)["n"] == len(tz)
    assert _status(V, path)[0] != 0
