"""Host parser of the paper's index on disk, vlg_index<alphabet_tag, wt_int<bit_vector_il<>, rank_support_il<>>> (vlg_sdsl_wtsa_file_*,
through vlg_matching_amd.index.read_sdsl_wtsa_file): on the files the reference wrote (tests/golden/wtsa_sdsl, tools/wtsa_sdsl_goldens.cpp),
on files tests/sdsl_wtsa.py assembles, and every refusal.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sdsl_wtsa as W  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "wtsa_sdsl")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _read(path, int_alphabet=False):
    from vlg_matching_amd.index import read_sdsl_wtsa_file
    return read_sdsl_wtsa_file(path, int_alphabet)


def _text(entry):
    return entry["text"] if entry["alphabet"] == "int" else list(entry["text"].encode())


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_parser_on_reference_files(V, name):
    e = MANIFEST[name]
    d = _read(os.path.join(GOLDEN, name), e["alphabet"] == "int")
    S, data_words, superblocks, block_num, n_rs = W.shape(e["n"], e["levels"])
    assert (d["n"], d["levels"], d["text_width"], d["text_count"]) == (e["n"], e["levels"], e["width"], e["n"] - 1)
    assert d["symbol_bytes"] == (4 if e["alphabet"] == "int" else 1)
    assert len(d["data"]) == block_num and len(d["rank_samples"]) == n_rs
    assert [int(x) for x in d["text"]] == _text(e)
    # the restatement writes the same bytes as the reference (the fixtures pin tests/sdsl_wtsa.py too)
    raw = open(os.path.join(GOLDEN, name), "rb").read()
    assert W.file_of_text(_text(e), e["alphabet"] == "int", e["width"]) == raw
    assert d["data"].tobytes() == W.il_members(W.wt_levels(W.suffix_array(_text(e))))[3].tobytes()


# texts whose trees hit the framing's corners: S = n * L a multiple of 64 (one more data word than ceil(S / 64)), a multiple of 512
# (a superblock with no data word of its own), and a level boundary inside a data word
CORNERS = {
    "s_mod_64": list(b"abcdefghijklmno"),             # n = 16, L = 4: S = 64
    "s_mod_512": list((b"banana" * 100)[:511]),       # n = 512, L = 9: S = 4608 = 9 * 512
    "inside_word": list(b"abracadabra"),              # n = 12, L = 4: levels end at bits 12, 24, 36 of word 0
}


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_parser_on_assembled_files(V, tmp_path, name):
    t = CORNERS[name]
    n, L = len(t) + 1, W.levels_of_n(len(t) + 1)
    S = n * L
    if name == "s_mod_64":
        assert S % 64 == 0
    if name == "s_mod_512":
        assert S % 512 == 0
    p = tmp_path / "f.sdsl"
    p.write_bytes(W.file_of_text(t))
    d = _read(p)
    S_, block_num, superblocks, data, rs = W.il_members(W.wt_levels(W.suffix_array(t)))
    assert d["n"] == n and d["levels"] == L and np.array_equal(d["data"], data)
    assert bytes(d["text"].tobytes()) == bytes(t)
    # the same text as ints, widths 1..64 where it fits (int_alphabet_tag)
    for w in (7, 8, 33, 64):
        p.write_bytes(W.file_of_text(t, True, w))
        d = _read(p, True)
        assert d["text_width"] == w and [int(x) for x in d["text"]] == t


def _refuse(tmp_path, raw, int_alphabet=False):
    from vlg_matching_amd.capi import VlgError
    p = tmp_path / "bad.sdsl"
    p.write_bytes(raw)
    with pytest.raises(VlgError) as e:
        _read(p, int_alphabet)
    return e.value.status


TEXT = list(b"abracadabrasimsalabim")


def test_refusals(V, tmp_path):
    from vlg_matching_amd.capi import E_INVALID
    good = W.file_of_text(TEXT)
    assert _read_bytes(tmp_path, good)["n"] == len(TEXT) + 1
    n = len(TEXT) + 1
    S, data_words, superblocks, block_num, _ = W.shape(n, W.levels_of_n(n))
    cases = {
        "truncated": good[:-1],
        "truncated in the data": good[:60],
        "trailing bytes": good + b"\0",
        "wt size != text size + 1": W.file_of_text(TEXT, size=n + 1),
        "sigma != size": W.file_of_text(TEXT, sigma=n - 1),
        "wrong max_level": W.file_of_text(TEXT, max_level=6),
        "block_shift != 9": W.file_of_text(TEXT, block_shift=8),
        "wrong block_num": W.file_of_text(TEXT, block_num=block_num + 1),
        "wrong superblocks": W.file_of_text(TEXT, superblocks=superblocks + 1),
        "wrong il size": W.file_of_text(TEXT, il_size=S - 1),
        "wrong data length": W.file_of_text(TEXT, data=np.zeros(block_num + 1, np.uint64)),
        "wrong rank-sample count": W.file_of_text(TEXT, rank_samples=np.zeros(1, np.uint64)),
        "empty file": b"",
    }
    for what, raw in cases.items():
        assert _refuse(tmp_path, raw) == E_INVALID, what
    # the text of another size than the tree
    assert _refuse(tmp_path, W.file_bytes(TEXT[:-1], W.wt_levels(W.suffix_array(TEXT)))) == E_INVALID


def test_refusals_int_width(V, tmp_path):
    from vlg_matching_amd.capi import E_INVALID
    good = W.file_of_text(TEXT, True, 8)
    assert _read_bytes(tmp_path, good, True)["text_width"] == 8
    for w in (0, 65, 255):
        raw = bytearray(good)
        raw[8] = w                                      # the width byte of int_vector<0>
        assert _refuse(tmp_path, bytes(raw), True) == E_INVALID, w


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_the_other_alphabet_tag_is_refused(V, tmp_path, name):
    from vlg_matching_amd.capi import E_INVALID
    e = MANIFEST[name]
    raw = open(os.path.join(GOLDEN, name), "rb").read()
    assert _refuse(tmp_path, raw, e["alphabet"] != "int") == E_INVALID


def test_rank_sample_branch(V, tmp_path):
    """m_block_num > 65536: 1024 rank samples in init_rank_samples' order; a wrong one is refused"""
    from vlg_matching_amd.capi import E_INVALID
    rng = np.random.default_rng(5)
    n = 300001
    L = W.levels_of_n(n)
    levels = [rng.integers(0, 2, n).astype(np.uint8) for _ in range(L)]     # the parser does not look at what the bits mean
    t = list(rng.integers(1, 256, n - 1))
    raw = W.file_bytes(t, levels)
    d = _read_bytes(tmp_path, raw)
    S, block_num, superblocks, data, rs = W.il_members(levels)
    assert len(rs) == 1024 and np.array_equal(d["rank_samples"], rs) and np.array_equal(d["data"], data)
    bad = rs.copy()
    bad[7] += 1
    assert _refuse(tmp_path, W.file_bytes(t, levels, rank_samples=bad)) == E_INVALID
    assert _refuse(tmp_path, W.file_bytes(t, levels, rank_samples=rs[:512])) == E_INVALID


def test_null_and_bad_arguments(V):
    import ctypes as C
    from vlg_matching_amd.capi import E_INVALID, lib
    f = C.c_void_p()
    assert lib().vlg_sdsl_wtsa_file_open(os.path.join(GOLDEN, "a.sdsl").encode(), 2, C.byref(f)) == E_INVALID
    assert lib().vlg_sdsl_wtsa_file_open(b"/nonexistent/x.sdsl", 1, C.byref(f)) == E_INVALID
    assert lib().vlg_sdsl_wtsa_file_open(None, 1, C.byref(f)) == E_INVALID


def test_paths_that_are_not_files(V, tmp_path):
    """a directory (fopen may succeed on one, with a size of LLONG_MAX) or a missing file: a status, never an exception"""
    import ctypes as C
    from vlg_matching_amd.capi import E_INVALID, lib
    f = C.c_void_p()
    for path in (HERE, str(tmp_path), str(tmp_path / "missing.sdsl")):
        for tag in (1, 4):
            assert lib().vlg_sdsl_wtsa_file_open(path.encode(), tag, C.byref(f)) == E_INVALID, (path, tag)
            assert not f.value
    h = C.c_void_p()
    assert lib().vlg_wtsa_load_sdsl(HERE.encode(), 1, C.byref(h)) == E_INVALID and not h.value


def _read_bytes(tmp_path, raw, int_alphabet=False):
    p = tmp_path / "ok.sdsl"
    p.write_bytes(raw)
    return _read(p, int_alphabet)


def test_header_sizes_follow_the_formulas():
    # bit_vector_il<512> sizes of the fixtures, restated: n = 1 (the empty text) is one level of one bit
    assert W.shape(1, 1) == (1, 1, 1, 3, 0)
    assert W.shape(16, 4)[1] == 2                       # S = 64: (S + 64) / 64 data words
    assert W.shape(512, 9)[2] == 10                     # S = 4608: (S + 512) / 512 superblocks, the last without data words
