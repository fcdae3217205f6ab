"""The paper's index on disk, on the device: vlg_wtsa_save_sdsl / vlg_wtsa_load_sdsl / vlg_wtsa_from_parts against the files the reference
wrote (tests/golden/wtsa_sdsl, tools/wtsa_sdsl_goldens.cpp), against the format restated in tests/sdsl_wtsa.py (the rank-sample branch
too large for a fixture), round trips of both alphabets, a tree of more than 2^32 bits, the device's refusals and the C++ surface."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sdsl_wtsa as W  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "wtsa_sdsl")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
KNOWN = json.load(open(os.path.join(HERE, "golden", "vlg_known_answers.json")))


@pytest.fixture(scope="module")
def V():
    import torch
    import vlg_matching_amd as v
    assert torch.cuda.is_available()
    v.lib()
    return v


def _built(V, e):
    t = np.array(e["text"], dtype=np.uint32) if e["alphabet"] == "int" else e["text"].encode()
    return V.WtsaIndex(t)


def _levels(idx):
    return [idx.level_bits(l) for l in range(idx.info()["levels"])]


def _sa(idx):
    import torch
    n = idx.info()["n"]
    d_i = torch.arange(n, dtype=torch.int64, device="cuda")
    d_o = torch.empty_like(d_i)
    idx.sa_device(d_i.data_ptr(), d_o.data_ptr(), n)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


def _image(idx):
    """bit_vector_il<512>::m_data of the tree, on the device"""
    import torch
    info = idx.info()
    words = W.shape(info["n"], info["levels"])[3]
    d = torch.zeros(words, dtype=torch.int64, device="cuda")
    idx.il_device(d.data_ptr(), words)
    torch.cuda.synchronize()
    return d


def _same_index(a, b):
    ia, ib = a.info(), b.info()
    assert ia == ib
    for l in range(ia["levels"]):
        assert np.array_equal(a.level_bits(l), b.level_bits(l)), l
    assert np.array_equal(_sa(a), _sa(b))


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_save_gives_the_reference_bytes(V, tmp_path, name):
    e = MANIFEST[name]
    p = tmp_path / "out.sdsl"
    _built(V, e).save_sdsl(p, e["width"])
    assert p.read_bytes() == open(os.path.join(GOLDEN, name), "rb").read()
    if e["alphabet"] == "byte":
        _built(V, e).save_sdsl(p)                        # 0 = 8 for a byte index
        assert p.read_bytes() == open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_load_gives_the_built_index(V, tmp_path, name):
    e = MANIFEST[name]
    path = os.path.join(GOLDEN, name)
    idx = V.WtsaIndex.load_sdsl(path, e["alphabet"] == "int")
    built = _built(V, e)
    _same_index(idx, built)
    # load -> save: the same bytes (an int index keeps the width of its file)
    p = tmp_path / "again.sdsl"
    idx.save_sdsl(p)
    assert p.read_bytes() == open(path, "rb").read()
    if e["alphabet"] == "byte":
        cases = [c for c in KNOWN["cases"] if c["text"] == e["text"] and "error" not in c]
        for c in cases:
            assert idx.search([c["query"]]).tuples(0).tolist() == c["tuples"], c
    if name.startswith("abracadabra"):
        q = ["97 99 .{2,5}? 97 .{4,8}? 98"] if e["alphabet"] == "int" else ["ac.{2,5}?a.{4,8}?b"]
        assert idx.search(q).tuples(0).tolist() == [[3, 10, 18]]


def _rank_branch_text(kind, n, rng):
    if kind == "byte":
        return rng.choice(np.frombuffer(b"acgt", np.uint8), n), 8
    if kind == "int_wide":
        t = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        t[0] = 2 ** 32 - 1
        return t, 40                                     # symbols < 2^32 stored 40 bits wide
    return rng.integers(0, 2, n).astype(np.uint32), 1    # 1-bit symbols


@pytest.mark.parametrize("kind", ["byte", "int_wide", "int_bits"])
def test_save_equals_the_restatement_in_the_rank_sample_branch(V, tmp_path, kind):
    """The expected file is assembled from the levels of the index under test (level_bits): this pins the bit_vector_il framing, the
    count words, the rank samples and the text packing at a size no fixture reaches, NOT the tree bits themselves -- those rest on
    test_gpu_wtsa.py's comparison with the reference's own wt_int and on the reference-written fixtures above."""
    rng = np.random.default_rng({"byte": 1, "int_wide": 2, "int_bits": 3}[kind])
    n = 300000
    t, width = _rank_branch_text(kind, n, rng)
    idx = V.WtsaIndex(t)
    p = tmp_path / "big.sdsl"
    idx.save_sdsl(p, width)
    int_tag = kind != "byte"
    want = W.file_bytes(t, _levels(idx), int_tag, width)
    assert W.shape(n + 1, W.levels_of_n(n + 1))[4] == 1024
    assert p.read_bytes() == want
    back = V.WtsaIndex.load_sdsl(p, int_tag)
    _same_index(idx, back)


def _batch(text, int_tag, rng, nq=64):
    qs = []
    for _ in range(nq):
        k = int(rng.integers(1, 4))
        subs = []
        for _ in range(k):
            s = int(rng.integers(0, max(len(text) - 3, 1)))
            sub = text[s:s + int(rng.integers(1, 4))]
            subs.append(" ".join(str(int(x)) for x in sub) if int_tag else bytes(sub).decode("latin-1"))
        gaps = [".{%d,%d}?" % (a, a + int(rng.integers(0, 30))) for a in rng.integers(0, 10, k - 1)]
        if int_tag:
            q = subs[0] + "".join(" %s %s" % (g, s) for g, s in zip(gaps, subs[1:]))
        else:
            q = subs[0] + "".join(g + s for g, s in zip(gaps, subs[1:]))
        qs.append(q)
    return qs


def _results(idx, qs):
    r = idx.search(qs, max_matches=200)
    return r.summary["checksum"], r.summary["n_matches"], [r.tuples(i).tolist() for i in range(len(qs))]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 1000, 1 << 20])
@pytest.mark.parametrize("int_tag", [False, True])
def test_round_trips(V, tmp_path, n, int_tag):
    rng = np.random.default_rng(n * 2 + int_tag)
    t = rng.integers(1, 70000, n).astype(np.uint32) if int_tag else rng.choice(np.frombuffer(b"acgtn", np.uint8), n)
    idx = V.WtsaIndex(t)
    p, q = tmp_path / "a.sdsl", tmp_path / "b.sdsl"
    idx.save_sdsl(p)
    back = V.WtsaIndex.load_sdsl(p, int_tag)
    back.save_sdsl(q)
    assert p.read_bytes() == q.read_bytes()
    import torch
    assert torch.equal(_image(idx), _image(back))
    if n < 5000:
        _same_index(idx, back)
    if n:
        qs = _batch(t, int_tag, rng)
        assert _results(back, qs) == _results(idx, qs)


def test_more_than_2_32_tree_bits(V, tmp_path):
    import torch
    rng = np.random.default_rng(11)
    n = 160_000_000                                     # 28 levels: S = 4.48e9 bits
    t = rng.choice(np.frombuffer(b"acgt", np.uint8), n)
    idx = V.WtsaIndex(t)
    info = idx.info()
    assert info["n"] * info["levels"] > 2 ** 32
    p = tmp_path / "large.sdsl"
    idx.save_sdsl(p)
    back = V.WtsaIndex.load_sdsl(p)
    assert back.info() == info
    assert torch.equal(_image(idx), _image(back))
    for l in (0, info["levels"] - 1):
        assert np.array_equal(idx.level_bits(l), back.level_bits(l))
    qs = _batch(t[:100000], False, rng, nq=256)
    a, b = idx.search(qs, max_matches=100), back.search(qs, max_matches=100)
    assert a.summary["checksum"] == b.summary["checksum"] and (a.counts == b.counts).all()


def _refused(V, parts):
    """from_parts must fail with no handle"""
    from vlg_matching_amd import capi
    tw = np.ascontiguousarray(parts["text_words"], dtype=np.uint64)
    data = np.ascontiguousarray(parts["data"], dtype=np.uint64)
    rs = np.ascontiguousarray(parts["rank_samples"], dtype=np.uint64)
    P = capi.WtsaParts(parts["n"], parts["symbol_bytes"], parts["levels"], tw.ctypes.data if len(tw) else None, parts["text_count"],
                       parts["text_width"], 0, data.ctypes.data, len(data), rs.ctypes.data if len(rs) else None, len(rs))
    h = C.c_void_p(1)
    st = capi.lib().vlg_wtsa_from_parts(C.byref(P), C.byref(h))
    assert st != 0 and not h.value
    return st


def test_device_refusals(V, tmp_path):
    from vlg_matching_amd import capi
    from vlg_matching_amd.index import read_sdsl_wtsa_file
    path = os.path.join(GOLDEN, "dna_3000.sdsl")
    good = read_sdsl_wtsa_file(path)
    assert V.WtsaIndex.from_parts(good).info()["n"] == 3001
    # a cumulative count word, and the final word
    for at in (9 * 3, len(good["data"]) - 1):
        p = dict(good, data=good["data"].copy())
        p["data"][at] ^= np.uint64(1)
        assert _refused(V, p) == capi.E_INVALID, at
    # a data bit flipped: the count words catch it
    p = dict(good, data=good["data"].copy())
    p["data"][5] ^= np.uint64(1 << 13)
    assert _refused(V, p) == capi.E_INVALID
    # a tree bit flipped with the count words made to agree: the per-level count catches it
    t = list(MANIFEST["dna_3000.sdsl"]["text"].encode())
    levels = W.wt_levels(W.suffix_array(t))
    levels[3] = levels[3].copy()
    levels[3][100] ^= 1
    f = tmp_path / "flip.sdsl"
    f.write_bytes(W.file_bytes(t, levels))
    with pytest.raises(V.VlgError) as e:
        V.WtsaIndex.load_sdsl(f)
    assert e.value.status == capi.E_INVALID
    # a bit past n * L
    p = dict(good, data=good["data"].copy())
    p["data"][-2] |= np.uint64(1 << 63)
    assert _refused(V, p) == capi.E_INVALID
    # a 0 byte in a byte text
    p = dict(good, text_words=good["text_words"].copy())
    p["text_words"].view(np.uint8)[17] = 0
    assert _refused(V, p) == capi.E_ZERO_BYTE
    # an integer symbol >= 2^32
    ti = MANIFEST["abracadabrasimsalabim_int64.sdsl"]["text"]
    f.write_bytes(W.file_bytes(ti[:4] + [2 ** 33] + ti[5:], W.wt_levels(W.suffix_array(ti)), True, 64))
    with pytest.raises(V.VlgError) as e:
        V.WtsaIndex.load_sdsl(f, True)
    assert e.value.status == capi.E_UNSUPPORTED
    # save: widths that do not fit
    byte_idx = V.WtsaIndex(b"abracadabra")
    with pytest.raises(V.VlgError):
        byte_idx.save_sdsl(f, 16)
    int_idx = V.WtsaIndex(np.array([5, 300, 7], np.uint32))
    with pytest.raises(V.VlgError):
        int_idx.save_sdsl(f, 8)
    with pytest.raises(V.VlgError):
        int_idx.save_sdsl(f, 65)
    int_idx.save_sdsl(f)                                 # a built int index: the width of its largest symbol
    assert read_sdsl_wtsa_file(f, True)["text_width"] == 9


CPP = r'''
#include <cstdio>
#include <fstream>
#include <iostream>
#include "vlg_index_gpu.hpp"
using namespace vlg_host;
int main(int argc, char** argv)
{
    vlg_index_gpu<byte_alphabet_tag> built, loaded, golden;
    construct_im(built, std::string("abracadabrasimsalabim"));
    const std::string file = std::string(argv[1]) + "/idx.sdsl";
    if (!store_to_file(built, file)) return 2;
    if (!load_from_file(loaded, file)) return 3;
    if (!load_from_file(golden, argv[2])) return 4;
    vlg_index_gpu<int_alphabet_tag> wrong;
    if (load_from_file(wrong, argv[2])) return 5;                   // a byte file is not an int_alphabet_tag index
    if (load_from_file(loaded, std::string(argv[1]) + "/missing.sdsl")) return 6;
    const std::string q = "ac.{2,5}?a.{4,8}?b";
    auto it = locate(golden, q).begin();
    if (it.is_end() || it[0] != 3 || it[1] != 10 || it[2] != 18) return 7;
    std::printf("%llu %llu %llu\n", (unsigned long long)count(built, "a"), (unsigned long long)count(loaded, "a"),
                (unsigned long long)count(golden, "a"));
    return 0;
}
'''


def test_cpp_store_and_load(V, tmp_path):
    src = tmp_path / "store_load.cpp"
    src.write_text(CPP)
    exe = tmp_path / "store_load"
    lib_dir = os.path.join(ROOT, "vlg_matching_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(lib_dir, "host"), str(src),
                           "-o", str(exe), "-L" + lib_dir, "-lvlg_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe), str(tmp_path), os.path.join(GOLDEN, "abracadabrasimsalabim.sdsl")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.split() == ["7", "7", "7"]
