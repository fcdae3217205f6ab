"""Integer-alphabet indexes on disk: csa_wt<wt_int<>, d, isa_d, sa_order_sa_sampling<>, isa_sampling<>, int_alphabet<>> files
(test/csa_int_test.cpp:29-33) written by vlg_index_save_sdsl[_int] and read by vlg_index_load_sdsl_int, the reference's level-wise
wt_int<> tree converted to and from the device's wavelet matrix on the GPU.  The file is checked member by member against the
reference's own wt_int<> / rank_support_v / int_alphabet (oracle/_ref, where built) and against the CPU oracle's restatement of them;
a file assembled in Python from reference-built members must load into the blob vlg_index_build_int makes of the same text."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdsl_int as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _texts():
    rng = np.random.default_rng(31)
    big = rng.integers(1, 2 ** 32 - 1, 80000, dtype=np.uint64).astype(np.uint32)
    big = np.unique(big)[:80000]
    return {
        "survey": np.array([5, 6, 7, 5, 6, 7, 1000, 5], dtype=np.uint32),
        "abra": np.frombuffer(b"abracadabrasimsalabim", dtype=np.uint8).astype(np.uint32),
        "sparse": rng.choice(np.array([3, 7, 7, 19, 1000, 70000, 2 ** 31 + 5], dtype=np.uint32), 5000),    # 32 original levels
        "words": (1 + rng.zipf(1.3, 20000) % 3000).astype(np.uint32),
        "one": np.array([42], dtype=np.uint32),
        "run": np.full(300, 9, dtype=np.uint32),
        "keeper": np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keeper.int"), dtype="<u8").astype(np.uint32),
        "wide_sigma": rng.permutation(np.concatenate([big, rng.choice(big, 150000 - len(big))])).astype(np.uint32),
        "continuous": rng.permutation(np.concatenate([np.arange(1, 201), rng.integers(1, 201, 800)])).astype(np.uint32),   # m_char empty
        "empty": np.zeros(0, dtype=np.uint32),
    }


TEXTS = _texts()
NAMES = list(TEXTS)
_CACHE = {}


def _case(oracle, name, dens):
    """(oracle index, suffix array) of one text"""
    key = (name, dens)
    if key not in _CACHE:
        text = TEXTS[name]
        o = oracle.IntIndex(text.astype(np.uint64), dens=dens)
        o1 = oracle.IntIndex(text.astype(np.uint64), dens=1)
        sa = np.array([o1.sa(i) for i in range(o1.n)], dtype=np.int64)
        _CACHE[key] = (o, sa)
    return _CACHE[key]


def _queries(text, n):
    rng = np.random.default_rng(17)
    t = text.tolist()
    qs = []
    for _ in range(n):
        a, b = (int(x) for x in rng.integers(0, len(t), 2))
        g = int(rng.integers(0, 20))
        qs.append("%d .{%d,%d}? %d" % (t[a], g, g + 30, t[b]))
    return qs + ["%d" % t[0], "%d .{0,5}? 999999" % t[-1]]


def _blob(torch, idx):
    nb = idx.blob_bytes()
    buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    idx.blob_export(buf.data_ptr(), nb)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _fetch(idx, qs):
    """counts, offsets, first positions and tuples of the batch"""
    return [a.tolist() for a in idx.search(qs).fetch()]


@pytest.mark.parametrize("name", NAMES)
def test_writer_against_reference_built_members(torch_cuda, V, oracle, tmp_path, name):
    refmod = oracle if oracle.ref() is not None else None
    text = TEXTS[name]
    for dens in (32, 5):
        o, sa = _case(oracle, name, dens)
        n = o.n
        bwt = o.bwt()
        idx = V.VlgIndex.build_int(text, dens=dens)
        for isa_dens in (64, 32):
            path = tmp_path / ("%s_%d_%d.sdsl" % (name, dens, isa_dens))
            idx.save_sdsl(path, isa_dens=isa_dens)
            f = S.read_file(path)
            assert f["unread"] == 0
            L = f["max_level"]
            assert L == S.levels_of(int(bwt.max())) and f["size"] == n and f["tree_bits"] == n * L
            tree = S.words_to_bits(f["tree_words"], n * L).reshape(L, n)
            assert (tree == o.level_bits()).all() and L == o.levels
            assert f["sigma"] == o.sigma == f["m_sigma"]
            assert f["C"] == o.C().tolist() and f["comp2char"] == o.comp2char().tolist() and f["C_width"] == S.hi(n) + 1
            assert f["rank_blocks"] == S.rank_v_blocks(tree.reshape(-1))
            flat = tree.reshape(-1)
            for b, sel in ((1, f["sel1"]), (0, f["sel0"])):
                pos = np.flatnonzero(flat == b)
                assert sel["cnt"] == len(pos)
                for i in range(1, len(pos) + 1, 64 * 7 + 1 if len(pos) > 5000 else 1):
                    if sel["blocks"][(i - 1) // 4096][0] == "long" or (i - 1) % 64 == 0:
                        assert S.select_at(sel, i) == pos[i - 1], (b, i)
            sd = f["m_char"]
            if int(o.comp2char()[-1]) + 1 == o.sigma:                      # continuous ("continuous", "keeper"): no m_char
                assert sd["size"] == 0
            else:
                assert sd["size"] == int(o.comp2char()[-1]) + 1 and sd["low_width"] == sd["wl"]
            assert f["sa_width"] == S.hi(n) + 1 and f["samples"] == sa[::dens].tolist() == o.samples().tolist()
            assert f["isa_width"] == S.hi(n) + 1 and len(f["isa"]) == (n - 1) // isa_dens + 1
            assert all(sa[f["isa"][j]] == isa_dens * j for j in range(len(f["isa"])))
            if refmod is not None:
                ref = refmod.RefWtIntPlain(bwt)
                assert (ref.level_bits() == tree).all() and ref.sigma == f["sigma"] and ref.levels == L
                assert f["rank_blocks"] == refmod.ref_rank_v_blocks(f["tree_words"], n * L).tolist()
                Cc, c2c = refmod.ref_int_alphabet(bwt)
                assert f["C"] == Cc.tolist() and f["comp2char"] == c2c.tolist()
        assert name != "continuous" or f["m_char"]["size"] == 0
        # an rrr source writes the same file as its plain twin
        rp = tmp_path / ("%s_%d_rrr.sdsl" % (name, dens))
        idx.compress().save_sdsl(rp)
        assert rp.read_bytes() == (tmp_path / ("%s_%d_64.sdsl" % (name, dens))).read_bytes()


def _assembled(oracle, name, path, dens=32, rrr=False):
    """a file assembled from reference-built members (the oracle's twins where oracle/_ref is missing)"""
    o, sa = _case(oracle, name, dens)
    n, bwt = o.n, o.bwt()
    if oracle.ref() is not None:
        ref = oracle.RefWtIntPlain(bwt)
        tree = ref.level_bits()
        Cc, c2c = oracle.ref_int_alphabet(bwt)
        words = S.bits_to_words(tree.reshape(-1))
        rb = oracle.ref_rank_v_blocks(words, n * ref.levels)
    else:
        tree, Cc, c2c, rb = o.level_bits(), o.C(), o.comp2char(), None
    isa = [0] * ((n - 1) // 64 + 1)
    for i, v in enumerate(sa.tolist()):
        if v % 64 == 0:
            isa[v // 64] = i
    S.write_file(path, n, tree, Cc.tolist(), c2c.tolist(), sa[::dens].tolist(), isa, rank_blocks=rb, rrr=rrr)
    return o


@pytest.mark.parametrize("name", NAMES)
def test_loader_on_a_reference_shaped_file(torch_cuda, V, oracle, tmp_path, name):
    torch = torch_cuda
    text = TEXTS[name]
    path = tmp_path / (name + ".sdsl")
    o = _assembled(oracle, name, path)
    idx = V.VlgIndex.load_sdsl_int(path)
    built = V.VlgIndex.build_int(text)
    assert (_blob(torch, idx) == _blob(torch, built)).all()
    Cc, c2c = idx.int_alphabet()
    assert Cc.tolist() == o.C().tolist() and c2c.tolist() == o.comp2char().tolist()
    rng = np.random.default_rng(5)
    pos = rng.integers(0, o.n + 1, 300).astype(np.uint64)
    syms = np.array([int(s) for s in rng.choice(o.comp2char(), 300)], dtype=np.uint32)
    d_i = torch.from_numpy(pos.view(np.int64)).cuda()
    d_s = torch.from_numpy(syms.view(np.int32)).cuda()
    d_o = torch.zeros_like(d_i)
    V.capi.check(V.lib().vlg_int_rank_batch(idx._h, d_i.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), len(pos), None))
    torch.cuda.synchronize()
    got = d_o.cpu().numpy().view(np.uint64).tolist()
    assert got == [o.rank(int(p), int(s)) for p, s in zip(pos, syms)]
    if len(text):
        qs = _queries(text, 40)
        res = idx.search(qs)
        for i, q in enumerate(qs):
            assert res.tuples(i).tolist() == o.search(q).tolist(), q
        plain = _fetch(idx, qs)
        rp = tmp_path / (name + "_rrr.sdsl")
        _assembled(oracle, name, rp, rrr=True)
        ridx = V.VlgIndex.load_sdsl_int(rp, rrr=True)
        assert ridx.info()["bv_kind"] == 3                                  # VLG_BV_INT_MATRIX_RRR63
        assert _fetch(ridx, qs) == plain


@pytest.mark.parametrize("name", NAMES)
def test_round_trip(torch_cuda, V, tmp_path, name):
    torch = torch_cuda
    text = TEXTS[name]
    for dens in (32, 7):
        idx = V.VlgIndex.build_int(text, dens=dens)
        path = tmp_path / ("%s_%d.sdsl" % (name, dens))
        idx.save_sdsl(path)
        back = V.VlgIndex.load_sdsl_int(path, dens=dens)
        assert (_blob(torch, back) == _blob(torch, idx)).all()
        if len(text):
            qs = _queries(text, 30)
            assert _fetch(back, qs) == _fetch(idx, qs)


def test_refusals(torch_cuda, V, oracle, tmp_path):
    text = TEXTS["words"]
    idx = V.VlgIndex.build_int(text)
    good = tmp_path / "good.sdsl"
    idx.save_sdsl(good)
    data = good.read_bytes()

    def load_ok():
        h = C.c_void_p()
        assert V.lib().vlg_index_load_sdsl_int(str(good).encode(), 32, 0, C.byref(h)) == 0
        V.lib().vlg_index_destroy(h)

    # a text-order index is not stored (resample it to SA order first)
    to = idx.resample(text_order=True, dens=32)
    st = V.lib().vlg_index_save_sdsl(to._h, str(tmp_path / "to.sdsl").encode())
    assert st == V.capi.E_UNSUPPORTED and b"SA order" in V.lib().vlg_last_error()
    load_ok()
    # a byte index through save_sdsl_int
    bidx = V.VlgIndex.build(b"abracadabra")
    assert V.lib().vlg_index_save_sdsl_int(bidx._h, str(tmp_path / "b.sdsl").encode(), 64) == V.capi.E_INVALID
    load_ok()
    bidx.save_sdsl(tmp_path / "byte.sdsl")
    bad = tmp_path / "bad.sdsl"
    cases = [("byte file", (tmp_path / "byte.sdsl").read_bytes(), 32), ("truncated", data[:-5], 32), ("trailing byte", data + b"\0", 32),
             ("wrong dens", data, 16)]
    oi = oracle.IntIndex(TEXTS["survey"].astype(np.uint64), dens=32)
    c2c = oi.comp2char().tolist()
    c2c[-1] = 2 ** 32 + 7
    L = S.levels_of(c2c[-1])
    tree = np.concatenate([np.zeros((L - oi.levels, oi.n), np.uint8), oi.level_bits()])
    big = S.write_file(tmp_path / "big.sdsl", oi.n, tree, oi.C().tolist(), c2c, oi.samples().tolist(), [0])
    cases.append(("symbol >= 2^32", big, 32))
    for what, blob, dens in cases:
        bad.write_bytes(blob)
        h = C.c_void_p()
        st = V.lib().vlg_index_load_sdsl_int(str(bad).encode(), dens, 0, C.byref(h))
        assert st != 0 and not h.value, what
        if what == "symbol >= 2^32":
            assert st == V.capi.E_UNSUPPORTED
        load_ok()
    # a tree that disagrees with C is refused on the device, not decoded into garbage
    oi2, sa2 = _case(oracle, "words", 32)
    tree2 = oi2.level_bits().copy()
    tree2[3, 0] ^= 1                                                           # one node now holds one 1 too many or too few
    S.write_file(bad, oi2.n, tree2, oi2.C().tolist(), oi2.comp2char().tolist(), sa2[::32].tolist(), [0] * ((oi2.n - 1) // 64 + 1))
    h = C.c_void_p()
    assert V.lib().vlg_index_load_sdsl_int(str(bad).encode(), 32, 0, C.byref(h)) == V.capi.E_INVALID and not h.value
    load_ok()


def test_moderate_round_trip(torch_cuda, V, tmp_path):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    ranks = np.arange(1, 50001, dtype=np.float64)
    p = (1.0 / ranks) / (1.0 / ranks).sum()
    text = (rng.choice(50000, 1 << 20, p=p) + 1).astype(np.uint32)
    idx = V.VlgIndex.build_int(text)
    path = tmp_path / "m.sdsl"
    t0 = time.perf_counter()
    idx.save_sdsl(path)
    t1 = time.perf_counter()
    back = V.VlgIndex.load_sdsl_int(path)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert (_blob(torch, back) == _blob(torch, idx)).all()
    qs = _queries(text, 200)
    assert _fetch(back, qs) == _fetch(idx, qs)
    print("2^20 tokens: save %.3f s, load %.3f s, file %d bytes" % (t1 - t0, t2 - t1, os.path.getsize(path)))
