"""Select on the device (vlg_select_support): select_support_mcl<1> / <0> and select_support_rrr on bit-vectors
(include/sdsl/select_support_mcl.hpp:347, rrr_vector.hpp:638), wt_pc::select / wt_int::select on the BWT (wt_pc.hpp:415-442,
wt_int.hpp:442), csa.psi / csa.lf / csa.bwt (suffix_array_helper.hpp:322-349, 425-429), for byte and integer indexes, plain and rrr,
SA-order and text-order sampled, built, loaded and attached.  The truth is the definition, computed from the text:
isa = inverse of sa, lf[i] = isa[(sa[i] - 1) mod n], psi[i] = isa[(sa[i] + 1) mod n], select(k, c) = flatnonzero(bwt == c)[k - 1]."""
import numpy as np
import pytest

from util import bwt_from_sa, dna_text, naive_sa, skewed_text

pytestmark = pytest.mark.gpu

NONE = np.uint64(2 ** 64 - 1)


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


def dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- bit-vectors -------------------------------------------------------------------------------------------------------------------------
def pack_bits(bits):
    b = np.zeros((len(bits) + 63) // 64 * 64, np.uint8)
    b[: len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64) if len(b) else np.zeros(0, np.uint64)


def bit_cases(nbits):
    rng = np.random.default_rng(nbits)
    out = {"zeros": np.zeros(nbits, np.uint8), "ones": np.ones(nbits, np.uint8), "half": (rng.random(nbits) < 0.5).astype(np.uint8),
           "sparse": (rng.random(nbits) < 0.03).astype(np.uint8), "first": np.zeros(nbits, np.uint8), "last": np.zeros(nbits, np.uint8)}
    out["first"][0] = 1
    out["last"][-1] = 1
    return out


def check_bit_select(ss, bits, ks=None):
    """every k in 0 .. count + 1 (or the given ones) for both bit values, against flatnonzero"""
    nbits = len(bits)
    for bit in (1, 0):
        pos = np.flatnonzero(bits == bit).astype(np.uint64)
        k = np.arange(len(pos) + 2, dtype=np.uint64) if ks is None else ks[bit]
        want = np.full(len(k), nbits, np.uint64)
        ok = (k >= 1) & (k <= len(pos))
        want[ok] = pos[k[ok].astype(np.int64) - 1]
        got = ss.bit_select(k, bit)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (bit, nbits, int(k[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


BIT_SIZES = [1, 223, 224, 225, 447, 448, 449, 2015, 2016, 2017, 64 * 224 - 1, 64 * 224 + 1, 10 ** 5]


@pytest.mark.parametrize("kind", ["plain", "rrr"])
def test_bit_select_every_k(torch_cuda, V, kind):
    make = V.BitVector if kind == "plain" else V.RrrBitVector
    for nbits in BIT_SIZES:
        for name, bits in bit_cases(nbits).items():
            bv = make(pack_bits(bits), nbits)
            for sample in (64, 0):
                ss = bv.select_support(sample)
                assert ss.hbm_bytes() > 0
                check_bit_select(ss, bits)
                assert ss.bit_select(1, 1) == (int(np.flatnonzero(bits)[0]) if bits.any() else nbits), (name, nbits)


@pytest.mark.parametrize("kind", ["plain", "rrr"])
def test_bit_select_sparse_vector_bounded_search(torch_cuda, V, kind):
    """2^24 bits with ones only at the two ends and 200 isolated ones between: neighbouring zero hints lie next to each other, neighbouring
    one hints up to 10^4 super-blocks apart"""
    nbits = 1 << 24
    rng = np.random.default_rng(24)
    bits = np.zeros(nbits, np.uint8)
    bits[:1000] = rng.random(1000) < 0.7
    bits[-1000:] = rng.random(1000) < 0.7
    bits[0] = bits[-1] = 1
    bits[rng.choice(np.arange(2000, nbits - 2000), 200, replace=False)] = 1
    bv = (V.BitVector if kind == "plain" else V.RrrBitVector)(pack_bits(bits), nbits)
    ss = bv.select_support(64)
    ones = np.flatnonzero(bits)
    n0 = nbits - len(ones)
    zero_rank = (ones - np.arange(len(ones))).astype(np.int64)          # zeros in front of every one
    near = np.concatenate([zero_rank - 1, zero_rank, zero_rank + 1, zero_rank + 2])
    k0 = np.unique(np.concatenate([near[(near >= 0) & (near <= n0 + 1)], rng.integers(0, n0 + 2, 10 ** 4), [0, 1, n0, n0 + 1]])).astype(np.uint64)
    check_bit_select(ss, bits, {1: np.arange(len(ones) + 2, dtype=np.uint64), 0: k0})


# ---- indexes -----------------------------------------------------------------------------------------------------------------------------
def suffix_array_doubling(t):
    """suffix array of an integer text that ends in its unique smallest symbol: prefix doubling on numpy sorts"""
    n = len(t)
    rank = np.unique(t, return_inverse=True)[1].astype(np.int64).reshape(-1)
    k = 1
    while True:
        second = np.full(n, -1, np.int64)
        second[: n - k] = rank[k:]
        sa = np.lexsort((second, rank))
        change = (rank[sa][1:] != rank[sa][:-1]) | (second[sa][1:] != second[sa][:-1])
        rank = np.zeros(n, np.int64)
        rank[sa] = np.concatenate([[0], np.cumsum(change)])
        if rank[sa[-1]] == n - 1:
            return sa.astype(np.int64)
        k *= 2


class Truth:
    """sa, isa, lf, psi, bwt of a text with its sentinel, and the select queries that cover every occurrence and every refusal"""

    def __init__(self, full, sa):
        n = len(full)
        self.n, self.full = n, full
        self.sa = np.asarray(sa, np.int64)
        self.isa = np.zeros(n, np.uint64)
        self.isa[self.sa] = np.arange(n, dtype=np.uint64)
        self.lf = self.isa[(self.sa - 1) % n]
        self.psi = self.isa[(self.sa + 1) % n]
        self.bwt = full[(self.sa - 1) % n]

    def select_queries(self, absent):
        """(k, c, want): every k in 0 .. count + 1 of every symbol that occurs, and k in 0 .. 2 of the absent ones"""
        n = self.n
        order = np.argsort(self.bwt, kind="stable")
        syms, start, cnt = np.unique(self.bwt[order], return_index=True, return_counts=True)
        k_in = np.arange(n) - np.repeat(start, cnt) + 1
        absent = np.asarray(absent, dtype=np.uint64)
        k = np.concatenate([k_in, np.zeros(len(syms)), cnt + 1, np.tile([0, 1, 2], len(absent))]).astype(np.uint64)
        c = np.concatenate([self.bwt[order], syms, syms, np.repeat(absent, 3)]).astype(np.uint64)
        want = np.concatenate([order, np.full(2 * len(syms) + 3 * len(absent), n)]).astype(np.uint64)
        return k, c, want


def check_index(V, idx, truth, absent, samples=(64, 0)):
    n = truth.n
    info = idx.info()
    assert info["n"] == n
    i = np.concatenate([np.arange(n, dtype=np.uint64), np.array([n, 2 ** 63], np.uint64)])
    lf = idx.lf(i)
    assert np.array_equal(lf[:n], truth.lf) and (lf[n:] == NONE).all()
    bwt = idx.bwt(i)
    assert np.array_equal(bwt[:n].astype(np.uint64), truth.bwt.astype(np.uint64)) and not bwt[n:].any()
    assert idx.lf(n - 1) == int(truth.lf[n - 1]) and idx.bwt(0) == int(truth.bwt[0])
    k, c, want = truth.select_queries(absent)
    for sample in samples:
        ss = idx.select_support(sample)
        got = ss.select(k, c)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (sample, int(k[bad[0]]), int(c[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
        psi = ss.psi(i)
        assert np.array_equal(psi[:n], truth.psi) and (psi[n:] == NONE).all(), sample
        assert np.array_equal(ss.psi(lf[:n]), i[:n]) and np.array_equal(idx.lf(psi[:n]), i[:n])
        assert ss.psi(0) == int(truth.psi[0]) and ss.select(1, int(truth.bwt[0])) == int(np.flatnonzero(truth.bwt == truth.bwt[0])[0])
        assert ss.select(0, 0) == n and ss.select(1, 0) == int(np.flatnonzero(truth.bwt == 0)[0]) and ss.select(2, 0) == n      # the sentinel occurs once


def with_sentinel(text):
    return np.concatenate([np.asarray(text), np.zeros(1, dtype=np.asarray(text).dtype)])


BYTE_TEXTS = {
    "dna": dna_text(3000, 5),
    "skewed": skewed_text(2500, 9),
    "all255": np.random.default_rng(1).permutation(np.tile(np.arange(1, 256, dtype=np.uint8), 8)),
    "run": np.frombuffer(b"a" * 500, np.uint8),
    "one": np.frombuffer(b"x", np.uint8),
}


# (name, force): the ids of the force=None cases stay "<name>"
BYTE_CASES = [pytest.param(name, force, id=name + ("-pos64=" + force if force else "")) for name in sorted(BYTE_TEXTS) for force in (None, "2")]


@pytest.mark.parametrize("name,force", BYTE_CASES)
def test_byte_select_psi_lf_bwt(torch_cuda, V, monkeypatch, name, force):
    """force: VLG_FORCE_POS64 -- "2" builds the index with 64-bit samples and wide SA indices: lf_bwt_kernel's kWide arms, and select and
    psi on a wide index"""
    if force:
        monkeypatch.setenv("VLG_FORCE_POS64", force)
    text = BYTE_TEXTS[name]
    full = with_sentinel(text).astype(np.uint8)
    sa = naive_sa(full)
    truth = Truth(full, sa)
    assert np.array_equal(truth.bwt, bwt_from_sa(full, sa))
    absent = np.setdiff1d(np.arange(256), np.unique(full))
    idx = V.VlgIndex.build(text.tobytes(), dens=32)
    if force:
        assert idx.info()["pos_bytes"] == 8
    for ix in (idx, idx.compress(), idx.resample(text_order=True, dens=8), idx.compress().resample(text_order=True, dens=8)):
        check_index(V, ix, truth, absent)


def _int_texts():
    rng = np.random.default_rng(17)
    big = np.unique(np.concatenate([rng.integers(1, 2 ** 32 - 1, 49, dtype=np.uint64), np.array([1, 2 ** 32 - 1], np.uint64)]))
    many = np.concatenate([np.arange(1, 80002), rng.integers(1, 80002, 200000 - 80001)])
    return {"three": rng.integers(1, 4, 3000).astype(np.uint32),
            "wide": rng.choice(big, 3000).astype(np.uint32),
            "many": rng.permutation(many).astype(np.uint32)}


INT_TEXTS = _int_texts()


@pytest.mark.parametrize("name", sorted(INT_TEXTS))
def test_int_select_psi_lf_bwt(torch_cuda, V, name, tmp_path):
    text = INT_TEXTS[name]
    full = with_sentinel(text).astype(np.uint32)
    if len(full) <= 5000:                                               # the naive sort, and the doubling sort checked against it
        t = [int(x) for x in full]
        sa = np.array(sorted(range(len(t)), key=lambda i: t[i:]), np.int64)
        assert np.array_equal(sa, suffix_array_doubling(full))
    else:
        sa = suffix_array_doubling(full)
    truth = Truth(full, sa)
    present = [int(x) for x in np.unique(full)]
    absent = [x for x in (present[-1] + 1, present[len(present) // 2] + 1, 2 ** 32 - 1) if x < 2 ** 32 and x not in present]
    if name == "many":
        assert len(present) == 80002 and V.VlgIndex.build_int(text).info()["max_code_len"] == 17
    idx = V.VlgIndex.build_int(text)
    path = str(tmp_path / "int.sdsl")
    idx.save_sdsl(path)
    for ix in (idx, idx.compress(), idx.resample(text_order=True, dens=8), idx.compress().resample(text_order=True, dens=8),
               V.VlgIndex.load_sdsl_int(path)):
        check_index(V, ix, truth, absent)


# ---- 2^20 symbols: identities through the existing entry points ------------------------------------------------------------------------------
def _sa_batch(torch, V, idx, pos):
    d_i = dev_u64(torch, pos)
    d_o = torch.zeros_like(d_i)
    V.capi.check(V.lib().vlg_sa_batch(idx._h, d_i.data_ptr(), d_o.data_ptr(), len(pos), None))
    return host_u64(d_o)


def _rank(torch, V, idx, pos, sym, is_int):
    d_i = dev_u64(torch, pos)
    d_s = torch.from_numpy(sym.astype(np.uint32).view(np.int32) if is_int else sym.astype(np.uint8)).cuda()
    d_o = torch.zeros_like(d_i)
    f = V.lib().vlg_int_rank_batch if is_int else V.lib().vlg_wt_rank_batch
    V.capi.check(f(idx._h, d_i.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), len(pos), None))
    return host_u64(d_o)


@pytest.mark.parametrize("alphabet", ["byte", "int"])
def test_select_identities_at_2_20(torch_cuda, V, alphabet):
    n_text = (1 << 20) - 1
    rng = np.random.default_rng(20)
    if alphabet == "byte":
        text = skewed_text(n_text, 3)
        base = V.VlgIndex.build(text.tobytes(), dens=32)
    else:
        text = (1 + np.minimum(rng.zipf(1.3, n_text), 50000)).astype(np.uint32)
        base = V.VlgIndex.build_int(text)
    is_int = alphabet == "int"
    n = n_text + 1
    syms, counts = np.unique(text, return_counts=True)
    m = 10 ** 5
    for idx in (base, base.compress()):
        ss = idx.select_support()
        if not is_int and idx is base:
            assert ss.hbm_bytes() <= idx.info()["hbm_bytes"] // 8
        # (k, c) with c drawn as the text draws it
        c = text[rng.integers(0, n_text, m)]
        k = (1 + rng.integers(0, 2 ** 62, m) % counts[np.searchsorted(syms, c)]).astype(np.uint64)
        p = ss.select(k, c)
        assert (p < n).all()
        assert np.array_equal(idx.bwt(p).astype(np.uint64), c.astype(np.uint64))
        assert np.array_equal(_rank(torch_cuda, V, idx, p, c, is_int), k - 1)
        i = rng.integers(0, n, m).astype(np.uint64)
        psi, lf = ss.psi(i), idx.lf(i)
        sa = _sa_batch(torch_cuda, V, idx, i)
        assert np.array_equal(_sa_batch(torch_cuda, V, idx, psi), (sa + 1) % n)
        assert np.array_equal(_sa_batch(torch_cuda, V, idx, lf), (sa + n - 1) % n)
        assert np.array_equal(idx.lf(psi), i)


# ---- handles and refusals ------------------------------------------------------------------------------------------------------------------
def test_support_on_attached_blob_and_two_streams(torch_cuda, V):
    torch = torch_cuda
    text = BYTE_TEXTS["skewed"]
    full = with_sentinel(text).astype(np.uint8)
    truth = Truth(full, naive_sa(full))
    idx = V.VlgIndex.build(text.tobytes(), dens=32)
    nbytes = idx.blob_bytes()
    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idx.blob_export(blob.data_ptr(), nbytes)
    torch.cuda.synchronize()
    att = V.VlgIndex.attach_blob(blob.data_ptr(), nbytes, keep=blob)
    absent = np.setdiff1d(np.arange(256), np.unique(full))
    check_index(V, att, truth, absent, (64,))
    k, c, want = truth.select_queries(absent)
    a, b = idx.select_support(64), idx.select_support(0)
    assert np.array_equal(att.select_support().select(k, c), a.select(k, c))
    # two supports on one index, two streams, device tensors
    d_k, d_c = dev_u64(torch, k), torch.from_numpy(c.astype(np.uint8)).cuda()
    d_i = dev_u64(torch, np.arange(truth.n))
    outs = [torch.zeros_like(d_k), torch.zeros_like(d_k)]
    psis = [torch.zeros_like(d_i), torch.zeros_like(d_i)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for s, sup, o, ps in zip(streams, (a, b), outs, psis):
        with torch.cuda.stream(s):
            sup.select_device(d_k.data_ptr(), d_c.data_ptr(), o.data_ptr(), len(k), stream=s.cuda_stream)
            sup.psi_device(d_i.data_ptr(), ps.data_ptr(), truth.n, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o, ps in zip(outs, psis):
        assert np.array_equal(host_u64(o), want) and np.array_equal(host_u64(ps), truth.psi)
    d_lf, d_bwt = torch.zeros_like(d_i), torch.zeros(truth.n, dtype=torch.uint8, device="cuda")
    idx.lf_device(d_i.data_ptr(), d_lf.data_ptr(), truth.n)
    idx.bwt_device(d_i.data_ptr(), d_bwt.data_ptr(), truth.n)
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(d_lf), truth.lf) and np.array_equal(d_bwt.cpu().numpy(), truth.bwt)


def test_select_refusals_and_empty_batches(torch_cuda, V):
    torch = torch_cuda
    L, E = V.lib(), V.capi.E_INVALID
    bits = (np.random.default_rng(4).random(5000) < 0.5).astype(np.uint8)
    bv = V.BitVector(pack_bits(bits), len(bits))
    sb = bv.select_support()
    byte_idx = V.VlgIndex.build(BYTE_TEXTS["dna"].tobytes())
    int_idx = V.VlgIndex.build_int(INT_TEXTS["three"])
    s_byte, s_int = byte_idx.select_support(), int_idx.select_support()
    d = dev_u64(torch, np.arange(1, 9))
    o = torch.full_like(d, -7)
    p, q = d.data_ptr(), o.data_ptr()
    assert L.vlg_wt_select_batch(sb._h, p, p, q, 8, None) == E and L.vlg_int_select_batch(sb._h, p, p, q, 8, None) == E
    assert L.vlg_psi_batch(sb._h, p, q, 8, None) == E
    assert L.vlg_bit_select_batch(s_byte._h, 1, p, q, 8, None) == E and L.vlg_bit_select_batch(s_int._h, 0, p, q, 8, None) == E
    assert L.vlg_int_select_batch(s_byte._h, p, p, q, 8, None) == E and L.vlg_wt_select_batch(s_int._h, p, p, q, 8, None) == E
    assert L.vlg_bit_select_batch(sb._h, 2, p, q, 8, None) == E
    for sample in (1, 100, 63, 1 << 20):
        with pytest.raises(V.VlgError) as e:
            bv.select_support(sample)
        assert e.value.status == E
    # count = 0: nothing happens, whatever the pointers
    assert L.vlg_bit_select_batch(sb._h, 1, None, None, 0, None) == 0 and L.vlg_wt_select_batch(s_byte._h, None, None, None, 0, None) == 0
    assert L.vlg_int_select_batch(s_int._h, None, None, None, 0, None) == 0 and L.vlg_psi_batch(s_byte._h, None, None, 0, None) == 0
    assert L.vlg_lf_batch(byte_idx._h, None, None, 0, None) == 0 and L.vlg_bwt_batch(int_idx._h, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (o == -7).all()
    assert len(sb.bit_select(np.zeros(0, np.uint64))) == 0 and len(s_byte.psi(np.zeros(0, np.uint64))) == 0
    # the device forms on torch tensors
    sb.bit_select_device(p, q, 8, bit=0)
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(o), np.flatnonzero(bits == 0)[:8].astype(np.uint64))
