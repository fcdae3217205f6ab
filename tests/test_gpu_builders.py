"""The three device builders on adversarial texts -- the ones that force the most prefix-doubling rounds, long common prefixes and
grid edges -- exact against the CPU oracle, and every device suffix array also certified against its text (tests/sa_certificate.py):
  * byte FM-index: vlg_suffix_array_device == oracle.suffix_array; VlgIndex.build(t, dens).export_parts() == the oracle's parts;
  * integer FM-index (build_int), symbols whose encoding holds zero bytes: csa[i] for every i, int_alphabet(), wt_int ranks;
  * the paper's index (WtsaIndex, byte and integer): wt[i] == SA[i] for every i."""
import numpy as np
import pytest

from sa_certificate import certify_suffix_array

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


def _fib(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _thue_morse(n):
    i = np.arange(n, dtype=np.uint64)
    par = np.zeros(n, dtype=np.uint64)
    for k in range(64):
        par ^= (i >> np.uint64(k)) & np.uint64(1)
    return np.where(par == 1, ord("b"), ord("a")).astype(np.uint8).tobytes()


def _periodic(p, n, seed):
    """period-p text of n bytes with one byte changed near the start and one near the end"""
    base = np.random.default_rng(seed).integers(ord("a"), ord("z") + 1, p).astype(np.uint8)
    t = np.tile(base, n // p + 1)[:n].copy()
    t[3] = ord("A")
    t[n - 5] = ord("Z")
    return t.tobytes()


BYTE_TEXTS = {"a%d" % k: (lambda k=k: b"a" * k) for k in list(range(1, 18)) + [255, 256, 257, 4095, 4096, 4097, 1 << 20]}
BYTE_TEXTS.update({
    "ab_x60000": lambda: b"ab" * 60000,
    "aab_x50000": lambda: b"aab" * 50000,
    "fibonacci_2^20": lambda: _fib(1 << 20),
    "thue_morse_2^20": lambda: _thue_morse(1 << 20),
    "period7_1MiB": lambda: _periodic(7, 1 << 20, 1),
    "period64_2MiB": lambda: _periodic(64, 2 << 20, 2),
    "period1000_4MiB": lambda: _periodic(1000, 4 << 20, 3),
    "ff_run_01": lambda: b"\xff" * 70000 + b"\x01",
    "high_runs": lambda: (b"\x80" * 3000 + b"\xff" * 5000 + b"\xfe") * 8 + b"\x81",
    "all_bytes": lambda: bytes(range(1, 256)),
    "all_bytes_x2": lambda: bytes(range(1, 256)) * 2,
    "all_bytes_x300": lambda: bytes(range(1, 256)) * 300,
})
# dens 1 and 64 (every suffix sampled / a sparser grid than the default) on a subset
DENS_TEXTS = ["a1", "a8", "a9", "a17", "a4097", "ab_x60000", "fibonacci_2^20", "period7_1MiB", "ff_run_01", "all_bytes_x2"]


def _device_sa(torch, V, text):
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_sa = torch.zeros(len(text) + 1, dtype=torch.int32, device="cuda")
    V.capi.check(V.lib().vlg_suffix_array_device(d_text.data_ptr(), len(text), d_sa.data_ptr(), None))
    torch.cuda.synchronize()
    return d_text, d_sa.to(torch.int64) & 0xFFFFFFFF


@pytest.mark.parametrize("name", list(BYTE_TEXTS))
def test_byte_builder_adversarial(torch_cuda, V, oracle, name):
    from test_gpu_parity import assert_parts_equal
    torch = torch_cuda
    text = BYTE_TEXTS[name]()
    d_text, d_sa = _device_sa(torch, V, text)
    certify_suffix_array(d_text, d_sa)
    sa = oracle.suffix_array(np.frombuffer(text + b"\0", np.uint8))
    assert (d_sa.cpu().numpy().view(np.uint64) == sa).all()
    for dens in ([1, 32, 64] if name in DENS_TEXTS else [32]):
        assert_parts_equal(V.VlgIndex.build(text, dens).export_parts(), oracle.Index.from_text(text, dens).parts())
    # the paper's index over the same text: wt[i] == SA[i] for every i
    w = V.WtsaIndex(text)
    d_i = torch.arange(len(sa), dtype=torch.int64, device="cuda")
    d_o = torch.zeros_like(d_i)
    w.sa_device(d_i.data_ptr(), d_o.data_ptr(), len(sa))
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == sa).all()


def _int_fib(n, a, b):
    return np.where(np.frombuffer(_fib(n), np.uint8) == ord("a"), a, b).astype(np.uint32)


def _int_texts():
    rng = np.random.default_rng(41)
    zero_byte_syms = np.array([256, 65536, 1 << 24, (1 << 32) - 1, 0x01000001, 0x00010000, 0x0100, 0xFF000000], dtype=np.uint32)
    p3 = np.tile(np.array([(1 << 32) - 1, 1 << 24, 256], dtype=np.uint32), 20000)
    p3[2], p3[-4] = 65536, 1
    p1000 = np.tile(rng.choice(zero_byte_syms, 1000), 60)
    p1000[7], p1000[-9] = 3, 0x7FFFFFFF
    t = {"run65536_x%d" % k: np.full(k, 65536, dtype=np.uint32) for k in (1, 2, 7, 8, 9, 16, 17, 257)}
    t.update({
        "run256_x5000": np.full(5000, 256, dtype=np.uint32),
        "run2^24_x70000": np.full(70000, 1 << 24, dtype=np.uint32),
        "run_max_then_1": np.concatenate([np.full(40000, (1 << 32) - 1, dtype=np.uint32), np.array([1], dtype=np.uint32)]),
        "period_256_65536": np.tile(np.array([256, 65536], dtype=np.uint32), 30000),
        "period3_changed": p3,
        "period1000_changed": p1000,
        "fibonacci_256_2^24": _int_fib(1 << 16, 256, 1 << 24),
        "zero_bytes_random": rng.choice(zero_byte_syms, 30000),
    })
    return t


INT_TEXTS = _int_texts()


@pytest.mark.parametrize("name", list(INT_TEXTS))
def test_int_builder_adversarial(torch_cuda, V, oracle, name):
    torch = torch_cuda
    text = INT_TEXTS[name]
    o = oracle.IntIndex(text.astype(np.uint64), dens=1)
    sa = o.samples()                                                     # dens 1: SA[0], SA[1], ...
    assert len(sa) == o.n == len(text) + 1
    certify_suffix_array(torch.from_numpy(text.astype(np.int64)), torch.from_numpy(sa.view(np.int64)))
    idx = V.VlgIndex.build_int(text)
    assert idx.info()["n"] == o.n
    Cc, c2c = idx.int_alphabet()
    o32 = oracle.IntIndex(text.astype(np.uint64), dens=32)
    assert Cc.tolist() == o32.C().tolist() and c2c.tolist() == o32.comp2char().tolist()
    L = V.lib()
    d_i = torch.arange(o.n, dtype=torch.int64, device="cuda")
    d_v = torch.zeros_like(d_i)
    V.capi.check(L.vlg_sa_batch(idx._h, d_i.data_ptr(), d_v.data_ptr(), o.n, None))
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy().view(np.uint64) == sa).all()
    # wt_int::rank(i, c) for present symbols, absent ones (some with zero bytes) and every grid edge
    rng = np.random.default_rng(7)
    bwt = o.bwt()
    syms = np.unique(np.concatenate([np.unique(text).astype(np.uint64), np.array([1, 2, 256, 65536, 1 << 24, (1 << 32) - 1], np.uint64)]))
    pos = np.unique(np.concatenate([rng.integers(0, o.n + 1, 3000), np.arange(0, o.n + 1, 64), [0, 1, o.n - 1, o.n]])).astype(np.uint64)
    P, S = np.meshgrid(pos, syms, indexing="ij")
    P, S = P.ravel(), S.ravel()
    want = np.zeros(len(P), dtype=np.uint64)
    for c in syms:
        cs = np.concatenate([[0], np.cumsum(bwt == c)]).astype(np.uint64)
        m = S == c
        want[m] = cs[P[m].astype(np.int64)]
    d_p = torch.from_numpy(P.view(np.int64)).cuda()
    d_s = torch.from_numpy(S.astype(np.uint32).view(np.int32)).cuda()
    d_o = torch.zeros(len(P), dtype=torch.int64, device="cuda")
    V.capi.check(L.vlg_int_rank_batch(idx._h, d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), len(P), None))
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == want).all()
    # the paper's index over the integer text
    w = V.WtsaIndex(text)
    d_o = torch.zeros_like(d_i)
    w.sa_device(d_i.data_ptr(), d_o.data_ptr(), o.n)
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == sa).all()


def test_failure_paths_free_their_scratch(torch_cuda, V):
    """A builder that fails after it has allocated device scratch gives all of it back: 64 refused calls of each of
      * build_int on 2^19 symbols whose last one is 0 (VLG_E_ZERO_BYTE, after the text and the suffix-array flags, 12 MiB, are on the device),
      * vlg_wtsa_from_parts, through the Python loader, on the dna_3000 golden with one count word altered (VLG_E_INVALID),
      * resample of a text-order index (VLG_E_INVALID),
    with the device's free memory read before and after (a build_int that freed nothing would be down 768 MiB), and a
    build_int and a WtsaIndex built right after still pass the suffix-array certificate."""
    import os
    from vlg_matching_amd import capi
    from vlg_matching_amd.index import read_sdsl_wtsa_file
    torch = torch_cuda

    def refused(call, status):
        with pytest.raises(V.VlgError) as e:
            call()
        assert e.value.status == status

    with_zero = np.full(1 << 19, 7, dtype=np.uint32)
    with_zero[-1] = 0
    good = read_sdsl_wtsa_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wtsa_sdsl", "dna_3000.sdsl"))
    damaged = dict(good, data=good["data"].copy())
    damaged["data"][9 * 3] ^= np.uint64(1)
    text = INT_TEXTS["zero_bytes_random"]
    text_order = V.VlgIndex.build_int(text).resample(text_order=True, dens=16)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(64):
        refused(lambda: V.VlgIndex.build_int(with_zero), capi.E_ZERO_BYTE)
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info()[0]
    print("free device memory: %d before, %d after 64 refused build_int calls" % (free_before, free_after))
    assert free_before - free_after < 128 << 20
    for _ in range(64):
        refused(lambda: V.WtsaIndex.from_parts(damaged), capi.E_INVALID)
        refused(lambda: text_order.resample(text_order=False, dens=32), capi.E_INVALID)
    # right after: both builders still work
    n = len(text) + 1
    d_text = torch.from_numpy(text.astype(np.int64)).cuda()
    d_i = torch.arange(n, dtype=torch.int64, device="cuda")
    d_sa = torch.zeros_like(d_i)
    idx = V.VlgIndex.build_int(text)
    V.capi.check(V.lib().vlg_sa_batch(idx._h, d_i.data_ptr(), d_sa.data_ptr(), n, None))
    torch.cuda.synchronize()
    certify_suffix_array(d_text, d_sa)
    d_sa.zero_()
    V.WtsaIndex(text).sa_device(d_i.data_ptr(), d_sa.data_ptr(), n)
    torch.cuda.synchronize()
    certify_suffix_array(d_text, d_sa)
