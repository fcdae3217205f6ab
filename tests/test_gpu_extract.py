"""Text access on the device (vlg_text_access_create, vlg_extract_batch, vlg_isa_batch): sdsl::extract(csa, begin, end)
(include/sdsl/suffix_array_algorithm.hpp:645-745), csa.text[i] and csa.isa[i] (csa_wt.hpp:145-151) from ISA samples kept in HBM, for
byte and integer indexes, plain and rrr, at every SA density.  Every check is against the text itself; ISA against the inverse of the
naive suffix array (small texts) or against csa[ISA[i]] = i (large ones)."""
import numpy as np
import pytest

from util import dna_text, naive_sa, skewed_text

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


def dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def with_sentinel(text):
    return np.concatenate([np.asarray(text), np.zeros(1, dtype=np.asarray(text).dtype)])


def int_naive_isa(text):
    t = [int(x) for x in text] + [0]
    sa = sorted(range(len(t)), key=lambda i: t[i:])
    isa = np.zeros(len(t), np.uint64)
    isa[np.array(sa, dtype=np.int64)] = np.arange(len(t), dtype=np.uint64)
    return isa


def byte_naive_isa(text):
    sa = naive_sa(with_sentinel(text))
    isa = np.zeros(len(sa), np.uint64)
    isa[sa.astype(np.int64)] = np.arange(len(sa), dtype=np.uint64)
    return isa


def sa_batch(torch, V, idx, pos):
    d_i = dev_u64(torch, pos)
    d_o = torch.zeros_like(d_i)
    V.capi.check(V.lib().vlg_sa_batch(idx._h, d_i.data_ptr(), d_o.data_ptr(), len(pos), None))
    return host_u64(d_o)


def edge_ranges(n, d, rng, n_random):
    """single symbols, [0, n-1], ranges on / across block edges, the last block, and random ones"""
    r = [(0, 0), (n - 1, n - 1), (0, n - 1), (n // 2, n // 2)]
    for k in range(0, n, d) if n // d < 200 else list(range(0, 200 * d, d)) + [((n - 1) // d) * d]:
        for b, e in ((k, k), (k, min(n - 1, k + d - 1)), (max(0, k - 1), min(n - 1, k + 1)), (max(0, k - d), min(n - 1, k + d)),
                     (k, min(n - 1, k + 3 * d + 1))):
            r.append((b, e))
    last = ((n - 1) // d) * d
    r += [(last, n - 1), (max(0, last - 1), n - 1), (n - 2 if n > 1 else 0, n - 1)]
    b = rng.integers(0, n, n_random)
    ln = rng.integers(0, min(n, 4 * d + 5), n_random)
    e = np.minimum(b + ln, n - 1)
    r += list(zip(b.tolist(), e.tolist()))
    return np.array([x[0] for x in r], np.uint64), np.array([x[1] for x in r], np.uint64)


def check_text_access(torch, V, idx, full, isa_ref, dens_list, n_random=2000, check_samples=True):
    """full: the text with its sentinel (numpy, the dtype extract returns); isa_ref: ISA or None (then csa[ISA[i]] = i is checked)"""
    n = len(full)
    rng = np.random.default_rng(n)
    for d in dens_list:
        ta = idx.text_access(d)
        b, e = edge_ranges(n, d, rng, n_random)
        out, off = ta.extract_batch(b, e)
        assert len(out) == int(off[-1])
        for r in range(len(b)):
            got = out[int(off[r]): int(off[r + 1])]
            want = full[int(b[r]): int(e[r]) + 1]
            assert np.array_equal(got, want), (d, int(b[r]), int(e[r]))
        whole = ta.extract(0, n - 1)
        whole = np.frombuffer(whole, np.uint8) if isinstance(whole, bytes) else whole
        assert np.array_equal(whole, full), d
        assert int(whole[-1]) == 0
        assert ta.text(n - 1) == 0 and ta.text(0) == int(full[0])
        isa = ta.isa(np.arange(n, dtype=np.uint64))
        if isa_ref is not None:
            assert np.array_equal(isa, isa_ref), d
        else:
            assert np.array_equal(sa_batch(torch, V, idx, isa), np.arange(n, dtype=np.uint64)), d
        assert ta.isa(n - 1) == int(isa[n - 1])
        if check_samples:
            assert np.array_equal(isa[::d], idx.isa_samples(d)), d


BYTE_TEXTS = {
    "dna": dna_text(3000, 5),
    "skewed": skewed_text(2500, 9),
    "all255": np.random.default_rng(1).permutation(np.tile(np.arange(1, 256, dtype=np.uint8), 8)),
}


# (name, force): the ids of the force=None cases stay "<name>"
BYTE_CASES = [pytest.param(name, force, id=name + ("-pos64=" + force if force else "")) for name in sorted(BYTE_TEXTS) for force in (None, "2")]


@pytest.mark.parametrize("name,force", BYTE_CASES)
def test_byte_extract_and_isa(torch_cuda, V, monkeypatch, name, force):
    """force: VLG_FORCE_POS64 -- "2" builds the index with 64-bit samples and wide SA indices, so the same checks run on the kWide arms of
    extract_kernel, isa_kernel and isa_samples_kernel (the 8-byte ISA samples of n >= 2^32 stay out of reach of a small text)"""
    if force:
        monkeypatch.setenv("VLG_FORCE_POS64", force)
    text = BYTE_TEXTS[name]
    full = with_sentinel(text).astype(np.uint8)
    n = len(full)
    isa_ref = byte_naive_isa(text)
    idx = V.VlgIndex.build(text.tobytes(), dens=32)
    if force:
        assert idx.info()["pos_bytes"] == 8
    for ix, label in ((idx, "plain"), (idx.compress(), "rrr"), (idx.resample(text_order=False, dens=1), "sa-dens-1"),
                      (idx.resample(text_order=False, dens=7), "sa-dens-7")):
        check_text_access(torch_cuda, V, ix, full, isa_ref, [1, 3, 64, n + 5])


INT_TEXTS = {
    "small_values": np.random.default_rng(2).integers(1, 6, 3000).astype(np.uint32),
    "large_values": np.random.default_rng(3).choice(np.array([7, 1000, 70000, 2 ** 31 + 5, 2 ** 32 - 2], np.uint64), 2000).astype(np.uint32),
    "one": np.array([42], np.uint32),
}


@pytest.mark.parametrize("name", sorted(INT_TEXTS))
def test_int_extract_and_isa(torch_cuda, V, name):
    text = INT_TEXTS[name]
    full = with_sentinel(text).astype(np.uint32)
    n = len(full)
    isa_ref = int_naive_isa(text)
    idx = V.VlgIndex.build_int(text, dens=16)
    for ix in (idx, idx.compress(), idx.resample(text_order=False, dens=1)):
        check_text_access(torch_cuda, V, ix, full, isa_ref, [1, 3, 64, n + 5])


def test_int_wide_alphabet_and_loaded(torch_cuda, V, tmp_path):
    rng = np.random.default_rng(31)
    big = np.unique(rng.integers(1, 2 ** 32 - 1, 90000, dtype=np.uint64).astype(np.uint32))[:80001]
    assert len(big) == 80001
    text = rng.permutation(np.concatenate([big, rng.choice(big, 40000)])).astype(np.uint32)
    full = with_sentinel(text)
    idx = V.VlgIndex.build_int(text, dens=32)
    for ix in (idx, idx.compress()):
        check_text_access(torch_cuda, V, ix, full, None, [16, 64], n_random=3000)
    path = tmp_path / "wide.sdsl"
    idx.save_sdsl(path)
    loaded = V.VlgIndex.load_sdsl_int(path, dens=32)
    check_text_access(torch_cuda, V, loaded, full, None, [64], n_random=3000)
    check_text_access(torch_cuda, V, loaded.compress(), full, None, [64], n_random=500)


def test_device_tensors(torch_cuda, V):
    torch = torch_cuda
    text = skewed_text(5000, 4)
    full = with_sentinel(text).astype(np.uint8)
    ta = V.VlgIndex.build(text.tobytes()).text_access(16)
    b = np.array([0, 17, 4990, 100], np.uint64)
    e = np.array([5000, 17, 5000, 131], np.uint64)
    out, off = ta.extract_batch(dev_u64(torch, b), dev_u64(torch, e))
    assert out.is_cuda and off.is_cuda
    out, off = out.cpu().numpy(), off.cpu().numpy()
    for r in range(len(b)):
        assert np.array_equal(out[off[r]: off[r + 1]], full[b[r]: e[r] + 1])
    # integer index: int32 device tensor holding the uint32 symbols
    itext = np.array([5, 2 ** 32 - 2, 9, 2 ** 31 + 1] * 50, np.uint32)
    ita = V.VlgIndex.build_int(itext).text_access()
    out, off = ita.extract_batch(dev_u64(torch, [0, 3]), dev_u64(torch, [200, 7]))
    got = out.cpu().numpy().view(np.uint32)
    ifull = with_sentinel(itext)
    assert np.array_equal(got[: int(off[1])], ifull[0:201]) and np.array_equal(got[int(off[1]):], ifull[3:8])


def test_refusals(torch_cuda, V):
    torch = torch_cuda
    C = V.capi
    text = dna_text(1000, 3)
    n = len(text) + 1
    idx = V.VlgIndex.build(text.tobytes(), dens=16)
    for to in (idx.resample(text_order=True, dens=16), V.VlgIndex.build_int(text.astype(np.uint32)).resample(text_order=True, dens=8)):
        with pytest.raises(V.VlgError) as ei:
            to.text_access(64)
        assert ei.value.status == C.E_UNSUPPORTED
    ta = idx.text_access(8)
    L = V.lib()

    def run(b, e, total=None, out_off=None):
        bb, ee = np.array(b, np.uint64), np.array(e, np.uint64)
        lens = np.where(ee >= bb, ee - bb + 1, 1).astype(np.uint64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) if out_off is None else np.array(out_off, np.uint64)
        tot = int(off[-1]) if total is None else total
        d_out = torch.zeros(max(tot, 1) + 64, dtype=torch.uint8, device="cuda")
        d_b, d_e, d_off = dev_u64(torch, bb), dev_u64(torch, ee), dev_u64(torch, off)      # (alive across the call)
        st = L.vlg_extract_batch(ta._h, d_b.data_ptr(), d_e.data_ptr(), d_off.data_ptr(), len(bb), tot, d_out.data_ptr(), None)
        return st, d_out

    assert run([0, 5], [3, 4])[0] == C.E_INVALID                 # begin > end
    assert run([0], [n])[0] == C.E_INVALID                        # end >= n
    assert run([0, 10], [3, 20], total=10)[0] == C.E_INVALID      # output beyond total
    st, d_out = run([5, 0], [4, 3])
    assert st == C.E_INVALID and int(d_out.sum().item()) == 0     # nothing written
    assert run([0, 10], [n - 1, 20])[0] == C.OK
    d = dev_u64(torch, [0])
    assert L.vlg_extract_batch(ta._h, None, d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), None) == C.E_INVALID
    assert L.vlg_extract_batch(None, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), None) == C.E_INVALID
    assert L.vlg_extract_batch(ta._h, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, 1, None, None) == C.E_INVALID
    assert L.vlg_extract_batch(ta._h, None, None, None, 0, 0, None, None) == C.OK
    assert L.vlg_isa_batch(ta._h, None, None, 0, None) == C.OK
    assert L.vlg_isa_batch(ta._h, None, d.data_ptr(), 1, None) == C.E_INVALID
    o = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_p = dev_u64(torch, [3, n])
    assert L.vlg_isa_batch(ta._h, d_p.data_ptr(), o.data_ptr(), 2, None) == C.E_INVALID
    assert L.vlg_text_access_create(None, 64, None, None) == C.E_INVALID
    with pytest.raises(V.VlgError) as ei:
        ta.extract_batch(dev_u64(torch, [5]), dev_u64(torch, [n]))
    assert ei.value.status == C.E_INVALID
    with pytest.raises(ValueError):
        ta.extract(5, 4)
    with pytest.raises(ValueError):
        ta.isa([n])


def test_large_texts(torch_cuda, V):
    torch = torch_cuda
    rng = np.random.default_rng(77)
    n_text = (1 << 20) + 333
    text = skewed_text(n_text, 12)
    full = with_sentinel(text).astype(np.uint8)
    n = len(full)
    idx = V.VlgIndex.build(text.tobytes())
    for d in (64, 1000):
        ta = idx.text_access(d)
        whole = np.frombuffer(ta.extract(0, n - 1), np.uint8)
        assert np.array_equal(whole, full)
        b = rng.integers(0, n, 20000).astype(np.uint64)
        e = np.minimum(b + rng.integers(0, 300, 20000).astype(np.uint64), n - 1)
        out, off = ta.extract_batch(b, e)
        for r in range(0, 20000, 7):
            assert np.array_equal(out[off[r]: off[r + 1]], full[b[r]: e[r] + 1])
        p = rng.integers(0, n, 50000).astype(np.uint64)
        assert np.array_equal(sa_batch(torch, V, idx, ta.isa(p)), p)
        assert np.array_equal(ta.isa(np.arange(0, n, d, dtype=np.uint64)), idx.isa_samples(d))
    itext = (1 + rng.zipf(1.3, 1 << 20) % 30000).astype(np.uint32)
    ifull = with_sentinel(itext)
    iidx = V.VlgIndex.build_int(itext)
    ta = iidx.text_access(64)
    assert np.array_equal(ta.extract(0, len(ifull) - 1), ifull)
    b = rng.integers(0, len(ifull), 20000).astype(np.uint64)
    e = np.minimum(b + rng.integers(0, 300, 20000).astype(np.uint64), len(ifull) - 1)
    out, off = ta.extract_batch(b, e)
    for r in range(0, 20000, 7):
        assert np.array_equal(out[off[r]: off[r + 1]], ifull[b[r]: e[r] + 1])
    p = rng.integers(0, len(ifull), 50000).astype(np.uint64)
    assert np.array_equal(sa_batch(torch, V, iidx, ta.isa(p)), p)


def test_c3_snippets_reduced(torch_cuda, V):
    """the snippet workload of tools/extract_bench.py on a C3 text scaled down: a window of +-64 symbols around the first position of
    every match, which must hold the matched first sub-pattern at the match position"""
    from vlg_matching_amd import workload
    c = workload.config("C3", scale=1.0 / 512)
    text = workload.gen_text(c["kind"], c["n"], c["seed"])
    parts = workload.gen_query_parts(text, c["nq"], c["k"], c["m"], c["qseed"])
    g = ".{%d,%d}?" % c["gap"]
    qs = [g.join(s.decode("latin-1") for s in p) for p in parts]
    idx = V.VlgIndex.build(text.tobytes())
    r = idx.search(qs)
    counts, qoff, first, _ = r.fetch()
    assert len(first) > 100
    qid = np.repeat(np.arange(len(qs)), counts.astype(np.int64))
    n = len(text) + 1
    b = np.maximum(first.astype(np.int64) - 64, 0).astype(np.uint64)
    e = np.minimum(first + 64, n - 1).astype(np.uint64)
    out, off = idx.text_access(64).extract_batch(b, e)
    for j in range(min(len(first), 20000)):
        w = out[int(off[j]): int(off[j + 1])].tobytes()
        at = int(first[j] - b[j])
        sub = parts[qid[j]][0]
        assert w[at: at + len(sub)] == sub, j
    assert np.array_equal(out[int(off[0]): int(off[1])], with_sentinel(text)[int(b[0]): int(e[0]) + 1])
