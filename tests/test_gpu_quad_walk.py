"""The quad image of the byte index's wavelet tree and the LF walk on it (csrc/quad_code.hpp, lf_walk.hpp: QuadWalk).

(a) vlg_quad_lf_batch over EVERY SA index of a text equals vlg_lf_batch and the oracle in LF, in the symbol read and in the levels counted
    (the symbol's code length).
(b) query batches with the workspace option quad_walk = 0 and = 1 give identical summaries ("lf_steps" and "wt_levels_locate" among them)
    and identical fetched arrays, through the in-place walks, the sweep's rounds, the stragglers' kernel alone, with and without shared
    trails, on a text-order resampled index, at density 1, on wide SA indices and on an index attached to an exported blob.
(c) an rrr index and an integer index have no image and search as before.

The texts are the smallest where the walk can go wrong: one symbol (a root of two leaves), a depth-1 leaf beside depth-2 leaves, a spine
with a leaf at every depth to 12, 255 byte values (codes of 7 to 9 bits), and roots of exactly 79, 80, 81, 160 and 161 digits around the
80-digit blocks."""
import numpy as np
import pytest

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


def _letters(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _spine():
    """13 symbols that occur 1, 1, 2, 4, ..., 2^11 times: the Huffman tree is a spine with a leaf at every depth down to 12"""
    counts = [1 << i for i in range(12)]                       # (the sentinel is the second symbol of count 1)
    t = np.concatenate([np.full(c, ord("a") + j, np.uint8) for j, c in enumerate(counts)])
    return np.random.default_rng(7).permutation(t).tobytes()


def _workload(kind):
    from vlg_matching_amd import workload
    return bytes(workload.gen_text(kind, 50000, seed=3))


TEXTS = {
    "empty": lambda: b"",
    "one_symbol": lambda: b"a" * 1000,
    "two_15_to_1": lambda: np.random.default_rng(5).permutation(np.array([ord("a")] * 1500 + [ord("b")] * 100, np.uint8)).tobytes(),
    "spine": _spine,
    "bytes255": lambda: np.random.default_rng(6).integers(1, 256, 20000).astype(np.uint8).tobytes(),
    "dna50k": lambda: _workload("dna"),
    "english50k": lambda: _workload("english"),
    "root79": lambda: _letters(78, 79),
    "root80": lambda: _letters(79, 80),
    "root81": lambda: _letters(80, 81),
    "root160": lambda: _letters(159, 160),
    "root161": lambda: _letters(160, 161),
}
_text_cache = {}


def _text(name):
    if name not in _text_cache:
        _text_cache[name] = TEXTS[name]()
    return _text_cache[name]


SAFE = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ")


def _queries(text, seed, nq=60):
    """gapped queries over sub-patterns cut from the text (only those free of regexp syntax), single symbols among them: long lists"""
    rng = np.random.default_rng(seed)
    subs = []
    for _ in range(100000):
        if len(subs) >= 3 * nq:
            break
        s = int(rng.integers(0, len(text)))
        sub = text[s:s + int(rng.integers(1, 4))]
        if sub and all(b in SAFE for b in sub):
            subs.append(sub.decode("latin-1"))
    assert len(subs) == 3 * nq
    qs = []
    for i in range(nq):
        k = 1 + i % 3
        q = subs[3 * i]
        for j in range(1, k):
            q += ".{0,%d}?%s" % (int(rng.integers(1, 200)), subs[3 * i + j])
        qs.append(q)
    return qs


def _lf_truth(oracle, text):
    """(LF, compact symbol, code length) of every SA index, from the oracle"""
    o = oracle.Index.from_text(text)
    p = o.parts()
    n = o.n
    bwt = o.bwt()
    lf = np.array([o.lf(i) for i in range(n)], dtype=np.uint64)
    comp = p["char2comp"][bwt].astype(np.uint8)
    levels = (p["paths"][bwt] >> np.uint64(56)).astype(np.uint32)
    return lf, comp, levels


def _quad_lf(torch, idx, n):
    d_i = torch.arange(n, dtype=torch.int64, device="cuda")
    d_lf = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_c = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_lv = torch.zeros(n, dtype=torch.int32, device="cuda")
    idx.quad_lf_device(d_i.data_ptr(), d_lf.data_ptr(), d_c.data_ptr(), d_lv.data_ptr(), n)
    return d_lf.cpu().numpy().view(np.uint64), d_c.cpu().numpy(), d_lv.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(TEXTS))
def test_quad_lf_equals_lf_batch_and_oracle(torch_cuda, V, oracle, name):
    text = _text(name)
    idx = V.VlgIndex.build(text)
    info, img = idx.info(), idx.quad_image()
    n = info["n"]
    assert n == len(text) + 1
    lf, comp, levels = _lf_truth(oracle, text)
    got_lf = idx.lf(np.arange(n, dtype=np.uint64))
    assert (np.atleast_1d(got_lf) == lf).all()
    if name == "empty":                                        # sigma = 1: nothing to walk, no image
        assert info["sigma"] == 1 and img == {"bytes": 0, "n_nodes": 0, "build_s": 0.0} and info["hbm_bytes"] == idx.blob_bytes()
        with pytest.raises(V.capi.VlgError) as e:
            _quad_lf(torch_cuda, idx, n)
        assert e.value.status == V.capi.E_UNSUPPORTED
        return
    assert img["bytes"] > 0 and img["n_nodes"] >= 1 and info["hbm_bytes"] == idx.blob_bytes() + img["bytes"]
    q_lf, q_c, q_lv = _quad_lf(torch_cuda, idx, n)
    assert (q_lf == lf).all()
    assert (q_c == comp).all()
    assert (q_lv == levels).all()
    assert int(q_lv.max()) == info["max_code_len"]
    if name == "spine":
        assert info["max_code_len"] == 12 and set(np.unique(q_lv).tolist()) == set(range(1, 13))
    if name == "two_15_to_1":
        assert sorted(np.unique(q_lv).tolist()) == [1, 2]
    # an index past the end answers as vlg_lf_batch does
    d_i = torch_cuda.tensor([n, n + 7], dtype=torch_cuda.int64, device="cuda")
    d_o = torch_cuda.zeros(2, dtype=torch_cuda.int64, device="cuda")
    idx.quad_lf_device(d_i.data_ptr(), d_o.data_ptr(), None, None, 2)
    assert d_o.cpu().numpy().view(np.uint64).tolist() == [2 ** 64 - 1] * 2


PATHS = [
    {"sweep": 0},                                                      # one walk per occurrence in place (locate_kernel)
    {"sweep_min": 1, "sweep_tail": 0},                                 # the sweep's rounds to the last element
    {"sweep_min": 1, "sweep_tail": 1 << 30},                           # the stragglers' kernel alone
    {"sweep_min": 1, "sweep_tail": 0, "trail": 0},
    {"sweep_min": 1, "sweep_tail": 1 << 30, "trail": 0},
    {"sweep_min": 1, "sweep_tail": 16},                                # rounds, then stragglers on shared trails
]


def _same_both_ways(idx, qs, paths=PATHS):
    from vlg_matching_amd.index import Workspace
    steps = 0
    for opts in paths:
        out = []
        for quad in (0, 1):
            ws = Workspace()
            for k, v in dict(opts, quad_walk=quad).items():
                ws.set_option(k, v)
            res = idx.search(qs, workspace=ws)
            out.append((res.summary, res.fetch(), ws.kernel_stats()))
        (s0, f0, k0), (s1, f1, k1) = out
        assert s0 == s1, (opts, s0, s1)
        assert s0["located_occurrences"] > 0 and k0["locate"]["launches"] > 0 and k0["locate"]["launches"] == k1["locate"]["launches"], opts
        for x, y in zip(f0, f1):
            assert (x == y).all(), opts
        steps += s0["lf_steps"]
    return steps


@pytest.mark.parametrize("name", [n for n in TEXTS if n != "empty"])
def test_queries_same_with_and_without_the_image(V, name):
    text = _text(name)
    idx = V.VlgIndex.build(text)
    assert idx.quad_image()["bytes"] > 0
    assert _same_both_ways(idx, _queries(text, 100 + len(text))) > 0 or len(text) < 200


@pytest.mark.parametrize("name", ["spine", "english50k"])
def test_resampled_dense_and_attached_indexes(torch_cuda, V, name):
    text = _text(name)
    qs = _queries(text, 7)
    idx = V.VlgIndex.build(text)
    # text-order samples: the marks are probed between the quad steps
    to = idx.resample(text_order=True, dens=16)
    assert to.info()["sampling"] == 1 and to.quad_image()["bytes"] == idx.quad_image()["bytes"]
    assert _same_both_ways(to, qs) > 0
    # every SA index sampled: no LF step either way
    dense = idx.resample(text_order=False, dens=1)
    assert dense.quad_image()["bytes"] > 0
    assert _same_both_ways(dense, qs) == 0
    # an exported blob carries no image; the index attached to it derives its own
    nbytes = idx.blob_bytes()
    assert idx.info()["hbm_bytes"] == nbytes + idx.quad_image()["bytes"]
    d_blob = torch_cuda.zeros(nbytes, dtype=torch_cuda.uint8, device="cuda")
    idx.blob_export(d_blob.data_ptr(), nbytes)
    att = V.VlgIndex.attach_blob(d_blob.data_ptr(), nbytes, keep=d_blob)
    assert att.quad_image()["bytes"] == idx.quad_image()["bytes"] and att.quad_image()["n_nodes"] == idx.quad_image()["n_nodes"]
    n = att.info()["n"]
    a, b = _quad_lf(torch_cuda, att, n), _quad_lf(torch_cuda, idx, n)
    for x, y in zip(a, b):
        assert (x == y).all()
    assert _same_both_ways(att, qs, PATHS[:3]) > 0


@pytest.mark.parametrize("name,force", [("spine", "1"), ("english50k", "2"), ("root81", "2")])
def test_wide_sa_indices(torch_cuda, V, oracle, monkeypatch, name, force):
    """VLG_FORCE_POS64: QuadWalk<true> -- 64-bit node-relative positions -- in all three kernels and in the test entry (quad_walk = 0:
    round 0 of the sweep in the binary pairs of sweep_first_pair)"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text = _text(name)
    idx = V.VlgIndex.build(text)
    assert idx.info()["pos_bytes"] == 8 and idx.quad_image()["bytes"] > 0
    lf, comp, levels = _lf_truth(oracle, text)
    q_lf, q_c, q_lv = _quad_lf(torch_cuda, idx, idx.info()["n"])
    assert (q_lf == lf).all() and (q_c == comp).all() and (q_lv == levels).all()
    assert _same_both_ways(idx, _queries(text, 9)) > 0 or len(text) < 200


def test_rrr_and_integer_indexes_have_no_image(torch_cuda, V):
    from vlg_matching_amd.index import Workspace
    text = _text("english50k")
    qs = _queries(text, 11)
    plain = V.VlgIndex.build(text)
    rrr = plain.compress()
    assert rrr.quad_image() == {"bytes": 0, "n_nodes": 0, "build_s": 0.0} and rrr.info()["hbm_bytes"] == rrr.blob_bytes()
    with pytest.raises(V.capi.VlgError) as e:
        _quad_lf(torch_cuda, rrr, 4)
    assert e.value.status == V.capi.E_UNSUPPORTED
    want = plain.search(qs)
    for quad in (0, 1):                                          # (the option changes nothing where there is no image)
        ws = Workspace()
        ws.set_option("quad_walk", quad)
        got = rrr.search(qs, workspace=ws)
        for k in ("n_matches", "checksum", "located_occurrences", "lf_steps", "wt_levels_locate"):
            assert got.summary[k] == want.summary[k], k
        for x, y in zip(got.fetch(), want.fetch()):
            assert (x == y).all()
    ints = np.frombuffer(text, np.uint8).astype(np.uint32)
    ii = V.VlgIndex.build_int(ints)
    assert ii.quad_image() == {"bytes": 0, "n_nodes": 0, "build_s": 0.0}
    with pytest.raises(V.capi.VlgError) as e:
        _quad_lf(torch_cuda, ii, 4)
    assert e.value.status == V.capi.E_UNSUPPORTED
    iq = ["%d %d .{0,50}? %d" % (ints[100], ints[101], ints[140]), "%d" % ints[5]]
    res = []
    for quad in (0, 1):
        ws = Workspace()
        ws.set_option("quad_walk", quad)
        r = ii.search(iq, workspace=ws)
        res.append((r.summary, r.fetch()))
    assert res[0][0] == res[1][0] and res[0][0]["n_matches"] > 0
    for x, y in zip(res[0][1], res[1][1]):
        assert (x == y).all()
