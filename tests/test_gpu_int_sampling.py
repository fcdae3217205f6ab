"""SA sampling options of the integer-alphabet FM-index: vlg_index_resample of an integer index into
text_order_sa_sampling (csa_sampling_strategy.hpp:127-246) or SA-order sampling of another density -- the resident suffix array at
density 1 -- and vlg_index_isa_samples of an integer index (:626-642), against the restated reference (oracle/vlg_oracle_int.c).
The reference's own integer CSA test types this covers: csa_wt<wt_int<>, 16, 16, text_order_sa_sampling<>, ., int_alphabet<>>
(test/csa_int_test.cpp:29-34), plain and over wt_int<rrr_vector<63>>."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SORTED_SWEEP_OFF = 1 << 30
QUADRATIC_MAX = 1000            # texts on which a text-order density above n (every walk to the text's start) is tested


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()                      # fails loudly if the HIP extension is missing
    return v


def dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def _texts():
    rng = np.random.default_rng(31)
    big = rng.integers(1, 2 ** 32 - 1, 80000, dtype=np.uint64).astype(np.uint32)          # 80 000 draws of symbols: sigma > 65534
    big = np.unique(big)[:80000]
    return {
        "survey": np.array([5, 6, 7, 5, 6, 7, 1000, 5], dtype=np.uint32),
        "abra": np.frombuffer(b"abracadabrasimsalabim", dtype=np.uint8).astype(np.uint32),
        "sparse": rng.choice(np.array([3, 7, 7, 19, 1000, 70000, 2 ** 31 + 5], dtype=np.uint32), 5000),
        "words": (1 + rng.zipf(1.3, 20000) % 3000).astype(np.uint32),
        "one": np.array([42], dtype=np.uint32),
        "run": np.full(300, 9, dtype=np.uint32),
        # the reference's own integer fixture (test/test_cases/keeper.int: 63 symbols of 8 bytes), kept as data
        "keeper": np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keeper.int"), dtype="<u8").astype(np.uint32),
        # every one of ~80 000 distinct symbols at least once in 150 000 tokens: not eligible for the sorted sweep (16-bit key), so
        # locate inside vlg_search_batch is the lane-per-occurrence kernel
        "wide_sigma": rng.permutation(np.concatenate([big, rng.choice(big, 150000 - len(big))])).astype(np.uint32),
    }


TEXTS = _texts()
NAMES = list(TEXTS)


def _queries(text, rng, nq, kmax=3, mmax=3, gapmax=40):
    t = text.tolist()
    qs = []
    for _ in range(nq):
        k = int(rng.integers(1, kmax + 1))
        subs = [t[s:s + int(rng.integers(1, mmax + 1))] for s in rng.integers(0, max(len(t) - mmax, 1), k)]
        q = " ".join(map(str, subs[0]))
        for sp in subs[1:]:
            a = int(rng.integers(0, 10))
            q += " .{%d,%d}? %s" % (a, a + int(rng.integers(0, gapmax)), " ".join(map(str, sp)))
        qs.append(q)
    return qs


_CACHE = {}


def _case(oracle, name):
    """(oracle of the SA-order d = 32 index, suffix array, queries, wanted tuples) of one text, computed once"""
    if name not in _CACHE:
        text = TEXTS[name]
        o = oracle.IntIndex(text.astype(np.uint64), dens=32)
        tz = np.concatenate([text.astype(np.int64), [0]])
        if len(tz) <= 6000:
            sa = np.array(sorted(range(len(tz)), key=lambda i: tz[i:].tolist()), dtype=np.int64)
        else:
            o1 = oracle.IntIndex(text.astype(np.uint64), dens=1)
            sa = np.array([o1.sa(i) for i in range(o1.n)], dtype=np.int64)
        rng = np.random.default_rng(17)
        qs = _queries(text, rng, 60) + ["%d .{0,5}? 999999" % int(text[0]), "%d" % int(text[-1])]
        want = [o.search(q).tolist() for q in qs]
        _CACHE[name] = (o, sa, qs, want)
    return _CACHE[name]


def _sa_batch(torch, V, idx, n):
    d_i = dev_u64(torch, np.arange(n, dtype=np.uint64))
    d_o = torch.zeros_like(d_i)
    V.capi.check(V.lib().vlg_sa_batch(idx._h, d_i.data_ptr(), d_o.data_ptr(), n, None))
    torch.cuda.synchronize()
    return host_u64(d_o).astype(np.int64)


_WS = {}


def _workspace(opts):
    """one workspace per option set for the whole module (a workspace keeps its arena and pinned host blocks from batch to batch)"""
    key = tuple(sorted(opts.items()))
    if key not in _WS:
        from vlg_matching_amd.index import Workspace
        ws = Workspace()
        for k, v in opts.items():
            ws.set_option(k, v)
        _WS[key] = ws
    return _WS[key]


def _located_steps(o, sa, qs, dens):
    """sum of SA[i] % dens over the occurrences that are located (a query with an absent sub-pattern locates nothing)"""
    steps = 0
    for q in qs:
        pats = [[int(x) for x in part.split()] for part in re.split(r"\.\{\d+,\d+\}\?", q)]
        occs = [o.backward_search(p) for p in pats]
        if min(c for c, _, _ in occs) == 0:
            continue
        for c, l, r in occs:
            steps += int((sa[l:r + 1] % dens).sum())
    return steps


def _assert_status(V, status, fn):
    with pytest.raises(V.VlgError) as e:
        fn()
    assert e.value.status == status, e.value


@pytest.mark.parametrize("rrr", [False, True], ids=["plain", "rrr"])
@pytest.mark.parametrize("name", NAMES)
def test_int_text_order_resample(torch_cuda, V, oracle, name, rrr):
    """csa_wt<wt_int<>, d, ., text_order_sa_sampling<>, ., int_alphabet<>> made by vlg_index_resample from an SA-order integer index
    (plain, or compressed first): the marks equal the restated reference's and (SA % d == 0), csa[i] == SA[i] for every i, every locate
    mode returns the oracle's tuples and the SA-order index's checksum -- with exactly sum(SA[i] % d) LF steps, the text-order oracle's
    count, when nothing is shared -- and the image travels as a blob.  A density above n samples SA = 0 alone, so every walk runs to the
    start of the text (n^2 / 2 LF steps for csa[i] of every i): that case is taken on the texts of at most QUADRATIC_MAX tokens."""
    torch = torch_cuda
    text = TEXTS[name]
    o, sa, qs, want = _case(oracle, name)
    n = len(sa)
    base = V.VlgIndex.build_int(text)
    src = base.compress() if rrr else base
    ref = base.search(qs, workspace=_workspace({}))
    for d in (1, 2, 16, 32, 64) + ((n + 5,) if len(text) <= QUADRATIC_MAX else ()):
        idx = src.resample(text_order=True, dens=d)
        info = idx.info()
        assert info["sampling"] == 1 and info["sa_sample_dens"] == d and info["n_samples"] == (n + d - 1) // d, (d, info)
        assert info["bv_kind"] == (3 if rrr else 2) and info["n"] == n
        to = oracle.IntIndex(text.astype(np.uint64), dens=d, text_order=True)
        marked = idx.marked()
        assert (marked == to.marked()).all() and (marked == (sa % d == 0)).all(), d
        assert (_sa_batch(torch, V, idx, n) == sa).all(), d
        st = np.zeros(4, dtype=np.uint64)
        for q in qs:
            to.search(q, stats=st)
        for opts in ({"sweep_min": SORTED_SWEEP_OFF, "dedup": 0}, {"sweep_min": 1, "sweep_tail": 16, "dedup": 0}, {"sweep_min": 1, "sweep_tail": 4, "trail": 0},
                     {"sweep_min": 1, "sweep_tail": SORTED_SWEEP_OFF}):
            res = idx.search(qs, workspace=_workspace(opts))
            for i in range(len(qs)):
                assert res.tuples(i).tolist() == want[i], (qs[i], d, opts)
            assert res.summary["checksum"] == ref.summary["checksum"] and res.summary["n_matches"] == ref.summary["n_matches"], (d, opts)
            if opts.get("dedup", 1) == 0:
                assert res.summary["located_occurrences"] == int(st[0]), (d, opts)
                assert res.summary["lf_steps"] == int(st[1]) == _located_steps(o, sa, qs, d), (d, opts)
        blob = torch.empty(idx.blob_bytes(), dtype=torch.uint8, device="cuda")
        idx.blob_export(blob.data_ptr(), blob.numel())
        att = V.VlgIndex.attach_blob(blob.data_ptr(), blob.numel(), keep=blob)
        assert att.info() == info
        r2 = att.search(qs, workspace=_workspace({}))
        assert (r2.counts == ref.counts).all() and r2.summary["checksum"] == ref.summary["checksum"], d
        for i in range(len(qs)):
            assert r2.tuples(i).tolist() == want[i], (qs[i], d)


@pytest.mark.parametrize("rrr", [False, True], ids=["plain", "rrr"])
@pytest.mark.parametrize("name", NAMES)
def test_int_sa_order_resample(torch_cuda, V, oracle, name, rrr):
    """SA-order resampling of an integer index gives the index vlg_index_build_int makes at that density; at density 1 the samples are
    the suffix array and locate copies SA intervals (VLG_LOCATE_COPY: no LF step, no partition round) in every locate mode."""
    torch = torch_cuda
    text = TEXTS[name]
    o, sa, qs, want = _case(oracle, name)
    n = len(sa)
    base = V.VlgIndex.build_int(text)
    src = base.compress() if rrr else base
    for d in (1, 8, 64):
        idx = src.resample(text_order=False, dens=d)
        info = idx.info()
        assert info["sampling"] == 0 and info["sa_sample_dens"] == d and info["n_samples"] == (n + d - 1) // d
        assert (_sa_batch(torch, V, idx, n) == sa).all(), d
        built = V.VlgIndex.build_int(text, dens=d)
        ref = built.search(qs, workspace=_workspace({}))
        for opts in ({}, {"sweep_min": 1}, {"sweep_min": 1, "dedup": 0}, {"sweep_min": SORTED_SWEEP_OFF}, {"sweep_min": 1, "trail": 0}):
            ws = _workspace(opts)
            ws.profile(True)
            res = idx.search(qs, workspace=ws)
            for i in range(len(qs)):
                assert res.tuples(i).tolist() == want[i], (qs[i], d, opts)
            assert (res.counts == ref.counts).all() and res.summary["checksum"] == ref.summary["checksum"], (d, opts)
            if d == 1:
                assert res.summary["located_occurrences"] > 0
                assert res.summary["locate_mode"] == V.capi.LOCATE_COPY and res.summary["lf_steps"] == 0, (opts, res.summary)
                assert ws.kernel_stats().get("locate_partition", {"launches": 0})["launches"] == 0, opts


@pytest.mark.parametrize("rrr", [False, True], ids=["plain", "rrr"])
@pytest.mark.parametrize("name", ["survey", "abra", "sparse", "words", "one", "run", "keeper"])
def test_int_isa_samples(V, oracle, name, rrr):
    """isa_sample of csa_wt<wt_int<>> (csa_sampling_strategy.hpp:626-642): out[j] = ISA[j * inv_dens], from an SA-order integer index;
    a text-order one keeps no SA-order samples to walk from and is refused, as for bytes."""
    text = TEXTS[name]
    _, sa, _, _ = _case(oracle, name)
    isa = np.empty_like(sa)
    isa[sa] = np.arange(len(sa))
    base = V.VlgIndex.build_int(text)
    idx = base.compress() if rrr else base
    for inv in (1, 7, 16, 32, 64):
        assert idx.isa_samples(inv).astype(np.int64).tolist() == isa[::inv].tolist(), inv
    to = idx.resample(text_order=True, dens=16)
    _assert_status(V, V.capi.E_UNSUPPORTED, lambda: to.isa_samples(16))


def test_int_sampling_refusals(V):
    """The byte index's rules with the same statuses: only an SA-order source is resampled, a text-order index is not compressed
    (compress first, then resample), an SA-order one has no marks, and the strategy code is checked."""
    base = V.VlgIndex.build_int(TEXTS["words"])
    to = base.resample(text_order=True, dens=16)
    _assert_status(V, V.capi.E_INVALID, lambda: to.resample(text_order=True, dens=8))
    _assert_status(V, V.capi.E_INVALID, lambda: to.resample(text_order=False, dens=8))
    _assert_status(V, V.capi.E_INVALID, lambda: to.compress())
    _assert_status(V, V.capi.E_INVALID, lambda: base.marked())
    h = C.c_void_p()
    _assert_status(V, V.capi.E_INVALID, lambda: V.capi.check(V.lib().vlg_index_resample(base._h, 7, 16, C.byref(h))))
    assert not h.value


def test_int_sampling_moderate_size(torch_cuda, V, oracle):
    """A word-level text of 2^20 tokens, 2 000 queries: text order d = 32 (plain and rrr), SA order d = 1 (resident suffix array) and
    SA order d = 32 give the same counts and checksum; 50 sampled queries match the restated reference (sampled among those whose
    sub-patterns occur at most 20 000 times in all: the CPU oracle locates every occurrence)."""
    rng = np.random.default_rng(7)
    text = (1 + rng.zipf(1.3, 1 << 20) % 3000).astype(np.uint32)
    qs = _queries(text, rng, 2000, kmax=3, mmax=3, gapmax=100)
    base = V.VlgIndex.build_int(text)
    ref = base.search(qs, workspace=_workspace({}))
    assert ref.summary["n_matches"] > 0
    o = oracle.IntIndex(text.astype(np.uint64), dens=32)
    occ = [sum(o.backward_search([int(x) for x in part.split()])[0] for part in re.split(r"\.\{\d+,\d+\}\?", q)) for q in qs]
    pick = [int(i) for i in rng.choice(np.flatnonzero(np.array(occ) <= 20000), 50, replace=False)]
    want = {i: o.search(qs[i]).tolist() for i in pick}
    for idx in (base.resample(text_order=True, dens=32), base.resample(text_order=False, dens=1), base.compress().resample(text_order=True, dens=32)):
        res = idx.search(qs, workspace=_workspace({}))
        assert (res.counts == ref.counts).all() and res.summary["checksum"] == ref.summary["checksum"], idx.info()
        for i in pick:
            assert res.tuples(i).tolist() == want[i], qs[i]


SWEEP_CHUNK = 2048              # elements a workgroup of the sweep's round 0 takes per turn (kSweepChunk)
LIST_STAGE = 256                # lists a turn may span and still keep them in LDS (kListStage)


def _staging_case():
    """A text of 9 800 symbols whose single-symbol lists, laid out in SA order (= symbol order), put every way round 0 looks its lists
    up side by side: 600 symbols four times each (the first turn of 2 048 elements spans 512 lists: walked in the global arrays), ten
    symbols 500 times each (a turn spans a handful of lists: staged in LDS; 500 does not divide 2 048, so lists straddle the turns'
    borders), and 2 400 tokens of twenty symbols no query asks for, so that not every SA index is an element of the batch and walks
    are of every length.  Queries for symbols the text does not hold stand between the others: their (empty) lists are dropped by the
    planner -- vlg_search_batch hands the sweep non-empty lists only -- and their queries must come back empty."""
    rng = np.random.default_rng(5)
    small = np.repeat(np.arange(1, 601, dtype=np.uint32), 4)
    large = np.repeat(np.arange(1001, 1011, dtype=np.uint32), 500)
    filler = rng.integers(5001, 5021, 2400).astype(np.uint32)
    text = rng.permutation(np.concatenate([small, large, filler]))
    asked = list(range(1, 601)) + list(range(1001, 1011))
    absent = [700 + 7 * j for j in range(20)] + [2000, 4000]
    syms = sorted(asked + absent)
    qs = [str(c) for c in syms]
    sizes = np.array([int((text == c).sum()) for c in asked])      # the lists of the sweep, in layout order
    return text, qs, sizes


def test_int_sweep_staging_layout_is_what_the_test_needs():
    """the layout the case above promises, from the text itself: which turns of round 0 are staged, and that lists straddle borders"""
    _, _, sizes = _staging_case()
    off = np.concatenate([[0], np.cumsum(sizes)])
    total = int(off[-1])
    assert total == 7400
    spans = []
    for base in range(0, total, SWEEP_CHUNK):
        end = min(base + SWEEP_CHUNK, total)
        first = int(np.searchsorted(off, base, side="right")) - 1
        last = int(np.searchsorted(off, end - 1, side="right")) - 1
        spans.append(last - first + 1)
    assert spans[0] > LIST_STAGE and max(spans[1:]) <= LIST_STAGE, spans          # one turn walks the global arrays, the others are staged
    straddled = [border for border in range(SWEEP_CHUNK, total, SWEEP_CHUNK) if border not in set(off.tolist())]
    assert len(straddled) >= 2, off                                                # borders that lie inside a list


_STAGING = {}


@pytest.mark.parametrize("trail", [1, 0], ids=["trail", "notrail"])
@pytest.mark.parametrize("rrr", [False, True], ids=["plain", "rrr"])
def test_int_sweep_first_round_staged_lists(V, oracle, rrr, trail):
    """Round 0 of the sorted sweep on the wavelet matrix with its lists staged in LDS and not (sweep_first_kernel, the byte index's
    kernel: VLG_STAGE_LISTS = 0 in the `alternates` variant never stages): every position equals the restated reference's, with the
    sweep run to a few stragglers, to the end, and not at all (the stragglers' kernel alone)."""
    if "case" not in _STAGING:
        text, qs, _ = _staging_case()
        o = oracle.IntIndex(text.astype(np.uint64), dens=32)
        _STAGING["case"] = (text, qs, [o.search(q).tolist() for q in qs])
    text, qs, want = _STAGING["case"]
    assert sum(len(w) for w in want) == 7400 and sum(1 for w in want if not w) == 22
    if rrr not in _STAGING:
        base = V.VlgIndex.build_int(text)
        _STAGING[rrr] = base.compress() if rrr else base
    idx = _STAGING[rrr]
    for tail in (4, 0, SORTED_SWEEP_OFF):
        opts = {"sweep_min": 1, "sweep_tail": tail, "trail": trail}
        res = idx.search(qs, workspace=_workspace(opts))
        assert res.summary["locate_mode"] == V.capi.LOCATE_SWEEP and res.summary["located_occurrences"] == 7400, (opts, res.summary)
        for i in range(len(qs)):
            assert res.tuples(i).tolist() == want[i], (qs[i], opts)
