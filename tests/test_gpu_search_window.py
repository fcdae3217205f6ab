"""vlg_search_batch on the FM-index inside text windows (vlg_queries_set_windows): query j on the window [B, E) has exactly the matches
of the same query on the stand-alone text text[B:E], with B added to every position.  The yardstick is tests/vlg_brute.py through the
generators and checks of test_gpu_wtsa_window.py (the lazy index's window test); the lazy index itself is a second one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_wtsa_window import U64, _batch, _brute_window, _check, _random_int_queries, _random_queries, _windows_of
from util import array_queries, dna_text

pytestmark = pytest.mark.gpu

FILTER_ALL = {"filter_min": 0, "filter_stream_min": 0}
# workspace options -> the summary fields of which one must be positive (that filter kind ran), or None
OPTION_ROWS = [
    ({}, None),
    ({"filter": 0}, None),
    (dict(FILTER_ALL, filter_pivot=0), ("filter_stream_segments",)),
    (dict(FILTER_ALL, filter_pivot=1), ("filter_bit_segments", "filter_range_segments")),
    (dict(FILTER_ALL, filter_pivot=1, pivot_range_ratio=1, pivot_rungs=2), ("filter_range_segments",)),
    ({"dedup": 0}, None),
    ({"list_sort": 0}, None),
    ({"list_sort": 2}, None),
]
FILTER_ROWS = [r for r in OPTION_ROWS if r[1]]


@pytest.fixture(scope="module")
def V():
    import vlg_matching_amd as v
    v.lib()
    return v


def _workspace(opts, cap=0):
    from vlg_matching_amd.index import Workspace
    ws = Workspace(cap)
    for k, v in opts.items():
        ws.set_option(k, v)
    return ws


TEXTS = ["dna223", "dna224", "dna225", "dna3000", "abab", "ints"]


def _text(name):
    if name.startswith("dna"):
        return dna_text(int(name[3:]), 31).tobytes()
    if name == "abab":
        return b"ab" * 600 + b"aab" * 100
    rng = np.random.default_rng(12)
    vocab = np.array([1, 2, 3, 7, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.uint64)       # (vlg_index_build_int refuses symbol 0)
    return vocab[rng.choice(len(vocab), 1500)].astype(np.uint32)


_cases = {}


def _case(V, name):
    """-> (text, [(make batch, representations, pairs (query, B, E), begin[], end[], expected matches per pair)]): computed once per text"""
    if name in _cases:
        return _cases[name]
    text = _text(name)
    rng = np.random.default_rng(len(text))
    if name == "ints":
        qs, fields = _random_int_queries(text, rng, 60)
        batches = [(lambda reps: V.index.Queries.from_int(reps), qs, fields)]
    else:
        qs = _random_queries(text, rng, 60, mmax=4 if len(text) > 1000 else 3)
        fields = [V.parse_query(q) for q in qs]
        batches = [(lambda reps: V.index.Queries(reps), qs, fields)]
        if name in ("dna3000", "abab"):
            af = [f for f in array_queries(text, 5, n=40) if len(f[0]) <= 9][:16]
            batches.append((lambda reps: _batch(V, reps), af, af))
    out = []
    for make, reps, fields in batches:
        pairs = [(j, B, E) for j, f in enumerate(fields) for (B, E) in _windows_of(text, f, rng, 32 if len(fields) == 60 else 8)]
        begin = np.array([B for _, B, _ in pairs], dtype=np.uint64)
        end = np.array([E for _, _, E in pairs], dtype=np.uint64)
        want = [_brute_window(text, fields[j], B, E) for j, B, E in pairs]
        # not vacuous: more than 1/8 of the pairs have a match, some pair more than 3
        assert sum(1 for w in want if w) > len(want) // 8 and any(len(w) > 3 for w in want)
        out.append((make, [reps[j] for j, _, _ in pairs], pairs, begin, end, want))
    assert sum(len(c[2]) for c in out) > 2000
    _cases[name] = (text, out)
    return _cases[name]


def _build(V, text):
    return V.VlgIndex.build_int(text) if isinstance(text, np.ndarray) else V.VlgIndex.build(text)


def _search_both(idx, batch, want, opts, ran=None):
    """the batch (which carries its windows) with and without tuples under the workspace options; -> the summary with tuples"""
    res = idx.search(batch, workspace=_workspace(opts))
    _check(res, want)
    _check(idx.search(batch, workspace=_workspace(dict(opts, tuples=0))), want, tuples=False)
    if ran:
        assert sum(res.summary[f] for f in ran) > 0, (opts, res.summary)
    return res.summary


@pytest.mark.parametrize("name", TEXTS)
def test_window_edges_against_brute_force(V, name):
    """(a) One batch entry per (query, window) pair -- the whole text, begin == end, a window one symbol shorter than a sub-pattern,
    windows whose begin / end cut through an occurrence of the first / middle / last sub-pattern, E - m + 1 on, before and behind an
    occurrence start, end = 2^64 - 1, begin = the text's length and beyond, random windows: counts, first positions, tuples, n_matches
    and checksum, with and without tuples.  Plain (d = 32), rrr, text-order and d = 1 indexes under the default options; every row of
    workspace options on the plain index, the rows that name a filter kind with the proof that it ran."""
    text, batches = _case(V, name)
    plain = _build(V, text)
    variants = [plain, plain.compress(), plain.resample(text_order=True, dens=7), plain.resample(text_order=False, dens=1)]
    for make, reps, pairs, begin, end, want in batches:
        batch = make(reps)
        batch.set_windows(begin, end)
        full = plain.search(make(reps)).summary
        for idx in variants:
            s = _search_both(idx, batch, want, {})
            # the lists are located whole, the joins consume the cut ones
            assert s["located_occurrences"] == full["located_occurrences"] and s["logical_occurrences"] < full["logical_occurrences"]
        for opts, ran in OPTION_ROWS[1:]:
            _search_both(plain, batch, want, opts, ran)
        # the dense index copies its suffix array: no LF step, windows or not
        assert variants[3].search(batch).summary["lf_steps"] == 0


def test_cuts_at_block_and_rung_borders(V):
    """(b) "ab" stands at 10 i: windows that begin at 10 r and end one or two symbols behind it put rlo and rhi of the list of "ab" on,
    before and behind a block of 64 and a group of the 4-ary ladder (r = 63 .. 65, 127, 128, 255 .. 257), and the elements next to
    a cut list in P are smaller / larger elements of the SAME list -- with every filter kind forced."""
    text = (b"ab" + b"c" * 8) * 700
    qs = ["ab", "ab.{0,8}?cc", "cc.{0,30}?ab.{0,8}?c"]
    fields = [V.parse_query(q) for q in qs]
    rs = [1, 63, 64, 65, 127, 128, 255, 256, 257, 699]
    wins = []
    for r in rs:
        wins += [(10 * r, 10 * r + 1), (10 * r, 10 * r + 2)]                 # "ab" cut in half; exactly "ab"
        wins += [(10 * r, 10 * r + 11), (10 * r, 10 * r + 12), (10 * r - 9, 10 * r + 2), (max(10 * r - 40, 0), 10 * r + 12)]
        wins += [(10 * a, 10 * r + 2) for a in rs if a < r]                  # both borders on the interesting ranks
    wins += [(0, 7000), (0, U64), (1, 7000), (0, 6992), (0, 6991)]
    pairs = [(j, B, E) for j in range(len(qs)) for B, E in wins]
    want = [_brute_window(text, fields[j], B, E) for j, B, E in pairs]
    assert sum(1 for w in want if w) > len(want) // 4 and max(len(w) for w in want) > 600
    assert want[pairs.index((0, 640, 641))] == [] and want[pairs.index((0, 640, 642))] == [[640]]
    batch = V.index.Queries([qs[j] for j, _, _ in pairs])
    batch.set_windows([B for _, B, _ in pairs], [E for _, _, E in pairs])
    idx = V.VlgIndex.build(text)
    for opts, ran in OPTION_ROWS:
        _search_both(idx, batch, want, opts, ran)


def test_several_super_chunks_and_join_chunks(V):
    """(c) 300 queries x 4 windows on 50 000 symbols under a 48 MiB workspace, reserved up front and grown by the plan: more join chunks
    than under the default workspace, the same counts, positions, tuples and checksum.  Windows of a few thousand symbols are checked
    against brute force, whole-text windows against the unwindowed search.  A query of 64 lists of 35 000 elements needs more join
    scratch than the small workspace has -- without a window it is refused -- and is answered on a window of 600 symbols."""
    from vlg_matching_amd.index import Workspace
    text = dna_text(50_000, 7, probs=(0.7, 0.1, 0.1, 0.1)).tobytes()
    n = len(text)
    rng = np.random.default_rng(50)
    qs = _random_queries(text, rng, 300, kmax=4, mmax=4)
    fields = [V.parse_query(q) for q in qs]
    pairs = []
    for j in range(len(qs)):
        for _ in range(3):
            B = int(rng.integers(0, n - 100))
            pairs.append((j, B, B + int(rng.integers(1, 6000))))
        pairs.append((j, 0, U64))
    big = ([b"A"] * 64, [1] * 63, [6] * 63, 1)
    idx = V.VlgIndex.build(text)
    small_cap = 48 << 20
    with pytest.raises(V.VlgError) as err:                                  # the premise: its full lists do not fit
        idx.search(_batch(V, [big, ([b"A"], [], [], 1)]), workspace=Workspace(small_cap))
    assert err.value.status == V.capi.E_WORKSPACE
    all_fields = [fields[j] for j, _, _ in pairs] + [big]
    begin = [B for _, B, _ in pairs] + [20_000]
    end = [E for _, _, E in pairs] + [20_600]
    batch = _batch(V, all_fields)
    batch.set_windows(begin, end)
    ref = idx.search(batch)
    whole = idx.search(_batch(V, fields))
    for i, (j, B, E) in enumerate(pairs):
        if E == U64:
            assert ref.tuples(i).tolist() == whole.tuples(j).tolist()
        elif i % 3 == 0:
            assert ref.tuples(i).tolist() == _brute_window(text, fields[j], B, E), (j, B, E)
    assert ref.tuples(len(pairs)).tolist() == _brute_window(text, big, 20_000, 20_600) and int(ref.counts[len(pairs)]) > 5
    reserved = Workspace(small_cap)
    reserved.set_option("reserve", small_cap)
    for ws in (reserved, Workspace(small_cap)):
        res = idx.search(batch, workspace=ws)
        assert res.summary["n_chunks"] > ref.summary["n_chunks"], (res.summary, ref.summary)
        for k in ("n_matches", "checksum", "n_tuple_values", "logical_occurrences", "located_occurrences"):
            assert res.summary[k] == ref.summary[k], k
        for x, y in zip(res.fetch(), ref.fetch()):
            assert (x == y).all()


def test_no_window_is_the_search_of_before(V):
    """(d) A batch whose windows were removed is a fresh batch, field for field of the summary, and launches no window cut; windows
    (0, n) and (0, 2^64 - 1) return the same arrays, matches, checksum and tuple values."""
    text = dna_text(3000, 31).tobytes()
    n = len(text)
    qs = _random_queries(text, np.random.default_rng(9), 70) + ["\xfe", "A"]
    idx = V.VlgIndex.build(text)
    ws = _workspace({})
    old = idx.search(V.index.Queries(qs), workspace=ws)
    batch = V.index.Queries(qs)
    assert batch.windows() is None
    batch.set_windows(5, 9)
    assert batch.windows() is not None
    batch.set_windows(None, None)
    assert batch.windows() is None
    new = idx.search(batch, workspace=ws)
    assert new.summary == old.summary
    for x, y in zip(new.fetch(), old.fetch()):
        assert x.tolist() == y.tolist()
    assert ws.kernel_stats()["window_cut"]["launches"] == 0
    for b, e in ((0, n), (0, U64), (None, n + 3), (0, None), (np.zeros(len(qs), np.uint64), np.full(len(qs), n, np.uint64))):
        win = idx.search(batch, workspace=ws, begin=b, end=e)
        assert batch.windows() is None                                      # (search(begin=, end=) restores what the batch carried)
        for x, y in zip(win.fetch(), old.fetch()):
            assert x.tolist() == y.tolist()
        for k in ("n_matches", "checksum", "n_tuple_values", "located_occurrences", "lf_steps", "wt_levels_locate", "wt_levels_bsearch", "locate_mode",
                  "logical_occurrences"):
            assert win.summary[k] == old.summary[k], k
    assert ws.kernel_stats()["window_cut"]["launches"] > 0
    batch.set_windows(7, 90)
    idx.search(batch, workspace=ws, begin=0, end=5)
    b, e = batch.windows()
    assert b.tolist() == [7] * len(qs) and e.tolist() == [90] * len(qs)


@pytest.mark.parametrize("name", ["dna3000", "abab", "ints"])
def test_agrees_with_the_lazy_index(V, name):
    """(e) the same text, batch and window arrays through WtsaIndex.search(begin=, end=): equal counts, first positions and tuples"""
    text, batches = _case(V, name)
    idx, lazy = _build(V, text), V.WtsaIndex(text)
    for make, reps, pairs, begin, end, want in batches:
        a = idx.search(make(reps), begin=begin, end=end)
        b = lazy.search(make(reps), begin=begin, end=end)
        for x, y in zip(a.fetch(), b.fetch()):
            assert x.tolist() == y.tolist()
        assert a.summary["n_matches"] == b.summary["n_matches"] > len(pairs) // 8 and a.summary["checksum"] == b.summary["checksum"]


@pytest.mark.parametrize("force", ["1", "2"])
def test_windows_on_64bit_positions(V, monkeypatch, force):
    """(f) VLG_FORCE_POS64 = 1: the pos_t = uint64_t instantiation of the cut and of everything behind it; = 2: 33-bit SA indices inside
    locate, 32-bit positions behind it (the kernels of a text of 2^32 + 1 symbols)"""
    monkeypatch.setenv("VLG_FORCE_POS64", force)
    text, batches = _case(V, "dna3000")
    idx = V.VlgIndex.build(text)
    assert idx.info()["pos_bytes"] == 8
    for make, reps, pairs, begin, end, want in batches:
        batch = make(reps)
        batch.set_windows(begin, end)
        _search_both(idx, batch, want, {})
        for opts, ran in FILTER_ROWS:
            _search_both(idx, batch, want, opts, ran)


def test_refusals_and_round_trips(V):
    """(g) begin > end is refused and keeps the previous windows; get returns what was set; the lazy index refuses a windowed batch; a
    collective search refuses it before anything is launched or exchanged; occurrences / intervals do not see windows."""
    text = dna_text(3000, 31).tobytes()
    idx, lazy = V.VlgIndex.build(text), V.WtsaIndex(text)
    qs = ["AC", "A.{0,5}?C", "GT.{1,9}?T.{0,3}?A"]
    batch = V.index.Queries(qs)
    occ0 = idx.occurrences(batch)[0].tolist()
    nsub = len(occ0)
    l0, r0 = np.zeros(nsub, np.uint64), np.zeros(nsub, np.uint64)
    V.capi.check(V.lib().vlg_queries_intervals(idx._h, batch._h, l0.ctypes.data, r0.ctypes.data, None))
    batch.set_windows([1, 2, 3], [10, U64, 3])
    b, e = batch.windows()
    assert b.tolist() == [1, 2, 3] and e.tolist() == [10, U64, 3]
    with pytest.raises(V.VlgError) as err:
        batch.set_windows([1, 5, 3], [10, 4, 3])
    assert err.value.status == V.capi.E_INVALID
    b, e = batch.windows()
    assert b.tolist() == [1, 2, 3] and e.tolist() == [10, U64, 3]
    batch.set_windows(None, [4, 5, 6])                                       # NULL begin: zeros
    assert [a.tolist() for a in batch.windows()] == [[0, 0, 0], [4, 5, 6]]
    batch.set_windows([4, 5, 6], None)                                       # NULL end: to the end of the text
    assert [a.tolist() for a in batch.windows()] == [[4, 5, 6], [U64] * 3]
    has = C.c_int(-1)
    V.capi.check(V.lib().vlg_queries_get_windows(batch._h, C.byref(has), None, None))
    assert has.value == 1
    with pytest.raises(ValueError):
        batch.set_windows([1, 2], None)
    # the lazy index takes its windows as arrays
    ws = _workspace({})
    h = C.c_void_p()
    assert V.lib().vlg_wtsa_search_batch(lazy._h, batch._h, 0, ws._h, C.byref(h)) == V.capi.E_INVALID and not h.value
    z = np.zeros(3, np.uint64)
    assert V.lib().vlg_wtsa_search_window_batch(lazy._h, batch._h, z.ctypes.data, None, 0, ws._h, C.byref(h)) == V.capi.E_INVALID and not h.value
    # occurrences / intervals answer per sub-pattern
    assert idx.occurrences(batch)[0].tolist() == occ0
    l1, r1 = np.zeros(nsub, np.uint64), np.zeros(nsub, np.uint64)
    V.capi.check(V.lib().vlg_queries_intervals(idx._h, batch._h, l1.ctypes.data, r1.ctypes.data, None))
    assert l1.tolist() == l0.tolist() and r1.tolist() == r0.tolist()
    # a collective search: refused before the first launch, the exchange is never called
    calls = []
    xws = _workspace({})
    xws.set_exchange(2, 0, lambda *a: calls.append(a) or 0)
    before = xws.kernel_stats()
    with pytest.raises(V.VlgError) as err:
        idx.search(batch, workspace=xws)
    assert err.value.status == V.capi.E_UNSUPPORTED and not calls
    assert xws.kernel_stats() == before and all(v["launches"] == 0 for v in before.values())
    # ... and the windowed batch is searched on one rank
    batch.set_windows(100, 2000)
    res = idx.search(batch)
    _check(res, [_brute_window(text, V.parse_query(q), 100, 2000) for q in qs])


def test_cpp_host_search_batch_windows(V, tmp_path):
    """(h) index_fm_gpu::search_batch_windows of host/index_fm_gpu.hpp, compiled against the library: positions equal the program's own
    brute force on every window; a window that begins behind its end throws"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "vlg_matching_amd")
    exe = str(tmp_path / "fm_window_host_check")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "fm_window_host_check.cpp"), "-L", pkg, "-lvlg_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok ")
