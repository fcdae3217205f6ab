"""The compacting round 0 of the sorted sweep (workspace option "sweep_compact", sweep_kernels.hpp: commit_turn).

Round 0 takes its elements in turns of C = VLG_SWEEP_CHUNK; the survivors of a turn go behind the survivors of all earlier turns,
which a look-back over one status word per turn supplies, and only they reach the round's partition.  Every test runs the sweep on
the whole batch (sweep_min = 1) down to a few stragglers, compares "sweep_compact" = 1 with the oracle tuple for tuple and with
"sweep_compact" = 0 on the positions and on the LF-step and tree-level counters, and so shows that no run raised the give-up word:
a search whose look-back gave up fails with VLG_E_INTERNAL ("sweep compaction stalled") instead of returning."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWEEP = {"sweep_min": 1, "sweep_tail": 16}
COUNTERS = ("n_matches", "checksum", "located_occurrences", "lf_steps", "wt_levels_locate")


@pytest.fixture(scope="module")
def V():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import vlg_matching_amd as v
    v.lib()
    return v


@pytest.fixture(scope="module")
def C(V):
    return V.capi.build_constants()["VLG_SWEEP_CHUNK"]


def _search(idx, qs, opts):
    from vlg_matching_amd.index import Workspace
    ws = Workspace()
    for k, v in dict(SWEEP, **opts).items():
        ws.set_option(k, v)
    res = idx.search(qs, workspace=ws)
    return res, ws.kernel_stats()


def _both(V, idx, qs, opts):
    """the batch with the compacting rounds and without: same positions, same counters; -> (compacting result, its stats, the other's)"""
    on, ks_on = _search(idx, qs, dict(opts, sweep_compact=1))
    off, ks_off = _search(idx, qs, dict(opts, sweep_compact=0))
    assert on.summary["locate_mode"] == V.capi.LOCATE_SWEEP and off.summary["locate_mode"] == V.capi.LOCATE_SWEEP
    for k in COUNTERS:
        assert on.summary[k] == off.summary[k], (k, opts)
    for x, y in zip(on.fetch(), off.fetch()):
        assert (x == y).all(), opts
    return on, ks_on, ks_off


def _partition(ks):
    return ks.get("locate_partition", {"launches": 0, "algorithmic_bytes": 0})


def _border_sizes(C):
    return [j * C + d for j in (0, 1, 2, 5) for d in (-1, 0, 1) if j * C + d > 0]


def _dna_with_exactly(m, seed):
    """random text over acgt, 4 m long, in which `a` occurs exactly m times"""
    rng = np.random.default_rng(seed)
    text = rng.choice(np.frombuffer(b"cgt", np.uint8), 4 * m)
    text[rng.choice(4 * m, size=m, replace=False)] = ord("a")
    return text.tobytes()


RUNS = {"shared_trails": {}, "no_trail": {"trail": 0}, "no_dedup": {"dedup": 0}}


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("kind", ["a_run", "dna"])
def test_one_list_ends_on_and_next_to_a_turn_border(V, oracle, C, kind, run):
    """One list of exactly j C + d occurrences, j in {0, 1, 2, 5}, d in {-1, 0, 1}: the last turn of round 0 holds one element, a
    whole turn, or is missing one.  "a" * n searched for `a`: with shared trails every walk ends in round 0 -- on a sample, or one
    step on, on the occurrence in front of it; the one occurrence with nothing in front of it is a straggler -- so no partition is
    launched at all.  Random DNA with exactly as many `a`: walks of every length, survivors and finished elements mixed in every
    row.  no_trail: only sample hits finish, nearly every element survives a round; no_dedup: the walks share nothing either."""
    opts = RUNS[run]
    for m in _border_sizes(C):
        text = b"a" * m if kind == "a_run" else _dna_with_exactly(m, m)
        o = oracle.Index.from_text(text)
        idx = V.VlgIndex.build(text)
        want = o.search("a").tolist()
        assert len(want) == m
        on, ks_on, ks_off = _both(V, idx, ["a"], opts)
        assert on.tuples(0).tolist() == want, (kind, run, m)
        if kind == "a_run" and run == "shared_trails":
            assert _partition(ks_on)["launches"] == 0, (m, ks_on)
        # (some element finishes in round 0 -- a text of m >= 32 occurrences holds a sampled one: where a partition ran at all, the
        # compacting round's was asked to move strictly less)
        if _partition(ks_off)["launches"] > 0:
            assert _partition(ks_on)["algorithmic_bytes"] < _partition(ks_off)["algorithmic_bytes"], (m, ks_on, ks_off)
        else:
            assert _partition(ks_on)["launches"] == 0, (m, ks_on)


def _hole_texts(n):
    """the `periodic` and `ab_run` texts of tests/test_gpu_boundaries.py"""
    rng = np.random.default_rng(5)
    block = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 37).tobytes())
    periodic = bytearray(block * (n // 37 + 1))[:n]
    for p in rng.integers(0, n, n // 500):
        periodic[p] = ord("n")
    return {"ab_run": b"ab" * (n // 2), "periodic": bytes(periodic)}


@pytest.mark.parametrize("name", ["ab_run", "periodic"])
def test_whole_turns_without_a_survivor_beside_full_ones(V, oracle, C, name):
    """Texts of long runs of adjacent occurrences, n >= 8 C: the lists whose elements all stand behind another occurrence finish in
    round 0 as a whole -- turns without a survivor in front, in the middle and at the end of the round -- while the elements of the
    other lists (the noise of `periodic`, its gapped query's sub-patterns) all walk on.  The partition must have been asked to move
    strictly less than with "sweep_compact" = 0."""
    n = max(40000, 8 * C) * (4 if name == "periodic" else 1)
    text = _hole_texts(n)[name]
    qs = {"ab_run": ["ab", "b", "a.{1,1}?a", "ba.{0,4}?b"], "periodic": ["a", "c", "g.{0,40}?t", text[:5].decode()]}[name]
    o = oracle.Index.from_text(text)
    idx = V.VlgIndex.build(text)
    on, ks_on, ks_off = _both(V, idx, qs, {})
    total = 0
    for i, q in enumerate(qs):
        want = o.search(q)
        assert on.tuples(i).tolist() == want.tolist(), q
        total += len(want)
    assert on.summary["located_occurrences"] >= 8 * C
    assert _partition(ks_off)["launches"] > 0
    assert _partition(ks_on)["algorithmic_bytes"] < _partition(ks_off)["algorithmic_bytes"], (ks_on, ks_off)


BIG_N = 16 << 20
_BIG = {}


def _big_case():
    """16 Mi symbols of seeded random DNA; the 4 one-letter and the 16 two-letter queries with their occurrences from the text itself"""
    if not _BIG:
        rng = np.random.default_rng(2025)
        t = rng.choice(np.frombuffer(b"acgt", np.uint8), BIG_N)
        qs, want = [], []
        for a in b"acgt":
            qs.append(chr(a))
            want.append(np.flatnonzero(t == a))
        for a in b"acgt":
            for b in b"acgt":
                qs.append(chr(a) + chr(b))
                want.append(np.flatnonzero((t[:-1] == a) & (t[1:] == b)))
        _BIG.update(text=t, qs=qs, want=want, matches=[_without_overlaps(w, len(q)) for w, q in zip(want, qs)])
    return _BIG["text"], _BIG["qs"], _BIG["want"], _BIG["matches"]


def _without_overlaps(occ, m):
    """the matches among the ascending occurrences of a pattern of m <= 2 letters: taken from the left, a match does not overlap the
    one before it, so of a run of occurrences side by side (`aa` in `aaaa`) every second one is a match"""
    if m == 1 or len(occ) == 0:
        return occ
    starts = np.flatnonzero(np.diff(occ, prepend=occ[0] - 2) != 1)
    run_start = np.repeat(occ[starts], np.diff(np.append(starts, len(occ))))
    return occ[(occ - run_start) % 2 == 0]


@pytest.mark.parametrize("alphabet", ["byte", "int"])
def test_more_turns_than_workgroups(V, C, alphabet):
    """About 3.3 10^7 occurrences: more turns than the capped grid of round 0 has workgroups (8192) at C = 2048, so
    workgroups draw turn after turn while others are still resident with earlier ones, and look-backs reach across windows of 64
    turns.  The device-built index (32-bit SA indices) and an integer-alphabet index of the same text; counts, first positions and
    checksum against "sweep" = 0 (the random-access kernel) and "sweep_compact" = 0.  The oracle here is the text itself: every
    match of every query -- not a sample of them -- against the places where the text holds the query's letters, and the number of
    located occurrences against all of those places."""
    import torch
    t, qs, occ, want = _big_case()
    if alphabet == "byte":
        d_text = torch.from_numpy(t).cuda()
        idx = V.VlgIndex.build_device(d_text.data_ptr(), len(t))
    else:
        sym = np.zeros(256, np.uint32)
        sym[np.frombuffer(b"acgt", np.uint8)] = [1, 2, 3, 4]
        idx = V.VlgIndex.build_int(sym[t])
        qs = [" ".join(str(int(sym[c])) for c in q.encode()) for q in qs]
    total = sum(len(w) for w in occ)
    assert total > 8192 * C or C < 2048
    on, ks_on, ks_off = _both(V, idx, qs, {})
    assert on.summary["located_occurrences"] == total
    plain, _ = _search(idx, qs, {"sweep": 0})
    for k in ("n_matches", "checksum", "located_occurrences"):
        assert on.summary[k] == plain.summary[k], k
    for x, y in zip(on.fetch(), plain.fetch()):
        assert (x == y).all()
    for i, w in enumerate(want):
        got = np.asarray(on.positions(i))
        assert len(got) == len(w) and (np.sort(got) == w).all(), qs[i]
    assert _partition(ks_on)["algorithmic_bytes"] < _partition(ks_off)["algorithmic_bytes"]
