"""bench.py's output on CPU.  The stdout line: built from a recorded full-size result (profiles/), it must stay below
bench.LINE_BYTES and still carry the metric, the rooflines and the baselines.  --dump-outputs: a stand-in result (no GPU) goes
through bench.dump_outputs; the files must hold what the result hands a caller, exactly, within the size cap, and the sample drawn
from a long output must be the same from run to run.  The command line: a plain run switches off every region the headline
figure does not need, --full switches them on again, and the --no-* options still leave single ones out of a --full run."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeResult:
    """What SearchResult exposes to bench.dump_outputs: summary + vlg_result_fetch into caller buffers."""

    def __init__(self, counts, first, tuples, checksum):
        self.counts = np.asarray(counts, dtype=np.uint64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        self.first = np.asarray(first, dtype=np.uint64)
        self.tuples = np.asarray(tuples, dtype=np.uint64)
        self.summary = {"n_queries": len(self.counts), "n_matches": len(self.first), "located_occurrences": 7 * len(self.first),
                        "n_tuple_values": len(self.tuples), "checksum": checksum}

    def fetch_into(self, counts_ptr, offsets_ptr, first_ptr, tuples_ptr):
        for a, p in ((self.counts, counts_ptr), (self.offsets, offsets_ptr), (self.first, first_ptr), (self.tuples, tuples_ptr)):
            if p is not None and a.size:
                C.memmove(p, a.ctypes.data, a.nbytes)


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_small_outputs_are_written_whole_and_exactly(tmp_path):
    bench = _bench()
    counts = [2, 0, 1]
    first = [5, (1 << 33) + 3, 17]
    res = _FakeResult(counts, first, [], checksum=(1 << 64) - 5)
    bench.dump_outputs(res, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == ["counts.npy", "first_positions.npy", "offsets.npy", "summary.npy"]
    for n in names:
        assert np.load(tmp_path / n).dtype == np.float64
    assert np.load(tmp_path / "counts.npy").tolist() == counts
    assert np.load(tmp_path / "offsets.npy").tolist() == [0, 2, 2, 3]
    assert np.load(tmp_path / "first_positions.npy").tolist() == first
    s = np.load(tmp_path / "summary.npy").astype(np.uint64)
    assert s[:4].tolist() == [3, 3, 21, 0]
    assert int(s[4]) | (int(s[5]) << 32) == (1 << 64) - 5


def test_long_outputs_are_a_fixed_sample_under_the_cap(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    nq = 3 << 20                                              # every array over its cap
    counts = rng.integers(0, 3, nq)
    first = rng.integers(0, 1 << 32, int(counts.sum()))
    tuples = rng.integers(0, 1 << 32, 2 * len(first))
    res = _FakeResult(counts, first, tuples, checksum=12345)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(res, str(tmp_path / d))
        runs.append({n[:-4]: np.load(tmp_path / d / n) for n in os.listdir(tmp_path / d)})
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    assert sorted(runs[0]) == sorted(runs[1])
    for n in runs[0]:
        assert np.array_equal(runs[0][n], runs[1][n]), n
    for name, full in (("counts", res.counts), ("offsets", res.offsets), ("first_positions", res.first), ("tuples", res.tuples)):
        pick = runs[0][name + "_index"].astype(np.int64)
        assert len(pick) > 0 and np.all(np.diff(pick) > 0) and pick[-1] < full.size
        assert np.array_equal(runs[0][name], full[pick].astype(np.float64)), name


def test_stdout_line_of_a_full_size_result_fits():
    bench = _bench()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r04_bench_C3_default.json")).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > bench.LINE_BYTES                 # the whole object would not fit
    line = json.dumps(bench.compact_line(full))
    assert len(line) < bench.LINE_BYTES and "\n" not in line
    c = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "checksum_rank0", "matches_per_step"):
        assert c[k] == full[k], k
    for k in ("ms_per_step", "frac", "achieved", "peak", "kernel_class"):
        assert c["roofline"][k] == full["roofline"][k] and c["rank_kernel_roofline"][k] == full["rank_kernel_roofline"][k]
    assert c["kernels_ms_per_step"] == full["kernels_ms_per_step"]
    assert c["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert c["cpu_baseline"]["sasearch"]["queries_per_sec"] == full["cpu_baseline"]["sasearch"]["queries_per_sec"]
    for name in ("C2", "C4", "C5"):
        for k in ("ms_per_step", "value", "checksum", "checked_against_expected"):
            assert c["other_configs"][name][k] == full["other_configs"][name][k]


def test_stdout_line_keeps_errors_and_stays_under_the_limit_whatever_comes():
    bench = _bench()
    msg = "RuntimeError: injected " + "x" * 300
    huge = {"metric": "m", "value": 1.0, "strong_scaling": {"error": msg},
            "other_configs": {"C%d" % i: {"ms_per_step": float(i), "note": "y" * 60, "value": 2.0 * i} for i in range(400)}}
    c = json.loads(json.dumps(bench.compact_line(huge)))
    assert len(json.dumps(c)) < bench.LINE_BYTES
    assert c["metric"] == "m" and c["value"] == 1.0 and c["strong_scaling"]["error"] == msg


def test_plain_run_leaves_out_what_the_headline_does_not_need():
    bench = _bench()
    extras = ("no_e2e", "no_dense_sa", "no_cpu_baseline", "no_strong")
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert not plain.full and (plain.steps, plain.warmup, plain.gpus) == (3, 2, 1)
    assert all(getattr(plain, k) for k in extras) and plain.other_configs == ""
    assert bench.parse_args(["--other-configs", "C2", "--dump-outputs", "d"]).other_configs == ""
    full = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2", "--full"])
    assert not any(getattr(full, k) for k in extras) and full.other_configs == "C2,C5,C4"
    some = bench.parse_args(["--full", "--no-e2e", "--other-configs", "C2"])
    assert some.no_e2e and not some.no_dense_sa and not some.no_cpu_baseline and some.other_configs == "C2"
