#!/usr/bin/env python3
"""Mismatch budgets on the FM-index path (vlg_queries_set_mismatches + vlg_search_batch) on DNA, shaped as in-silico PCR:
    python tools/approx_bench.py [--n 104857600] [--queries 10000] [--repeat 5]   -> one JSON line, also written to --out
  queries   primer pairs: two 20-mers cut out of one place of the text 100 .. 2000 apart, 0 .. 2 random substitutions applied to each,
            the gap .{100,2000}?
  budgets   the same batch with the budgets 0, 1 and 2 on every sub-pattern.  Budget 0 is a batch without budgets and goes through the
            main path: the floor the others stand beside (fewer occurrences: a primer with a substitution occurs nowhere, mostly).
"class_intervals" is raised (--class-intervals) so that no query overflows.  Every time is the median of --repeat runs after a warm-up
run, with the fastest and the slowest beside it; the kernel classes ("class_search" among them) come from a further profiled run each
(vlg_workspace_profile: events around every launch), and "class_search_share" is that run's class_search time over that run's own
wall time ("profiled_ms"), not over the median of the unprofiled runs."""
import argparse
import json
import os
import statistics
import sys
import time

M, GAP = 20, (100, 2000)


def timed(fn, repeat, sync):
    fn()
    sync()
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "runs": repeat}, out


def make_queries(text, nq, seed):
    """primer pairs cut out of the text; -> (regexps, substitutions applied per sub-pattern)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    regexps, applied = [], []
    for p in rng.integers(0, len(text) - (2 * M + GAP[1]), size=nq).tolist():
        d = int(rng.integers(GAP[0], GAP[1] + 1))
        primers = []
        for at in (p, p + M + d):
            s = bytearray(text[at:at + M].tobytes())
            ns = int(rng.integers(0, 3))
            for t in rng.choice(M, size=ns, replace=False).tolist():
                s[t] = int(rng.choice([c for c in b"ACGT" if c != s[t]]))
            primers.append(s.decode("latin-1"))
            applied.append(ns)
        regexps.append("%s.{%d,%d}?%s" % (primers[0], GAP[0], GAP[1], primers[1]))
    return regexps, applied


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100 << 20)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--class-intervals", type=int, default=4096)
    ap.add_argument("--workspace-gb", type=float, default=64.0)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "approx_search_dna.json"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import vlg_matching_amd as V
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    text = workload.gen_text("dna", args.n, 2)
    regexps, applied = make_queries(text, args.queries, 16)
    idx = V.VlgIndex.build(text)
    ws = Workspace(int(args.workspace_gb * (1 << 30)))
    ws.set_option("tuples", 0)
    ws.set_option("class_intervals", args.class_intervals)
    q = Queries(regexps)

    def measure(budget):
        q.set_mismatches(budget)
        t, r = timed(lambda: idx.search(q, workspace=ws), args.repeat, sync)
        ws.profile(True)
        t0 = time.perf_counter()
        idx.search(q, workspace=ws)
        sync()
        profiled_ms = (time.perf_counter() - t0) * 1e3
        ks = ws.kernel_stats()
        kernels = {k: v["total_ms"] for k, v in ks.items() if v["total_ms"] > 0}
        ws.profile(False)
        s = r.summary
        out = dict(t, kernels_ms=kernels, class_search_ms=kernels.get("class_search", 0.0), class_search_launches=ks["class_search"]["launches"],
                   profiled_ms=profiled_ms, class_search_share=kernels.get("class_search", 0.0) / profiled_ms,
                   **{k: s[k] for k in ("n_matches", "checksum", "located_occurrences", "logical_occurrences", "lf_steps", "wt_levels_bsearch",
                                        "join_slots", "n_chunks", "locate_mode")})
        if budget:
            off = r.class_intervals()[0]
            per_sub = (off[1:] - off[:-1]).astype("int64")
            out.update(intervals=int(off[-1]), intervals_per_subpattern_max=int(per_sub.max()), intervals_per_subpattern_mean=float(per_sub.mean()))
        return out

    out = {"text": "dna", "n": args.n, "queries": args.queries, "m": M, "gap": list(GAP), "class_intervals": args.class_intervals,
           "substitutions_applied": {str(v): applied.count(v) for v in (0, 1, 2)}, "index": idx.info(), "example": regexps[0]}
    for budget in (0, 1, 2):
        out["budget_%d" % budget] = measure(budget)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
