#!/usr/bin/env python3
"""Character classes on the FM-index path (vlg_queries_parse_classes + vlg_search_batch) on a protein-like text:
    python tools/class_bench.py [--n 268435456] [--queries 10000] [--repeat 5]   -> one JSON line
  classes   PROSITE-shaped queries: k sub-patterns of m residues cut out of one place of the text, up to three positions of each widened
            to the residue's physico-chemical group ([LIVM], [FYW], [KRH], [DE], [ST], [NQ], [AG]), gaps x(2,4) x(3) x(8) x(3,5) in turn
  literal   the same batch with every class replaced by one of its members (the text's own residue), through the main path: what the
            class figures stand beside -- other answers, fewer occurrences
Every time is the median of --repeat runs after a warm-up run, with the fastest and the slowest beside it; the kernel classes
("class_search" among them) come from a further profiled run each (vlg_workspace_profile: events around every launch)."""
import argparse
import json
import os
import statistics
import sys
import time

GROUPS = ["LIVM", "FYW", "KRH", "DE", "ST", "NQ", "AG"]
GAPS = [(2, 4), (3, 3), (8, 8), (3, 5)]


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


def make_queries(text, nq, k, m, seed):
    """-> (class regexps, literal regexps): every query is cut out of one place of the text, its sub-patterns at distances the gaps
    allow, so that it has at least that match"""
    import numpy as np
    group_of = {c: g for g in GROUPS for c in g}
    rng = np.random.default_rng(seed)
    span = k * m + sum(g[1] for g in GAPS)
    classes, literal = [], []
    for p in rng.integers(0, len(text) - span, size=nq).tolist():
        cq, lq = "", ""
        for i in range(k):
            if i:
                lo, hi = GAPS[(i - 1) % len(GAPS)]
                p += int(rng.integers(lo, hi + 1))
                cq += ".{%d,%d}?" % (lo, hi)
                lq += ".{%d,%d}?" % (lo, hi)
            s = text[p:p + m].tobytes().decode("latin-1")
            wide = set(rng.choice(m, size=int(rng.integers(1, 4)), replace=False).tolist())
            cq += "".join("[" + group_of[c] + "]" if t in wide and c in group_of else c for t, c in enumerate(s))
            lq += s
            p += m
        classes.append(cq)
        literal.append(lq)
    return classes, literal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--m", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workspace-gb", type=float, default=64.0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import vlg_matching_amd as V
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    text = workload.gen_text("protein", args.n, 4)
    classes, literal = make_queries(text, args.queries, args.k, args.m, 14)
    idx = V.VlgIndex.build(text)
    cap = int(args.workspace_gb * (1 << 30))
    ws = Workspace(cap)
    ws.set_option("tuples", 0)

    def measure(batch):
        t, r = timed(lambda: idx.search(batch, workspace=ws), args.repeat, sync)
        ws.profile(True)
        idx.search(batch, workspace=ws)
        ks = ws.kernel_stats()
        kernels = {k: v["total_ms"] for k, v in ks.items() if v["total_ms"] > 0}
        ws.profile(False)
        s = r.summary
        return dict(t, kernels_ms=kernels, class_search_ms=kernels.get("class_search", 0.0), class_search_launches=ks["class_search"]["launches"],
                    **{k: s[k] for k in ("n_matches", "checksum", "located_occurrences", "logical_occurrences", "lf_steps", "wt_levels_bsearch",
                                         "join_slots", "n_chunks", "locate_mode")}), r

    out = {"text": "protein", "n": args.n, "queries": args.queries, "k": args.k, "m": args.m, "index": idx.info(), "example": classes[0]}
    t0 = time.perf_counter()
    qc = Queries.from_classes(classes)
    out["parse_ms"] = (time.perf_counter() - t0) * 1e3
    out["classes"], r = measure(qc)
    off = r.class_intervals()[0]
    per_sub = (off[1:] - off[:-1]).astype("int64")
    out["classes"].update(intervals=int(off[-1]), intervals_per_subpattern_max=int(per_sub.max()), intervals_per_subpattern_mean=float(per_sub.mean()))
    del r
    out["literal"], _ = measure(Queries(literal))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
