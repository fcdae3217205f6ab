#!/usr/bin/env python3
"""Text windows on the FM-index path (vlg_queries_set_windows + vlg_search_batch) on a benchmark workload:
    python tools/fm_window_bench.py [--config C3] [--repeat 5]   -> one JSON line
  whole       the batch without windows (what the windowed figures stand beside)
  window      every query of the batch on its own window of 1/1000 of the text at a random place (the windows of
              tools/wtsa_bench.py --window: same seed), all matches inside
  collection  the first 1000 queries x 100 equal slices of the text, one batch entry per (query, slice) pair
Every time is the median of --repeat runs after a warm-up run, with the fastest and the slowest beside it; the kernel classes come
from a further profiled run each (vlg_workspace_profile: events around every launch)."""
import argparse
import json
import os
import statistics
import sys
import time


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workspace-gb", type=float, default=160.0)
    ap.add_argument("--collection-queries", type=int, default=1000)
    ap.add_argument("--slices", type=int, default=100)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import vlg_matching_amd as V
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    cfg = workload.config(args.config, args.scale)
    text = workload.gen_text(cfg["kind"], cfg["n"], cfg["seed"])
    queries = workload.gen_queries(text, cfg["nq"], cfg["k"], cfg["m"], cfg["gap"], cfg["qseed"])
    n, nq = cfg["n"], cfg["nq"]
    idx = V.VlgIndex.build(text)
    cap = int(args.workspace_gb * (1 << 30))
    ws = Workspace(cap)
    ws.set_option("tuples", 0)
    ws.set_option("reserve", cap)

    def measure(batch):
        t, r = timed(lambda: idx.search(batch, workspace=ws), args.repeat, sync)
        ws.profile(True)
        idx.search(batch, workspace=ws)
        classes = {k: v["total_ms"] for k, v in ws.kernel_stats().items() if v["total_ms"] > 0}
        ws.profile(False)
        s = r.summary
        return dict(t, entries=batch.n, kernels_ms=classes, window_cut_ms=classes.get("window_cut", 0.0),
                    **{k: s[k] for k in ("n_matches", "checksum", "located_occurrences", "logical_occurrences", "join_slots", "n_chunks",
                                         "filter_survivors")})

    out = {"config": args.config, "scale": args.scale, "n": n, "queries": nq, "k": cfg["k"], "index": idx.info()}
    q = Queries(queries)
    out["whole"] = measure(q)
    rng = np.random.default_rng(7)
    width = max(n // 1000, 1)
    begin = rng.integers(0, n - width + 1, nq).astype(np.uint64)
    q.set_windows(begin, begin + np.uint64(width))
    out["window"] = dict(measure(q), width=width)
    out["window"]["join_slots_of_whole"] = out["window"]["join_slots"] / max(out["whole"]["join_slots"], 1)
    del q
    cq, sl = min(args.collection_queries, nq), args.slices
    edges = [n * i // sl for i in range(sl + 1)]
    coll = Queries([queries[j] for j in range(cq) for _ in range(sl)])
    coll.set_windows(np.array(edges[:-1] * cq, dtype=np.uint64), np.array(edges[1:] * cq, dtype=np.uint64))
    c = measure(coll)
    c.update(queries=cq, slices=sl, located_of_logical=c["located_occurrences"] / max(c["logical_occurrences"], 1),
             window_cut_share=c["window_cut_ms"] / max(sum(c["kernels_ms"].values()), 1e-9))
    out["collection"] = c
    # the same queries on the whole text, once: what a caller who sorts the matches into documents on the host would run
    out["collection_queries_whole"] = measure(Queries(queries[:cq]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
