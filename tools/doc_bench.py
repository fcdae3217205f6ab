#!/usr/bin/env python3
"""Document-bounded search (vlg_documents + vlg_queries_set_documents) on the protein workload cut into proteins:
    python tools/doc_bench.py [--n 67108864] [--queries 10000] [--mean-length 350] [--repeat 5] [--out profiles/doc_search_protein.json]
  documents   the class batch of tools/class_bench.py (PROSITE-shaped motifs) with the text cut into documents of random lengths
              around --mean-length: no motif may cross from one protein into the next
  plain       the same batch without documents
Every time is the median of --repeat runs after a warm-up run, with the fastest and the slowest beside it; the kernel classes come
from a further profiled run each (vlg_workspace_profile: events around every launch).  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from class_bench import make_queries, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--m", type=int, default=5)
    ap.add_argument("--mean-length", type=int, default=350)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workspace-gb", type=float, default=64.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import vlg_matching_amd as V
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    text = workload.gen_text("protein", args.n, 4)
    classes, _ = make_queries(text, args.queries, args.k, args.m, 14)
    rng = np.random.default_rng(15)
    lengths = rng.integers(max(args.mean_length // 7, 1), 2 * args.mean_length - args.mean_length // 7, size=2 * args.n // args.mean_length + 16)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    starts = starts[starts < args.n]
    idx = V.VlgIndex.build(text)
    ws = Workspace(int(args.workspace_gb * (1 << 30)))
    ws.set_option("tuples", 0)
    t0 = time.perf_counter()
    docs = V.Documents.from_starts(starts, args.n)
    create_ms = (time.perf_counter() - t0) * 1e3

    def measure(batch):
        t, r = timed(lambda: idx.search(batch, workspace=ws), args.repeat, sync)
        ws.profile(True)
        idx.search(batch, workspace=ws)
        ks = ws.kernel_stats()
        kernels = {k: v["total_ms"] for k, v in ks.items() if v["total_ms"] > 0}
        ws.profile(False)
        s = r.summary
        return dict(t, kernels_ms=kernels, **{k: s[k] for k in ("n_matches", "checksum", "located_occurrences", "logical_occurrences", "join_slots",
                                                               "n_chunks", "filter_survivors", "filter_stream_segments", "filter_bit_segments",
                                                               "filter_range_segments")})

    batch = Queries.from_classes(classes)
    out = {"text": "protein", "n": args.n, "queries": args.queries, "k": args.k, "m": args.m, "documents": int(docs.count()),
           "mean_length": float(args.n / docs.count()), "documents_create_ms": create_ms, "example": classes[0]}
    out["plain"] = measure(batch)
    batch.set_documents(docs)
    out["documents_run"] = measure(batch)
    batch.set_documents(None)
    out["plain_again"] = measure(batch)
    out["step_ratio"] = out["documents_run"]["ms"] / out["plain"]["ms"]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
