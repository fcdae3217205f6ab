#!/usr/bin/env python3
"""Document listing (vlg_result_list_documents) against the path it replaces:
    python tools/doc_list_bench.py [--repeat 5] [--out profiles/doc_listing.json] [--kernel-stats default=CSV --kernel-stats store_ids=CSV]
  dense    2^26 dna symbols, 64 queries of one 4-symbol sub-pattern (more than 10^7 matches), documents of about 1000 symbols
  sparse   the protein workload of tools/doc_bench.py (10 000 PROSITE-shaped motifs, proteins of about 350 residues): few matches
  listing  SearchResult.list_documents + the fetch of df, offsets, docs, counts, first_match
  df       the same with pairs=False and the fetch of df, offsets
  host     what a caller had before: vlg_result_fetch of every first position, np.searchsorted over the starts, run-length encoding
Every time is the median of --repeat runs after a warm-up run, with the fastest and the slowest beside it, and each path's bytes over
PCIe are counted from the shapes.  The scatter pass's two variants (the head's document found again from its position, or read from
4 bytes per match the head pass stored: VLG_DOCLIST_STORE_IDS=1) run in a fresh child process each, one after the other.
--kernel-stats NAME=CSV adds the kernel times of a `rocprofv3 --kernel-trace --stats` run of `--part dense --variant NAME` (a run of its
own) and the share of the HBM peak the head and scatter passes reach on their algorithmic bytes.  One JSON line; --out also writes it."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
HBM_PEAK = 8.0e12              # bytes / s


def runs_on_host(first, off, starts):
    """the yardstick of tests/test_gpu_doc_listing.py: -> (df, docs, counts, first_match)"""
    import numpy as np
    M = len(first)
    doc = np.searchsorted(starts, first, "right") - 1
    head = np.ones(M, bool)
    head[1:] = doc[1:] != doc[:-1]
    o = off[:-1].astype(np.int64)
    head[o[o < M]] = True
    fm = np.flatnonzero(head)
    pair_off = np.searchsorted(fm, off.astype(np.int64), "left")
    q_of = np.searchsorted(pair_off, np.arange(len(fm)), "right") - 1
    end = np.minimum(np.append(fm[1:], M), off.astype(np.int64)[q_of + 1])
    return np.diff(pair_off), doc[fm], end - fm, fm


def part(name, repeat):
    import numpy as np
    import torch
    import vlg_matching_amd as V
    from class_bench import make_queries, timed
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    n = 1 << 26
    rng = np.random.default_rng(15)
    if name == "dense":
        text = workload.gen_text("dna", n, 4)
        batch = Queries(workload.gen_queries(text, 64, 1, 4, (0, 0), 14))
        mean = 1000
    else:
        text = workload.gen_text("protein", n, 4)
        batch = Queries.from_classes(make_queries(text, 10000, 3, 5, 14)[0])
        mean = 350
    lengths = rng.integers(max(mean // 7, 1), 2 * mean - mean // 7, size=2 * n // mean + 16)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    starts = starts[starts < n]
    docs = V.Documents.from_starts(starts, n)
    ws = Workspace(64 << 30)
    ws.set_option("tuples", 0)
    idx = V.VlgIndex.build(text)
    t_search, res = timed(lambda: idx.search(batch, workspace=ws), 2, sync)
    nq, M = res.summary["n_queries"], res.summary["n_matches"]
    counts, off, first = np.zeros(nq, np.uint64), np.zeros(nq + 1, np.uint64), np.zeros(max(M, 1), np.uint64)

    def host():
        res.fetch_into(counts.ctypes.data, off.ctypes.data, first.ctypes.data, None)
        return runs_on_host(first[:M], off, starts)

    def listing():
        l = res.list_documents(docs)
        return l.df, l.docs, l.counts, l.first_match, l.offsets

    def only_df():
        l = res.list_documents(docs, pairs=False)
        return l.df, l.offsets

    def device_only():
        return res.list_documents(docs)

    t_host, want = timed(host, repeat, sync)
    t_list, got = timed(listing, repeat, sync)
    t_df, got_df = timed(only_df, repeat, sync)
    t_dev, _ = timed(device_only, repeat, sync)
    t_fetch, _ = timed(lambda: res.fetch_into(None, None, first.ctypes.data, None), repeat, sync)
    same = all(np.array_equal(a, b) for a, b in zip(want, got[:4])) and np.array_equal(want[0], got_df[0])
    pairs = int(len(got[1]))
    width = idx.info()["pos_bytes"]
    return {"part": name, "n": n, "queries": nq, "matches": M, "documents": int(docs.count()), "pairs": pairs, "position_bytes": width,
            "store_ids": os.environ.get("VLG_DOCLIST_STORE_IDS", "0"), "listing_equals_host": bool(same),
            "search": t_search, "host_fetch_searchsorted_rle": t_host, "host_fetch_alone": t_fetch, "listing_and_fetch": t_list,
            "df_and_fetch": t_df, "listing_on_device_alone": t_dev,
            "pcie_bytes_host_path": M * width, "pcie_bytes_listing": 2 * (nq + 1) * 8 + 16 + pairs * 12, "pcie_bytes_df": 2 * (nq + 1) * 8 + 16,
            "algorithmic_bytes_heads": M * width + M // 8 + (4 * M if os.environ.get("VLG_DOCLIST_STORE_IDS", "0") != "0" else 0),
            "algorithmic_bytes_scatter": M // 8 + pairs * ((4 if os.environ.get("VLG_DOCLIST_STORE_IDS", "0") != "0" else width) + 12)}


def kernel_rows(path):
    """the doc_* kernels of a rocprofv3 kernel-stats csv -> {short name: mean ms per call} (the scan's kernels are rocPRIM's, which the
    search launches too: the file does not tell them apart)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            short = next((k for k in ("doc_heads_kernel", "doc_scatter_kernel", "doc_borders_kernel") if k in name), None)
            if short:
                out[short] = out.get(short, 0.0) + float(row["AverageNs"]) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default=None, help="dense | sparse: run that part in this process and print its JSON line (what the children do)")
    ap.add_argument("--variant", default="default", choices=["default", "store_ids"])
    ap.add_argument("--kernel-stats", action="append", default=[], help="NAME=CSV of a profiled run of --part dense --variant NAME")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    if args.part:
        print(json.dumps(part(args.part, args.repeat)), flush=True)
        return
    out = {"repeat": args.repeat, "hbm_peak_bytes_per_s": HBM_PEAK, "runs": []}
    for variant in ("default", "store_ids"):
        for name in ("dense", "sparse"):
            env = dict(os.environ, VLG_DOCLIST_STORE_IDS="1" if variant == "store_ids" else "0")
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", name, "--variant", variant, "--repeat", str(args.repeat)],
                               env=env, capture_output=True, text=True)
            if p.returncode != 0:                                            # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(p.returncode)
            row = json.loads(p.stdout.strip().splitlines()[-1])
            row["variant"], row["process_seconds"] = variant, time.perf_counter() - t0
            out["runs"].append(row)
            print(json.dumps(row), flush=True)
    for spec in args.kernel_stats:
        variant, path = spec.split("=", 1)
        dense = next(r for r in out["runs"] if r["variant"] == variant and r["part"] == "dense")
        ks = kernel_rows(path)
        dense["kernels_ms"] = ks
        for k, b in (("doc_heads_kernel", "algorithmic_bytes_heads"), ("doc_scatter_kernel", "algorithmic_bytes_scatter")):
            if ks.get(k):
                dense["hbm_fraction_" + k] = dense[b] / (ks[k] * 1e-3) / HBM_PEAK
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
