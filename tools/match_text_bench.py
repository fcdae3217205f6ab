#!/usr/bin/env python3
"""Match texts (vlg_result_extract_matches) against the path they replace:
    python tools/match_text_bench.py [--repeat 5] [--out profiles/match_texts.json] [--runs-from JSON --kernel-stats protein=CSV --kernel-stats pcr=CSV]
  protein  the protein workload of tools/doc_bench.py (10 000 PROSITE-shaped class queries of three sub-patterns): few symbols a match
  pcr      the batch of tools/approx_bench.py at budget 2 (10 000 primer pairs, the gap .{100,2000}?): the texts are the amplicons
  device   SearchResult.extract_matches + MatchTexts.fetch (offsets, begin, symbols)
  alone    extract_matches without the fetch: the texts are in HBM
  host     what a caller had before: vlg_result_fetch of first positions and tuples, the ranges in numpy, TextAccess.extract_batch
           (upload of begin / end / offsets, vlg_extract_batch, download of the symbols)
Every time is the median of --repeat runs after a warm-up run, with the fastest and the slowest beside it; every text of the device
path is compared with the host path's; each path's bytes over PCIe are counted from the shapes (not measured: the keys say so), and the LF steps per symbol delivered
from the ranges and the text access's density (a lane walks from the next ISA sample down to its segment's first symbol).  Each part
runs in a fresh child process.  --kernel-stats NAME=CSV adds the kernel times of a `rocprofv3 --kernel-trace --stats` run of
`--part NAME --repeat 2` (a run of its own; --kernel-stats-repeat for another repeat) and the span pass's time per match: its
total time over the extract_matches calls of that run (a result of several pieces takes several launches a call) and the matches.  One JSON line; --out also writes it."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FLANK = 10


def spans_on_host(counts, off, first, tuples, ks, m_last, n_text, flank):
    """the rule of include/vlg_hip.h without documents -> (b, inclusive e) per match"""
    import numpy as np
    c, k = counts.astype(np.int64), ks.astype(np.int64)
    q_of = np.repeat(np.arange(len(k)), c)
    toff = np.concatenate([[0], np.cumsum(c * k)])
    i_in_q = np.arange(len(first)) - off.astype(np.int64)[q_of]
    p0 = first.astype(np.int64)
    pl = tuples.astype(np.int64)[toff[q_of] + i_in_q * k[q_of] + k[q_of] - 1]
    ce = pl + m_last[q_of]
    return np.maximum(p0 - flank, 0).astype(np.uint64), (np.minimum(ce + flank, n_text) - 1).astype(np.uint64)


def part(name, repeat, n, density):
    import numpy as np
    import torch
    import vlg_matching_amd as V
    from class_bench import make_queries, timed
    from vlg_matching_amd import workload
    from vlg_matching_amd.index import Queries, Workspace
    torch.zeros(1, device="cuda")
    sync = torch.cuda.synchronize
    ws = Workspace(64 << 30)
    if name == "protein":
        text = workload.gen_text("protein", n, 4)
        regexps = make_queries(text, 10000, 3, 5, 14)[0]
        batch = Queries.from_classes(regexps)
        m_last = np.array([len(V.parse_class_query(r)[0][-1]) for r in regexps], np.int64)
    else:
        import approx_bench
        text = workload.gen_text("dna", n, 2)
        regexps = approx_bench.make_queries(text, 10000, 16)[0]
        batch = Queries(regexps)
        batch.set_mismatches(2)
        ws.set_option("class_intervals", 4096)
        m_last = np.full(len(regexps), approx_bench.M, np.int64)
    idx = V.VlgIndex.build(text)
    ta = idx.text_access(density)
    t_search, res = timed(lambda: idx.search(batch, workspace=ws), 2, sync)
    nq, M, TV = res.summary["n_queries"], res.summary["n_matches"], res.summary["n_tuple_values"]
    counts, off = np.zeros(nq, np.uint64), np.zeros(nq + 1, np.uint64)
    first, tuples = np.zeros(max(M, 1), np.uint64), np.zeros(max(TV, 1), np.uint64)
    ks = batch.ks

    def host():
        res.fetch_into(counts.ctypes.data, off.ctypes.data, first.ctypes.data, tuples.ctypes.data)
        b, e = spans_on_host(counts, off, first[:M], tuples[:TV], ks, m_last, n, FLANK)
        sym, o = ta.extract_batch(b, e)
        return o, b, sym

    def device():
        return res.extract_matches(batch, ta, flank=FLANK).fetch()

    t_host, want = timed(host, repeat, sync)
    t_dev, got = timed(device, repeat, sync)
    t_alone, mt = timed(lambda: res.extract_matches(batch, ta, flank=FLANK), repeat, sync)
    same = all(np.array_equal(a, b) for a, b in zip(want, got))
    b, e = want[1].astype(np.int64), want[1].astype(np.int64) + np.diff(want[0].astype(np.int64)) - 1
    lf = int((np.minimum((e // density + 1) * density, n + 1) - b).sum())
    symbols = int(want[0][-1])
    width = idx.info()["pos_bytes"]
    return {"part": name, "n": n, "queries": nq, "matches": M, "tuple_values": TV, "symbols": symbols, "symbols_per_match": symbols / max(M, 1),
            "flank": FLANK, "text_access_density": density, "position_bytes": width, "texts_equal_host": bool(same), "search": t_search,
            "host_fetch_ranges_extract_download": t_host, "device_and_fetch": t_dev, "device_alone": t_alone,
            "pcie_bytes_from_shapes_host_path": {"down": (M + TV) * width + symbols, "up": (3 * M + 1) * 8},
            "pcie_bytes_from_shapes_device_path": {"down": (2 * M + 1) * 8 + symbols + 16, "up": (nq + 1) * 8 + nq * 20},
            "lf_steps": lf, "lf_steps_per_symbol": lf / max(symbols, 1)}


def kernel_rows(path):
    """the kernels of the device path in a rocprofv3 kernel-stats csv -> {short name: {calls, total ms}}"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            short = next((k for k in ("match_span_kernel", "extract_kernel", "extract_check_kernel") if k in row["Name"]), None)
            if short:
                r = out.setdefault(short, {"calls": 0, "total_ms": 0.0})
                r["calls"] += int(row["Calls"])
                r["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-protein", type=int, default=1 << 26)
    ap.add_argument("--n-pcr", type=int, default=100 << 20)
    ap.add_argument("--density", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default=None, help="protein | pcr: run that part in this process and print its JSON line (what the children do)")
    ap.add_argument("--kernel-stats", action="append", default=[], help="NAME=CSV of a profiled run of --part NAME")
    ap.add_argument("--kernel-stats-repeat", type=int, default=2, help="the --repeat of the profiled runs")
    ap.add_argument("--runs-from", default=None, help="an earlier --out file: take its runs instead of measuring, add --kernel-stats to them")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    sizes = {"protein": args.n_protein, "pcr": args.n_pcr}
    if args.part:
        print(json.dumps(part(args.part, args.repeat, sizes[args.part], args.density)), flush=True)
        return
    out = {"repeat": args.repeat, "runs": []}
    if args.runs_from:                                                       # (the profiled runs come later than the timed ones)
        out = json.loads(open(args.runs_from).read())
    for name in () if args.runs_from else ("protein", "pcr"):
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", name, "--repeat", str(args.repeat), "--n-protein", str(args.n_protein),
                            "--n-pcr", str(args.n_pcr), "--density", str(args.density)], capture_output=True, text=True)
        if p.returncode != 0:                                                # nothing more is started after a failure
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        row = json.loads(p.stdout.strip().splitlines()[-1])
        row["process_seconds"] = time.perf_counter() - t0
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
    for spec in args.kernel_stats:
        name, path = spec.split("=", 1)
        row = next(r for r in out["runs"] if r["part"] == name)
        row["kernels"] = kernel_rows(path)
        span = row["kernels"].get("match_span_kernel")
        if span and span["calls"]:                                           # (a result of several pieces takes several launches a call)
            calls = 2 * (args.kernel_stats_repeat + 1)                       # extract_matches calls of a --part run: device and alone, warm-up + repeat each
            row["span_pass_launches_per_extract_call"] = span["calls"] / calls
            row["span_pass_ns_per_match"] = span["total_ms"] * 1e6 / calls / max(row["matches"], 1)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
