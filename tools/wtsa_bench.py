#!/usr/bin/env python3
"""The lazy WT-over-SA search (vlg_wtsa_*) beside the FM-index path on the same workload: build time, the
forward searches, and the search with a cap on the matches per query (what a caller that stops iterating early pays).
    python tools/wtsa_bench.py [--config C2] [--caps 1,10,100,0]   -> one JSON line
Further modes (any of them together: the text and the index are made once), every time the median of --repeat runs after a warm-up
run, with the fastest and the slowest beside it:
    --whole     the whole-text search at every cap (no window).  --tree DIR runs it on another checkout of this project (the parent
                commit, built there): the non-regression comparison of the windowed kernel, in the same session on the same machine
    --window    every query of the batch on its own window of 1/1000 of the text at a random place, beside nothing else; and
                vlg_wtsa_range_report_batch: values per second for ranges of about 10, 10^3 and 10^5 values inside windows of 1 % of the
                text, beside the quantile rate of vlg_wtsa_range_walk_batch
    --paging    the heaviest 100 queries of the batch, their first 4096 matches: pages of 16 continued through next_positions (and
                pages that quadruple what is held -- 16, then 48, 192, ... -- what vlg_iterator_gpu asks for) against searching again
                from position 0 with four times the cap (16, 64, ... 4096: the iterator's rule before it could continue)"""
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
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--caps", default="1,10,100")
    ap.add_argument("--fm", action="store_true", help="also time the FM-index path (all matches) on the same batch")
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--window", action="store_true")
    ap.add_argument("--paging", action="store_true")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--tree", default=None, help="root of another checkout of this project to measure instead of this one")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    t0 = time.perf_counter()
    w = V.WtsaIndex(text)
    sync()
    t_build = time.perf_counter() - t0
    q = Queries(queries)
    ws = Workspace(64 << 30)
    ws.set_option("tuples", 0)
    t0 = time.perf_counter()
    sp, ep = w.ranges(q)
    t_ranges = time.perf_counter() - t0
    n, nq = cfg["n"], cfg["nq"]
    caps = [int(c) for c in args.caps.split(",")]
    out = {"config": args.config, "scale": args.scale, "n": n, "queries": nq, "k": cfg["k"], "wtsa_info": w.info(),
           "tree": args.tree or ".", "build_s": t_build, "forward_search_ms": t_ranges * 1e3,
           "logical_occurrences": int((ep + 1 - sp).sum())}
    modes = args.whole or args.window or args.paging

    def summary(r):
        return {"matches": r.summary["n_matches"], "checksum": r.summary["checksum"]}

    if not modes:
        out["caps"] = {}
        for cap in caps:
            w.search(q, max_matches=cap, workspace=ws)
            t0 = time.perf_counter()
            r = w.search(q, max_matches=cap, workspace=ws)
            sync()
            dt = time.perf_counter() - t0
            out["caps"][str(cap)] = dict(summary(r), ms=dt * 1e3, queries_per_sec=nq / dt)
    if args.whole:
        out["whole_text"] = {}
        for cap in caps:
            t, r = timed(lambda: w.search(q, max_matches=cap, workspace=ws), args.repeat, sync)
            out["whole_text"][str(cap)] = dict(t, **summary(r))
    if args.window:
        rng = np.random.default_rng(7)
        width = max(n // 1000, 1)
        begin = rng.integers(0, n - width + 1, nq).astype(np.uint64)
        end = begin + np.uint64(width)
        out["window"] = {"width": width, "caps": {}}
        for cap in sorted(set(caps + [0])):
            t, r = timed(lambda: w.search(q, max_matches=cap, workspace=ws, begin=begin, end=end), args.repeat, sync)
            out["window"]["caps"][str(cap)] = dict(t, **summary(r))
        # range_report: SA ranges 100 times as long as the wanted count, value windows of 1 % of the text
        nv = n + 1
        rep = {}

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()
        for target, m in ((10, 100000), (1000, 10000), (100000, 100)):
            ln = min(target * 100, nv)
            l = rng.integers(0, nv - ln + 1, m).astype(np.uint64)
            vlb = rng.integers(0, n - n // 100, m).astype(np.uint64)
            d_l, d_n, d_a, d_b = dev(l), dev(np.full(m, ln)), dev(vlb), dev(vlb + np.uint64(n // 100 - 1))
            d_cnt = torch.zeros(m, dtype=torch.int64, device="cuda")
            tc, _ = timed(lambda: w.range_count_device(d_l.data_ptr(), d_n.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_cnt.data_ptr(), m), args.repeat, sync)
            off = np.zeros(m + 1, dtype=np.uint64)
            off[1:] = np.cumsum(d_cnt.cpu().numpy().view(np.uint64))
            total = int(off[m])
            d_off, d_out = dev(off), torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
            tr, _ = timed(lambda: w.range_report_device(d_l.data_ptr(), d_n.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_off.data_ptr(), m, total,
                                                        d_out.data_ptr()), args.repeat, sync)
            # the same number of plain quantile walks on the same ranges (vlg_wtsa_range_walk_batch)
            j = np.repeat(np.arange(m), np.diff(off.astype(np.int64)))
            d_ql, d_qn, d_qx = dev(l[j]), dev(np.full(total, ln)), dev(rng.integers(0, ln, total))
            tq, _ = timed(lambda: w.range_walk_device(d_ql.data_ptr(), d_qn.data_ptr(), d_qx.data_ptr(), True, d_out.data_ptr(), total), args.repeat, sync)
            rep[str(target)] = {"ranges": m, "sa_range_len": ln, "values": total, "count": tc, "report": tr, "values_per_sec": total / (tr["ms"] * 1e-3),
                                "quantile_walks": tq, "quantile_walks_per_sec": total / (tq["ms"] * 1e-3)}
        out["range_report"] = rep
    if args.paging:
        weight = np.add.reduceat((ep + 1 - sp).astype(np.int64), q.subpattern_range()[:-1].astype(np.int64))
        heavy = np.argsort(-weight, kind="stable")[:100]
        hq = Queries([queries[int(i)] for i in heavy])
        m = len(heavy)
        want, page = 4096, 16
        wst = Workspace(8 << 30)                                   # a caller that pages wants the tuples

        def continued(grow):
            """all queries stay in the batch; one that is done gets an empty window (it costs nothing)"""
            at, got, cap, rounds = np.zeros(m, np.uint64), np.zeros(m, np.int64), page, 0
            stop = np.full(m, n, np.uint64)
            while True:
                r = w.search(hq, max_matches=cap, workspace=wst, begin=at, end=stop)
                rounds += 1
                got += r.counts.astype(np.int64)
                nxt = r.next_positions()
                done = (nxt == np.uint64(2 ** 64 - 1)) | (got >= want)
                at = np.where(done, np.uint64(n), nxt)
                if done.all():
                    return int(np.minimum(got, want).sum()), rounds
                if grow > 1:
                    cap = min((grow - 1) * int(got.max()), want)        # the next page makes `grow` times what is held

        def restarted():
            """the rule before: search again from position 0 with four times the cap until enough matches came or all of them"""
            cap, rounds, live, total = page, 0, list(range(m)), 0
            while live:
                r = w.search(Queries([queries[int(heavy[i])] for i in live]), max_matches=cap, workspace=wst)
                rounds += 1
                c = r.counts.astype(np.int64)
                fin = (c < cap) | (c >= want)
                total += int(np.minimum(c[fin], want).sum())
                live = [i for i, f in zip(live, fin) if not f]
                cap *= 4
            return total, rounds
        res = {}
        for name, fn in (("continue_pages_of_16", lambda: continued(1)), ("continue_held_x4", lambda: continued(4)), ("restart_x4", restarted)):
            t, (matches, rounds) = timed(fn, max(args.repeat // 2, 3), sync)
            res[name] = dict(t, matches=matches, searches=rounds)
        out["paging"] = dict(res, queries=m, first_matches=want, heaviest_occurrences=int(weight[heavy[0]]))
    if args.fm:
        idx = V.VlgIndex.build(text)
        idx.search(q, workspace=ws)
        t0 = time.perf_counter()
        r = idx.search(q, workspace=ws)
        sync()
        dt = time.perf_counter() - t0
        out["fm_index_all_matches"] = {"ms": dt * 1e3, "matches": r.summary["n_matches"], "checksum": r.summary["checksum"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
