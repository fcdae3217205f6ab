#!/usr/bin/env python3
"""Text access on the clock (vlg_text_access_create, vlg_extract_batch, vlg_isa_batch): on BASELINE config 3's text (1 GiB English-like,
workload.py) and on the word-level integer text of tools/int_bench.py, at inv_dens 16 and 64:
  - the creation time of the handle (ISA samples computed on the device: n LF steps in all);
  - extract throughput in symbols/s for 10^5 windows of +-64 symbols (around first positions of the C3 search batch; random positions
    on the integer text) and for one whole-text extract;
  - ISA throughput for 10^7 random positions;
  - LF steps per second of each, counted exactly from the ranges and positions, next to the locate walk's of the C3 search batch.
Prints one JSON line per measurement and appends them to the output file.  Development / profiling tool, not the metric.

    python tools/extract_bench.py [out=profiles/r07_extract.jsonl] [steps=5] [n_tokens_log2=27]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import vlg_matching_amd as V
from vlg_matching_amd import workload
from vlg_matching_amd.index import Queries, Workspace

WINDOWS, HALF, ISA_QUERIES = 100000, 64, 10 ** 7


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def clock(fn, steps):
    """median wall time of fn() over `steps` runs after one warm-up (every call ends synchronised)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def extract_lf_steps(b, e, n, d):
    """LF steps of vlg_extract_batch on ranges [b, e]: segment s of a range walks from min((s + 1) d, n) down to max(b, s d)"""
    b, e = b.astype(np.int64), e.astype(np.int64)
    s0, s1 = b // d, e // d
    # first segment: from min((s0 + 1) d, n) to b; every later segment s: from min((s + 1) d, n) to s d
    first_top = np.minimum((s0 + 1) * d, n)
    steps = (first_top - b).sum()
    later = s1 - s0                                             # segments s0 + 1 .. s1
    steps += (later * d).sum()
    # the last block of a range whose last segment reaches the end of the text: its walk starts at n, not (s + 1) d
    cut = (s1 > s0) & ((s1 + 1) * d > n)
    steps -= ((s1 + 1) * d - n)[cut].sum()
    return int(steps)


def isa_lf_steps(p, n, d):
    p = p.astype(np.int64)
    return int((np.minimum((p + d - 1) // d * d, n) - p).sum())


def measure(label, idx, n, sym_bytes, windows, steps, extra):
    lines = []
    rng = np.random.default_rng(7)
    p = rng.integers(0, n, ISA_QUERIES).astype(np.uint64)
    d_p = dev_u64(p)
    d_isa = torch.empty_like(d_p)
    b = np.maximum(windows.astype(np.int64) - HALF, 0).astype(np.uint64)
    e = np.minimum(windows.astype(np.int64) + HALF, n - 1).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(e - b + 1)]).astype(np.uint64)
    d_b, d_e, d_off = dev_u64(b), dev_u64(e), dev_u64(off)
    total_w = int(off[-1])
    d_wout = torch.empty(total_w * sym_bytes, dtype=torch.uint8, device="cuda")
    d_whole = torch.empty(n * sym_bytes, dtype=torch.uint8, device="cuda")
    z, last, zo = dev_u64([0]), dev_u64([n - 1]), dev_u64([0])
    for d in (16, 64):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ta = idx.text_access(d)
        torch.cuda.synchronize()
        t_create = time.perf_counter() - t0
        t_create2, _ = clock(lambda: idx.text_access(d), 2)
        t_win, _ = clock(lambda: ta.extract_device(d_b.data_ptr(), d_e.data_ptr(), d_off.data_ptr(), len(b), total_w, d_wout.data_ptr()), steps)
        t_whole, _ = clock(lambda: ta.extract_device(z.data_ptr(), last.data_ptr(), zo.data_ptr(), 1, n, d_whole.data_ptr()), steps)
        t_isa, _ = clock(lambda: ta.isa_device(d_p.data_ptr(), d_isa.data_ptr(), ISA_QUERIES), steps)
        lf_win, lf_whole, lf_isa = extract_lf_steps(b, e, n, d), extract_lf_steps(np.array([0]), np.array([n - 1]), n, d), isa_lf_steps(p, n, d)
        # spot checks: the samples the handle holds are vlg_index_isa_samples', and csa[ISA[p]] = p
        chk = d_isa[:100000].clone()
        sa = torch.empty_like(chk)
        V.capi.check(V.lib().vlg_sa_batch(idx._h, chk.data_ptr(), sa.data_ptr(), 100000, None))
        torch.cuda.synchronize()
        if not np.array_equal(sa.cpu().numpy().view(np.uint64), p[:100000]):
            raise SystemExit("%s d=%d: csa[isa[p]] != p" % (label, d))
        line = {"tool": "extract_bench", "text": label, "n": n, "inv_dens": d, "symbol_bytes": sym_bytes,
                "create_s": t_create, "create_s_warm": t_create2, "create_lf_steps_per_s": n / t_create2,
                "windows": len(b), "window_symbols": total_w, "windows_ms": t_win * 1e3, "windows_symbols_per_s": total_w / t_win,
                "windows_lf_steps": lf_win, "windows_lf_steps_per_s": lf_win / t_win,
                "whole_ms": t_whole * 1e3, "whole_symbols_per_s": n / t_whole, "whole_lf_steps": lf_whole, "whole_lf_steps_per_s": lf_whole / t_whole,
                "isa_queries": ISA_QUERIES, "isa_ms": t_isa * 1e3, "isa_per_s": ISA_QUERIES / t_isa, "isa_lf_steps": lf_isa,
                "isa_lf_steps_per_s": lf_isa / t_isa, "handle_isa_bytes": ((n - 1) // d + 1) * (4 if n < (1 << 32) else 8)}
        line.update(extra)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del ta
    whole = d_whole[: 4096 * sym_bytes].cpu().numpy()
    return lines, whole


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_extract.jsonl")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lg = int(sys.argv[3]) if len(sys.argv) > 3 else 27
    lines = []
    # ---- C3: the byte index of the benchmark's text, its search batch for the window positions and the locate walk's LF rate ----------
    cfg = workload.config("C3")
    text = workload.gen_text(cfg["kind"], cfg["n"], cfg["seed"])
    d_text = torch.from_numpy(text).cuda()
    idx = V.VlgIndex.build_device(d_text.data_ptr(), len(text))
    del d_text
    q = Queries(workload.gen_queries(text, cfg["nq"], cfg["k"], cfg["m"], cfg["gap"], cfg["qseed"]))
    ws = Workspace(160 << 30)
    ws.set_option("tuples", 0)
    idx.search(q, workspace=ws)
    ws.profile(True)
    r = idx.search(q, workspace=ws)
    torch.cuda.synchronize()
    ks = ws.kernel_stats()
    ws.profile(False)
    s = r.summary
    workload.check_expected("C3", {"n_matches": s["n_matches"], "checksum": s["checksum"], "located_occurrences": s["located_occurrences"]})
    first, _ = r.fetch32()
    del r, ws, q
    torch.cuda.empty_cache()
    pick = np.linspace(0, len(first) - 1, WINDOWS).astype(np.int64)
    windows = first[pick].astype(np.uint64)
    locate_ms = ks.get("locate", {}).get("total_ms", 0.0)         # the LF step kernel of the locate stage (partition and resolve apart)
    extra = {"what": "C3 text (1 GiB English-like, workload.py); windows of +-%d symbols around %d first positions of the C3 search batch, "
                     "evenly spread over its %d matches" % (HALF, WINDOWS, len(first)),
             "c3_locate_mode": s["locate_mode"], "c3_locate_lf_steps": s["lf_steps"], "c3_locate_kernels_ms": locate_ms,
             "c3_locate_lf_steps_per_s": s["lf_steps"] / (locate_ms * 1e-3) if locate_ms > 0 else None,
             "c3_kernels_ms": {k: v["total_ms"] for k, v in ks.items() if v["total_ms"] > 0}}
    ls, head = measure("C3", idx, len(text) + 1, 1, windows, steps, extra)
    if not np.array_equal(head, text[:4096]):
        raise SystemExit("C3: the whole-text extract differs from the text")
    lines += ls
    del idx, first, text
    torch.cuda.empty_cache()
    # ---- the word-level integer text of tools/int_bench.py ----------------------------------------------------------------------------
    n_tok = 1 << lg
    rng = np.random.default_rng(3)
    ranks = np.arange(1, 50001, dtype=np.float64)
    p = (1.0 / ranks) / (1.0 / ranks).sum()
    itext = (rng.choice(50000, n_tok, p=p) + 1).astype(np.uint32)
    iidx = V.VlgIndex.build_int(itext)
    windows = np.random.default_rng(11).integers(0, n_tok + 1, WINDOWS).astype(np.uint64)
    extra = {"what": "word-level integer text of tools/int_bench.py: 2^%d tokens, Zipf(1.0) over 50 000 words (seed 3); windows of +-%d "
                     "symbols around %d random positions" % (lg, HALF, WINDOWS), "levels": iidx.info()["max_code_len"]}
    ls, head = measure("int_words", iidx, n_tok + 1, 4, windows, steps, extra)
    if not np.array_equal(head.view(np.uint32), itext[:4096]):
        raise SystemExit("integer text: the whole-text extract differs from the text")
    lines += ls
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
