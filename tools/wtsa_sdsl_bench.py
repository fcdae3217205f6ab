#!/usr/bin/env python3
"""The paper's index on disk, on the clock: vlg_wtsa_build, then vlg_wtsa_save_sdsl (vlg_index<alphabet_tag, wt_int<bit_vector_il<>,
rank_support_il<>>>) and vlg_wtsa_load_sdsl, for C3's 1 GiB text and the word-level integer text of tools/int_bench.py.  One JSON line
per case:
  save_s = the whole of vlg_wtsa_save_sdsl; save_device_ms is vlg_wtsa_il_device alone (m_data of the tree assembled on the device,
           event-timed on the stream, no host synchronisation inside); save_rest_s = save_s - save_device_ms: text packing, the save's
           own conversion and copy back, and the host write
  load_s = load_host_parse_s (vlg_sdsl_wtsa_file_*) + load_device_ms (vlg_wtsa_from_parts: upload, gather, counts, checks)
  conversion_gb_s / copy_gb_s: the same byte count for both -- 2 x the m_data bytes, what a device-to-device copy of the image reads
           and writes -- over save_device_ms and over the event-timed copy of those bytes in the same run (conversion_over_copy)
  same_checksum: a query batch gives the same checksum and counts on the loaded index as on the built one
Development / profiling tool, not the metric.

    python tools/wtsa_sdsl_bench.py [--cases c3,words] [--dir DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _event_ms(fn, reps=3):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def run_case(name, text, queries, tmp):
    import ctypes as C
    import vlg_matching_amd as V
    from vlg_matching_amd import capi
    int_tag = text.dtype != np.uint8
    t0 = time.perf_counter()
    idx = V.WtsaIndex(text)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    info = idx.info()
    n, L = info["n"], info["levels"]
    S = n * L
    words = (S + 64) // 64 + (S + 512) // 512 + 1
    img = torch.empty(words, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(img)
    dev_ms = _event_ms(lambda: idx.il_device(img.data_ptr(), words))       # (asynchronous on the null stream the events are on)
    copy_ms = _event_ms(lambda: dst.copy_(img))
    del img, dst
    torch.cuda.empty_cache()
    path = os.path.join(tmp, name + ".sdsl")
    t0 = time.perf_counter()
    idx.save_sdsl(path)
    t_save = time.perf_counter() - t0
    size = os.path.getsize(path)
    f, P = C.c_void_p(), capi.WtsaParts()
    t0 = time.perf_counter()
    capi.check(capi.lib().vlg_sdsl_wtsa_file_open(path.encode(), 4 if int_tag else 1, C.byref(f)))
    capi.check(capi.lib().vlg_sdsl_wtsa_file_parts(f, C.byref(P)))
    t_parse = time.perf_counter() - t0
    h = C.c_void_p()
    t0 = time.perf_counter()
    capi.check(capi.lib().vlg_wtsa_from_parts(C.byref(P), C.byref(h)))
    t_dev = time.perf_counter() - t0
    capi.lib().vlg_wtsa_destroy(h)
    capi.lib().vlg_sdsl_wtsa_file_close(f)
    t0 = time.perf_counter()
    loaded = V.WtsaIndex.load_sdsl(path, int_tag)
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t0
    os.remove(path)
    a = idx.search(queries, max_matches=10)
    b = loaded.search(queries, max_matches=10)
    same = a.summary["checksum"] == b.summary["checksum"] and bool((a.counts == b.counts).all())
    gb = words * 8 / 1e9
    return {"tool": "wtsa_sdsl_bench", "case": name, "symbols": n - 1, "alphabet": "int" if int_tag else "byte", "levels": L,
            "tree_bits": S, "il_words": words, "file_bytes": size, "build_s": t_build,
            "save_s": t_save, "save_device_ms": dev_ms, "save_rest_s": t_save - dev_ms / 1e3,
            "load_s": t_load, "load_host_parse_s": t_parse, "load_device_ms": t_dev * 1e3,
            "conversion_gb_s": 2 * gb / (dev_ms / 1e3), "copy_gb_s": 2 * gb / (copy_ms / 1e3), "copy_ms": copy_ms,
            "conversion_over_copy": dev_ms / copy_ms, "queries": len(queries), "checksum": int(a.summary["checksum"]), "same_checksum": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,words")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    args = ap.parse_args()
    from vlg_matching_amd import workload
    torch.zeros(1, device="cuda")
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        for case in args.cases.split(","):
            if case == "c3":
                cfg = workload.config("C3", 1.0)
                text = workload.gen_text(cfg["kind"], cfg["n"], cfg["seed"])
                queries = workload.gen_queries(text, 10000, cfg["k"], cfg["m"], cfg["gap"], cfg["qseed"])
            else:                                        # the text of tools/int_bench.py: Zipf(1.0) ids over 50 000 words, 2^27 tokens
                rng = np.random.default_rng(3)
                ranks = np.arange(1, 50001, dtype=np.float64)
                p = (1.0 / ranks) / (1.0 / ranks).sum()
                text = (rng.choice(50000, 1 << 27, p=p) + 1).astype(np.uint32)
                qrng = np.random.default_rng(5)
                queries = []
                for _ in range(10000):
                    s = int(qrng.integers(0, len(text) - 40))
                    queries.append("%d %d .{0,20}? %d" % (text[s], text[s + 1], text[s + 5 + int(qrng.integers(0, 10))]))
            print(json.dumps(run_case(case, text, queries, tmp)), flush=True)
            del text


if __name__ == "__main__":
    main()
