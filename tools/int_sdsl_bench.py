#!/usr/bin/env python3
"""Integer-alphabet indexes on disk, on the clock: the word-level text of tools/int_bench.py through vlg_index_build_int, then
vlg_index_save_sdsl (csa_wt<wt_int<>, 32, 64, ., ., int_alphabet<>>) and vlg_index_load_sdsl_int.  Prints one JSON line:
  save_s = device_ms (vlg_index_export_int_tree: the compact BWT out of the wavelet matrix, the level steps, the copy back) + host_write_s
  load_s = host_parse_s (vlg_sdsl_int_file_*) + device_ms (vlg_index_from_int_parts: upload, level steps, wavelet matrix)
Development / profiling tool, not the metric.

    python tools/int_sdsl_bench.py [n_tokens_log2=27] [path]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import vlg_matching_amd as V
from vlg_matching_amd.index import read_sdsl_int_file


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 27
    n = 1 << lg
    rng = np.random.default_rng(3)                       # the text of tools/int_bench.py: Zipf(1.0) ids over 50 000 words
    ranks = np.arange(1, 50001, dtype=np.float64)
    p = (1.0 / ranks) / (1.0 / ranks).sum()
    text = (rng.choice(50000, n, p=p) + 1).astype(np.uint32)
    torch.zeros(1, device="cuda")
    t0 = time.perf_counter()
    idx = V.VlgIndex.build_int(text)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    info = idx.info()
    with tempfile.TemporaryDirectory() as tmp:
        path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tmp, "words.sdsl")
        t0 = time.perf_counter()
        levels, _ = idx.int_tree()
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        idx.save_sdsl(path)
        t_save = time.perf_counter() - t0
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        parts = read_sdsl_int_file(path)
        t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        back = V.VlgIndex.from_int_parts(parts)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        del parts
        t0 = time.perf_counter()
        again = V.VlgIndex.load_sdsl_int(path)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
    nb = idx.blob_bytes()
    bufs = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    idx.blob_export(bufs[0].data_ptr(), nb)
    again.blob_export(bufs[1].data_ptr(), nb)
    same = bool(torch.equal(bufs[0], bufs[1])) and back.blob_bytes() == nb
    print(json.dumps({"tool": "int_sdsl_bench", "tokens": n, "n": info["n"], "sigma": info["sigma"], "levels_compact": info["max_code_len"],
                      "levels_original": levels, "file_bytes": size, "tree_bits": info["n"] * levels,
                      "save_s": t_save, "save_device_ms": t_tree * 1e3, "save_host_write_s": t_save - t_tree,
                      "load_s": t_load, "load_host_parse_s": t_parse, "load_device_ms": t_dev * 1e3,
                      "build_int_s": t_build, "loaded_blob_identical": same}))


if __name__ == "__main__":
    main()
