#!/usr/bin/env python3
"""Select on the clock (vlg_select_support): time per select against time per rank on the same structure in the same run.
  - 10^7 random bit-selects against 10^7 random vlg_bitvector_rank_batch on a plain bit-vector of 2^32 - 2^16 bits (the stand-alone
    bit-vector's limit is 2^32 - 1), at densities 0.5 and 0.01, select1 and select0; the rrr bit-vector (encoded on the host) at 2^28 bits;
  - 10^7 random (k, c) selects against 10^7 vlg_wt_rank_batch on BASELINE config 3's index, c drawn as the text draws it, and 10^7 psi
    against 10^7 LF, plain and rrr-63;
  - the same on the word-level integer text of tools/int_bench.py;
  - the creation time of every handle and its bytes.
Median of `steps` runs after a warm-up.  Prints one JSON line per measurement and appends them to the output file.  Development /
profiling tool, not the metric.

    python tools/select_bench.py [out=profiles/r11_select.jsonl] [steps=5] [n_tokens_log2=27] [bits_log2=32]"""
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

QUERIES = 10 ** 7


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
    return float(np.median(ts))


def timed_support(src, sample=0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ss = src.select_support(sample)
    torch.cuda.synchronize()
    return ss, time.perf_counter() - t0


def emit(lines, line):
    line = dict({"tool": "select_bench", "queries": QUERIES}, **line)
    print(json.dumps(line), flush=True)
    with open(lines, "a") as f:                                   # (appended at once: a later stage that fails loses nothing)
        f.write(json.dumps(line) + "\n")


def random_words(rng, n_words, density):
    if density == 0.5:
        return rng.integers(0, 2 ** 64, n_words, dtype=np.uint64)

    def ands(k):
        w = rng.integers(0, 2 ** 64, n_words, dtype=np.uint64)
        for _ in range(k - 1):
            w &= rng.integers(0, 2 ** 64, n_words, dtype=np.uint64)
        return w
    return ands(7) | ands(9)                                      # 1/128 + 1/512 - their product: 0.0097


def bench_bits(lines, steps, kind, nbits, density):
    rng = np.random.default_rng(int(density * 1000) + 1)
    words = random_words(rng, nbits // 64, density)
    bv = (V.BitVector if kind == "plain" else V.RrrBitVector)(words, nbits)
    del words
    d_end = dev_u64([nbits])
    bv.rank_device(d_end.data_ptr(), d_end.data_ptr(), 1)
    ones = int(d_end.cpu().numpy().view(np.uint64)[0])
    ss, t_create = timed_support(bv)
    d_pos = dev_u64(rng.integers(0, nbits + 1, QUERIES))
    d_out = torch.empty_like(d_pos)
    t_rank = clock(lambda: bv.rank_device(d_pos.data_ptr(), d_out.data_ptr(), QUERIES), steps)
    for bit, have in ((1, ones), (0, nbits - ones)):
        d_k = dev_u64(1 + rng.integers(0, have, QUERIES))
        t_sel = clock(lambda: ss.bit_select_device(d_k.data_ptr(), d_out.data_ptr(), QUERIES, bit=bit), steps)
        # spot check: rank(select(k)) = k - 1 for the ones, select(k) - rank = k - 1 for the zeros
        d_r = torch.empty_like(d_out)
        bv.rank_device(d_out.data_ptr(), d_r.data_ptr(), 100000)
        torch.cuda.synchronize()
        p, r, k = (t[:100000].cpu().numpy().view(np.uint64) for t in (d_out, d_r, d_k))
        if not np.array_equal(r if bit else p - r, k - 1):
            raise SystemExit("%s bit-vector, density %g: rank(select%d(k)) != k - 1" % (kind, density, bit))
        emit(lines, {"structure": kind + " bit-vector", "nbits": nbits, "density": ones / nbits, "bit": bit, "sample": 512,
                     "select_ms": t_sel * 1e3, "rank_ms": t_rank * 1e3, "select_per_rank": t_sel / t_rank, "select_ns": t_sel / QUERIES * 1e9,
                     "rank_ns": t_rank / QUERIES * 1e9, "create_s": t_create, "support_bytes": ss.hbm_bytes(), "source_bytes": bv.hbm_bytes()})


def bench_index(lines, steps, label, idx, text, is_int, what):
    n = len(text) + 1
    rng = np.random.default_rng(5)
    counts = np.bincount(text)
    c = text[rng.integers(0, len(text), QUERIES)]
    k = (1 + rng.integers(0, 2 ** 62, QUERIES) % counts[c]).astype(np.uint64)
    d_k = dev_u64(k)
    d_c = torch.from_numpy(c.astype(np.uint32).view(np.int32) if is_int else c.astype(np.uint8)).cuda()
    d_i = dev_u64(rng.integers(0, n, QUERIES))
    d_out, d_out2 = torch.empty_like(d_i), torch.empty_like(d_i)
    rank = V.lib().vlg_int_rank_batch if is_int else V.lib().vlg_wt_rank_batch
    for ix, bv in ((idx, "plain"), (idx.compress(), "rrr-63")):
        ss, t_create = timed_support(ix)
        t_rank = clock(lambda: V.capi.check(rank(ix._h, d_i.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), QUERIES, None)), steps)
        t_sel = clock(lambda: ss.select_device(d_k.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), QUERIES), steps)
        V.capi.check(rank(ix._h, d_out.data_ptr(), d_c.data_ptr(), d_out2.data_ptr(), 100000, None))
        torch.cuda.synchronize()
        if not np.array_equal(d_out2[:100000].cpu().numpy().view(np.uint64), k[:100000] - 1):
            raise SystemExit("%s %s: rank(select(k, c), c) != k - 1" % (label, bv))
        t_lf = clock(lambda: ix.lf_device(d_i.data_ptr(), d_out.data_ptr(), QUERIES), steps)
        t_psi = clock(lambda: ss.psi_device(d_i.data_ptr(), d_out.data_ptr(), QUERIES), steps)
        ix.lf_device(d_out.data_ptr(), d_out2.data_ptr(), QUERIES)
        torch.cuda.synchronize()
        if not torch.equal(d_out2, d_i):
            raise SystemExit("%s %s: lf[psi[i]] != i" % (label, bv))
        info = ix.info()
        emit(lines, {"structure": label + " " + bv, "what": what, "n": n, "sigma": info["sigma"], "levels_max": info["max_code_len"], "sample": 512,
                     "select_ms": t_sel * 1e3, "rank_ms": t_rank * 1e3, "select_per_rank": t_sel / t_rank, "select_ns": t_sel / QUERIES * 1e9,
                     "rank_ns": t_rank / QUERIES * 1e9, "psi_ms": t_psi * 1e3, "lf_ms": t_lf * 1e3, "psi_per_lf": t_psi / t_lf,
                     "psi_ns": t_psi / QUERIES * 1e9, "lf_ns": t_lf / QUERIES * 1e9, "create_s": t_create, "support_bytes": ss.hbm_bytes(),
                     "source_bytes": info["hbm_bytes"]})
        del ss, ix


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_select.jsonl")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lg = int(sys.argv[3]) if len(sys.argv) > 3 else 27
    bits_lg = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    lines = out_path
    nbits = (1 << bits_lg) - (1 << 16 if bits_lg >= 32 else 0)
    for density in (0.5, 0.01):
        bench_bits(lines, steps, "plain", nbits, density)
        bench_bits(lines, steps, "rrr", 1 << min(bits_lg, 28), density)
        torch.cuda.empty_cache()
    cfg = workload.config("C3")
    text = workload.gen_text(cfg["kind"], cfg["n"] if lg >= 27 else 1 << (lg + 3), cfg["seed"])
    d_text = torch.from_numpy(text).cuda()
    idx = V.VlgIndex.build_device(d_text.data_ptr(), len(text))
    del d_text
    bench_index(lines, steps, "C3", idx, text, False, "C3 text (English-like, workload.py), %d bytes" % len(text))
    del idx, text
    torch.cuda.empty_cache()
    n_tok = 1 << lg
    rng = np.random.default_rng(3)
    ranks = np.arange(1, 50001, dtype=np.float64)
    p = (1.0 / ranks) / (1.0 / ranks).sum()
    itext = (rng.choice(50000, n_tok, p=p) + 1).astype(np.uint32)
    iidx = V.VlgIndex.build_int(itext)
    bench_index(lines, steps, "int_words", iidx, itext, True,
                "word-level integer text of tools/int_bench.py: 2^%d tokens, Zipf(1.0) over 50 000 words (seed 3)" % lg)


if __name__ == "__main__":
    main()
