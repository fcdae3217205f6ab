"""The batches of tests/golden/sweep_recorded.json: what they are and what is observed of them.  Shared by tools/sweep_record.py,
which wrote the fixture at the commit it names, and tests/test_gpu_sweep_recorded.py, which replays it.

A case is "<group>/<text>/<options>"; a group needs a process of its own where it sets an environment variable the library reads
(GROUP_ENV).  Queries: the k <= 3 ones of util.array_queries(text, seed, 500) -- 150 per text, sub-patterns of 1..3 symbols, every
kind of gap -- as the batch Queries.from_arrays makes; for the integer-alphabet index the same sub-patterns as decimals in the parser's
dialect (gaps between sub-patterns, as near to the bounds as the dialect can say)."""
import hashlib

import numpy as np

from util import array_queries, dna_text

TEXTS = {"dna3000": lambda: dna_text(3000, 7).tobytes(), "dna50000": lambda: dna_text(50000, 8).tobytes()}
SWEEP = {"sweep_min": 1, "sweep_tail": 16}
OPTIONS = {
    "sweep": SWEEP,
    "no_trail": dict(SWEEP, trail=0),
    "no_compact": dict(SWEEP, sweep_compact=0),
    "stragglers": {"sweep_min": 1, "sweep_tail": 1 << 30},      # no sorted round: the init pass, then the stragglers' kernel
    "tail0": {"sweep_min": 1, "sweep_tail": 0},
}
UNSAMPLE = dict(SWEEP, unsample_pct=1, unsample_min=1, unsample_tail=16)
GROUPS = ("plain", "rrr", "int", "wide", "extra")
GROUP_ENV = {"wide": {"VLG_FORCE_POS64": "2"}}                    # 33-bit SA indices, 32-bit text positions
CLASSES = ("locate", "locate_partition", "locate_resolve", "expand", "sort")


def _batch(text):
    return [b for b in array_queries(text, 100 + len(text), n=500) if len(b[0]) <= 3]


def _int_regexps(batch):
    out = []
    for subs, lo, hi, _ in batch:
        q = " ".join(str(c) for c in subs[0])
        for i in range(1, len(subs)):
            a = max(0, min(lo[i - 1], 1 << 20) - len(subs[i - 1]))
            b = max(a, min(hi[i - 1], 1 << 20) - len(subs[i - 1]))
            q += " .{%d,%d}? " % (a, b) + " ".join(str(c) for c in subs[i])
        out.append(q)
    return out


def _digest(a):
    a = np.ascontiguousarray(a)
    return {"len": int(a.size), "sha256": hashlib.sha256(a.astype("<u8").tobytes()).hexdigest()}


def observe(res, ws):
    """everything a batch leaves behind that is a deterministic function of index, batch and options"""
    counts, offsets, first, tuples = res.fetch()
    ks = ws.kernel_stats()
    return {"summary": dict(res.summary),
            "fetch": {"counts": _digest(counts), "offsets": _digest(offsets), "first": _digest(first), "tuples": _digest(tuples)},
            "kernels": {c: {f: ks[c][f] if c in ks else 0 for f in ("launches", "algorithmic_bytes")} for c in CLASSES}}


def cases(V, group):
    """name -> a function that runs the batch in a fresh workspace and observes it; indexes are built once per text"""
    from vlg_matching_amd.index import Queries, Workspace
    out = {}

    def add(name, idx, q, opts):
        def run():
            ws = Workspace()
            for k, v in opts.items():
                ws.set_option(k, v)
            return observe(idx.search(q, workspace=ws), ws)
        out[name] = run

    for tname, make in TEXTS.items():
        text = make()
        batch = _batch(text)
        if group == "int":
            idx = V.VlgIndex.build_int(np.frombuffer(text, np.uint8).astype(np.uint32))
            q = Queries.from_int(_int_regexps(batch))
        else:
            idx = V.VlgIndex.build(text)
            if group == "rrr":
                idx = idx.compress()
            q = Queries.from_arrays([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], [b[3] for b in batch])
        if group == "extra":
            add("extra/%s/unsample" % tname, idx, q, UNSAMPLE)                                  # K3u
            add("extra/%s/dense" % tname, idx.resample(text_order=False, dens=1), q, SWEEP)     # the copy of the resident suffix array
            continue
        for oname, opts in OPTIONS.items():
            add("%s/%s/%s" % (group, tname, oname), idx, q, opts)
    return out
