"""Plain statements of where a sub-pattern with a mismatch budget occurs (Hamming distance, substitutions only), for checking the
kernels against.  A sub-pattern is a list of positions, each a 256-entry boolean row (row[c] = byte c is accepted) as in
tests/vlg_class_brute.py; a literal sub-pattern has one True per row.  Numpy only."""
import numpy as np


def _text_array(text):
    if isinstance(text, (bytes, bytearray)):
        return np.frombuffer(bytes(text), dtype=np.uint8)
    return np.asarray(text)


def misses(text, rows):
    """per start v with v + m <= n: #{t : text[v + t] not accepted by rows[t]}"""
    text, rows = _text_array(text), np.asarray(rows, dtype=bool).reshape(-1, 256)
    n, m = len(text), len(rows)
    if m == 0 or m > n:
        return np.zeros(0, np.int64)
    miss = np.zeros(n - m + 1, dtype=np.int64)
    for t in range(m):
        miss += ~rows[t][text[t:n - m + 1 + t]]
    return miss


def approx_occurrences(text, rows, k):
    """Every start v of the text where the sub-pattern fits (v + m <= n) with at most k positions not accepted, ascending (uint64)."""
    return np.nonzero(misses(text, rows) <= k)[0].astype(np.uint64)


def frontier_widths(text, rows, k):
    """For each suffix length j = 1 .. m: how many distinct strings of length j occur in the text within k misses of rows[m - j:].
    These are the frontiers of a backward search with the budget, step by step; the last entry is the number of SA intervals the
    sub-pattern has, the largest the "class_intervals" it needs."""
    raw = bytes(_text_array(text).astype(np.uint8))
    rows = np.asarray(rows, dtype=bool).reshape(-1, 256)
    m = len(rows)
    out = []
    for j in range(1, m + 1):
        out.append(len({raw[int(v): int(v) + j] for v in approx_occurrences(raw, rows[m - j:], k)}))
    return out
