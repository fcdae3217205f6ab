"""Shared helpers for the tests: seeded synthetic texts and brute-force checkers."""
import numpy as np


def dna_text(n, seed, probs=(0.25, 0.25, 0.25, 0.25)):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=probs)].copy()


def skewed_text(n, seed, sigma=40):
    """Zipf-ish byte text over `sigma` printable symbols (deep Huffman tree)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, sigma + 1) ** 1.3
    p /= p.sum()
    return (33 + rng.choice(sigma, size=n, p=p)).astype(np.uint8)


def naive_sa(text_with_sentinel):
    t = bytes(text_with_sentinel)
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.uint64)


def naive_occurrences(text, pat):
    t, p = bytes(text), bytes(pat)
    out, i = [], t.find(p)
    while i >= 0:
        out.append(i)
        i = t.find(p, i + 1)
    return out


def bwt_from_sa(text_with_sentinel, sa):
    t = np.asarray(text_with_sentinel, dtype=np.uint8)
    n = len(t)
    return t[(np.asarray(sa, dtype=np.int64) - 1) % n]


def reference_semantics_join(lists, lo, hi, end_len):
    """Pure-Python restatement of SURVEY Appendix C (small cases only)."""
    k = len(lists)
    p = [0] * k
    out = []
    if any(len(l) == 0 for l in lists):
        return out
    while p[0] < len(lists[0]):
        prev = lists[0][p[0]]
        stop = again = False
        for i in range(1, k):
            while p[i] < len(lists[i]) and lists[i][p[i]] < prev + lo[i - 1]:
                p[i] += 1
            if p[i] == len(lists[i]):
                stop = True
                break
            if lists[i][p[i]] > prev + hi[i - 1]:
                p[i - 1] += 1
                again = True
                break
            prev = lists[i][p[i]]
        if stop:
            break
        if again:
            continue
        out.append([int(lists[i][p[i]]) for i in range(k)])
        end = lists[k - 1][p[k - 1]] + end_len
        while p[0] < len(lists[0]) and lists[0][p[0]] < end:
            p[0] += 1
    return out


I63 = (1 << 63) - 1
ARRAY_KS = (1, 2, 3, 8, 9, 31, 32, 33, 40, 64)


def array_queries(text, seed, n=150, absent=b"\xfe"):
    """Query shapes only vlg_queries_create can express (the parser always adds |s_{i-1}| to a gap, stops at 2^62 and sets end_len to a
    sub-pattern's length): [(sub-patterns, lo[k-1], hi[k-1], end_len)] over sub-patterns of 1..3 symbols cut from `text` -- k from
    ARRAY_KS, a different gap for every sub-pattern: lo = 0 behind an equal sub-pattern, lo below the previous length, lo == hi,
    hi = 2^63 - 1, lo = hi = 2^63 - 1 (no match), end_len in {1, |s_0|, |s_last|, 1000, 2^63 - 1}, and a sub-pattern that does not
    occur in the first, a middle and the last place."""
    rng = np.random.default_rng(seed)
    text = bytes(text)
    out = []
    for qi in range(n):
        k = ARRAY_KS[qi % len(ARRAY_KS)]
        subs, lo, hi = [], [], []
        for i in range(k):
            s = int(rng.integers(0, len(text) - 3))
            sub = text[s:s + (1 if k >= 31 and rng.integers(0, 4) else int(rng.integers(1, 4)))]   # (deep queries: mostly single symbols, so that some match)
            if i:
                kind = int(rng.integers(0, 6 if k < 31 else 5))            # (deep queries keep a chance to match: no exact distances)
                if kind == 0:                                               # the same sub-pattern again, maybe at the same position
                    sub, a, b = subs[-1], 0, int(rng.integers(0, 20))
                elif kind == 1:                                             # overlapping the previous sub-pattern
                    a = int(rng.integers(0, len(subs[-1])))
                    b = a + int(rng.integers(0, 30))
                elif kind == 2:
                    a, b = int(rng.integers(0, 12)), I63
                elif kind in (3, 4):
                    a = int(rng.integers(0, 25))
                    b = a + int(rng.integers(4, 60))
                else:
                    a = b = int(rng.integers(1, 30))
                lo.append(a)
                hi.append(b)
            subs.append(sub)
        special = qi // len(ARRAY_KS) % 8
        if k > 1 and special == 5:
            j = int(rng.integers(0, k - 1))
            lo[j] = hi[j] = I63
        if special == 6:
            subs[(0, k // 2, k - 1)[qi % 3]] = absent
        end_len = (1, len(subs[0]), len(subs[-1]), 1000, I63)[int(rng.integers(0, 5))]
        out.append((subs, lo, hi, end_len))
    return out
