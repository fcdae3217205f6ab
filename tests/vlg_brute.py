"""A plain statement of what a variable-length-gap search returns, for checking the kernels and the CPU oracle against.

Numpy and plain Python only, Python integers throughout (a position plus a bound near 2^63 does not wrap).  Nothing in here keeps a
pointer per list that only moves forward, as the reference's vlg_iterator, the oracle's merge join and the device kernels all do:
a match is found from its definition, by asking of every candidate, in order, whether a chain of partners leads from it through the
remaining lists."""
from bisect import bisect_left, bisect_right

import numpy as np


def occurrences(text, pat):
    """Every start of `pat` in `text`, ascending (uint64).  text / pat: bytes, or arrays of integer symbols."""
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8)
    if isinstance(pat, (bytes, bytearray)):
        pat = np.frombuffer(bytes(pat), dtype=np.uint8)
    text, pat = np.asarray(text), np.asarray(pat)
    n, m = len(text), len(pat)
    if m == 0 or m > n:
        return np.zeros(0, np.uint64)
    ok = np.ones(n - m + 1, dtype=bool)
    for t in range(m):
        ok &= text[t:n - m + 1 + t] == pat[t]
    return np.nonzero(ok)[0].astype(np.uint64)


def lazy_matches(lists, lo, hi, end_len, cap=None):
    """lists: k ascending position lists; lo / hi: k - 1 start-to-start bounds; -> the matches, a list of k-tuples (lists of ints).

    Match m is the lexicographically least tuple (x_0 .. x_{k-1}) with x_i in lists[i], lo[i-1] <= x_i - x_{i-1} <= hi[i-1] and
    x_0 >= restart, where restart is 0 at first and x_{k-1} + end_len of the match before.  An empty list means no match.  At most
    `cap` matches are returned.

    Feasibility is decided for all candidates at once: an element of list i is LIVE when i is the last list or a live element of
    list i + 1 lies inside its window -- one sweep over the lists per query.  A match is then the least live x_0 >= restart followed,
    list by list, by the least live element inside the window of the one before.  (lazy_matches_by_sweeps below asks the same of
    every candidate separately; it is what this one is pinned against, and too slow for batches of deep queries.)"""
    k = len(lists)
    L = [[int(v) for v in l] for l in lists]
    lo, hi, end_len = [int(v) for v in lo], [int(v) for v in hi], int(end_len)
    assert len(lo) == k - 1 and len(hi) == k - 1 and end_len >= 1
    if k == 0 or any(not l for l in L):
        return []
    live = [None] * (k - 1) + [L[k - 1]]
    for i in range(k - 2, -1, -1):
        nxt, live[i] = live[i + 1], []
        for x in L[i]:
            p = bisect_left(nxt, x + lo[i])
            if p < len(nxt) and nxt[p] <= x + hi[i]:
                live[i].append(x)
    out, restart = [], 0
    while cap is None or len(out) < cap:
        p = bisect_left(live[0], restart)
        if p == len(live[0]):
            break
        tup = [live[0][p]]
        for i in range(1, k):
            x = live[i][bisect_left(live[i], tup[-1] + lo[i - 1])]      # (there is one: tup[-1] is live)
            assert x <= tup[-1] + hi[i - 1]
            tup.append(x)
        out.append(tup)
        restart = tup[-1] + end_len
    return out


def lazy_matches_by_sweeps(lists, lo, hi, end_len, cap=None):
    """The same definition taken candidate by candidate: for each x_0 >= restart in order, a forward sweep over the lists -- which
    elements of list 1 can follow it, which of list 2 can follow those, ... -- says whether a tuple starts there; the tuple is then
    completed the same way, every x_i the least element of its window from which the sweep still reaches the last list."""
    k = len(lists)
    L = [[int(v) for v in l] for l in lists]
    lo, hi, end_len = [int(v) for v in lo], [int(v) for v in hi], int(end_len)
    assert len(lo) == k - 1 and len(hi) == k - 1 and end_len >= 1
    if k == 0 or any(not l for l in L):
        return []
    # Element j of list i is a "break" for the step to list i + 1 when the window of element j + 1 neither overlaps nor touches its
    # own: between two breaks the windows [x + lo, x + hi] of neighbouring elements join up, so a whole run of elements reaches one
    # interval of positions.  (Only there to sweep a run at once instead of element by element.)
    breaks = [[j for j in range(len(L[i]) - 1) if L[i][j + 1] - L[i][j] > hi[i] - lo[i] + 1] for i in range(k - 1)]

    def step(i, runs):
        """runs: index intervals [a, b) of list i -> the index intervals of list i + 1 that hold a partner of one of those elements"""
        src, dst, out = L[i], L[i + 1], []
        for a, b in runs:
            cuts = breaks[i][bisect_left(breaks[i], a): bisect_left(breaks[i], b - 1)]
            for s, e in zip([a] + [c + 1 for c in cuts], [c + 1 for c in cuts] + [b]):
                p, q = bisect_left(dst, src[s] + lo[i]), bisect_right(dst, src[e - 1] + hi[i])
                if p < q:
                    if out and out[-1][1] >= p:
                        out[-1] = (out[-1][0], max(out[-1][1], q))
                    else:
                        out.append((p, q))
        return out

    verdict = {}

    def feasible(i, j):
        """does a chain of partners lead from element j of list i through every later list?  (a forward sweep over the lists)"""
        if (i, j) not in verdict:
            runs = [(j, j + 1)]
            for t in range(i, k - 1):
                runs = step(t, runs)
                if not runs:
                    break
            verdict[(i, j)] = bool(runs)
        return verdict[(i, j)]

    def first_feasible(i, a, b):
        """the least feasible element of list i inside [a, b], or None"""
        for j in range(bisect_left(L[i], a), bisect_right(L[i], b)):
            if feasible(i, j):
                return L[i][j]
        return None

    out, restart = [], 0
    while cap is None or len(out) < cap:
        x = first_feasible(0, restart, L[0][-1])                    # every candidate x_0 >= restart, in order
        if x is None:
            break
        tup = [x]
        for i in range(1, k):                                        # the least tuple: every x_i the least that can still be completed
            x = first_feasible(i, x + lo[i - 1], x + hi[i - 1])
            assert x is not None
            tup.append(x)
        out.append(tup)
        restart = tup[-1] + end_len
    return out
