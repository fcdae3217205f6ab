"""Plain statements of where a sub-pattern with character classes occurs, and of the class grammar, for checking the parser and
the kernels against.  A class sub-pattern is a list of positions, each a set of bytes; here a position is a 256-entry boolean row
(row[c] = byte c is accepted).  Numpy, `re` and plain Python only."""
import re

import numpy as np


def rows_of(masks):
    """uint8 [m, 32] mask rows of the C interface (bit c of a row = byte c) -> bool [m, 256]"""
    return np.unpackbits(np.asarray(masks, dtype=np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)


def masks_of(rows):
    """bool [m, 256] -> the uint8 [m, 32] mask rows of the C interface"""
    return np.packbits(np.asarray(rows, dtype=bool).reshape(-1, 256), axis=1, bitorder="little")


def row(members):
    r = np.zeros(256, dtype=bool)
    r[list(bytes(members))] = True
    return r


def class_occurrences(text, rows):
    """Every start of a member string of rows[0] x ... x rows[m-1] in `text`, ascending (uint64): one boolean AND per position."""
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8)
    text, rows = np.asarray(text), np.asarray(rows, dtype=bool)
    n, m = len(text), len(rows)
    if m == 0 or m > n:
        return np.zeros(0, np.uint64)
    ok = np.ones(n - m + 1, dtype=bool)
    for t in range(m):
        ok &= rows[t][text[t:n - m + 1 + t]]
    return np.nonzero(ok)[0].astype(np.uint64)


def lookahead(rows):
    """The sub-pattern as a Python bytes regexp (?=[..][..]): a zero-width match at every start, overlapping ones included."""
    parts = []
    for r in np.asarray(rows, dtype=bool):
        parts.append(b"[" + b"".join(b"\\x%02x" % c for c in np.flatnonzero(r)) + b"]")
    return re.compile(b"(?=" + b"".join(parts) + b")", re.S)


def class_occurrences_re(text, rows):
    return np.array([m.start() for m in lookahead(rows).finditer(bytes(text))], dtype=np.uint64)


def distinct_member_strings(text, rows):
    """the member strings of the sub-pattern that occur in text: one SA interval each"""
    text = bytes(text)
    m = len(rows)
    return {text[int(p): int(p) + m] for p in class_occurrences(text, rows)}


class GrammarError(Exception):
    def __init__(self, status, why):
        self.status = status
        super().__init__(why)


E_INVALID, E_PARSE = 1, 4
MAX_SUBPATTERNS = 64


def _number(b):
    """std::stoull: optional blanks, optional sign, digits, anything behind them ignored; None when there is no number"""
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?)([0-9]+)", b)
    if not m or int(m.group(2)) >= 1 << 64:
        return None
    v = int(m.group(2))
    return (-v) % (1 << 64) if m.group(1) == b"-" else v


def parse(regexp):
    """The library dialect with classes, restated: -> (sub-patterns, lo[], hi[], end_len), a sub-pattern being a list of bool[256] rows.
    Raises GrammarError(E_PARSE / E_INVALID).  Read left to right: \\x is the byte x; [ opens a class that the next unescaped ] closes;
    .{ outside a class opens a gap .{a,b}? ; anything else is itself."""
    s = regexp.encode("latin-1") if isinstance(regexp, str) else bytes(regexp)
    subs, cur, gaps = [], [], []
    i = 0
    while i < len(s):
        c = s[i]
        if c == 0x5C:                                                   # backslash
            if i + 1 >= len(s):
                raise GrammarError(E_PARSE, "lone backslash")
            cur.append(row(s[i + 1:i + 2]))
            i += 2
        elif c == 0x5B:                                                 # [
            j = i + 1
            comp = j < len(s) and s[j] == 0x5E
            j += comp
            members, closed = np.zeros(256, dtype=bool), False
            any_member = False
            while j < len(s):
                if s[j] == 0x5D:
                    closed = True
                    j += 1
                    break
                x = s[j]
                if x == 0x5C:
                    if j + 1 >= len(s):
                        raise GrammarError(E_PARSE, "lone backslash")
                    x = s[j + 1]
                    j += 1
                j += 1
                y = x
                if j + 1 < len(s) and s[j] == 0x2D and s[j + 1] != 0x5D:  # x-y; a '-' in front of ] is itself
                    y = s[j + 1]
                    j += 2
                    if y == 0x5C:
                        if j >= len(s):
                            raise GrammarError(E_PARSE, "lone backslash")
                        y = s[j]
                        j += 1
                    if x > y:
                        raise GrammarError(E_PARSE, "range the wrong way round")
                if x == 0:
                    raise GrammarError(E_INVALID, "NUL in a class")
                members[x:y + 1] = True
                any_member = True
            if not closed:
                raise GrammarError(E_PARSE, "unterminated class")
            if not any_member:
                raise GrammarError(E_PARSE, "empty class")
            if comp:
                members = ~members
                members[0] = False
                if not members.any():
                    raise GrammarError(E_INVALID, "complement accepts nothing")
            cur.append(members)
            i = j
        elif c == 0x2E and s[i + 1:i + 2] == b"{":
            if len(subs) + 1 >= MAX_SUBPATTERNS:
                raise GrammarError(E_INVALID, "too many sub-patterns")
            ge = s.find(b"}", i)
            if ge < 0:
                raise GrammarError(E_PARSE, "gap")
            comma = s.find(b",", i, ge + 1)
            a = _number(s[i + 2:comma]) if comma >= 0 else None
            b = _number(s[comma + 1:ge]) if comma >= 0 else None
            if a is None or b is None or a > b:
                raise GrammarError(E_PARSE, "gap")
            if b >= 1 << 62:
                raise GrammarError(E_INVALID, "gap bound too large")
            if s[ge + 1:ge + 2] != b"?":
                raise GrammarError(E_PARSE, "lazy gaps only")
            subs.append(cur)
            cur = []
            gaps.append((a, b))
            i = ge + 2
        else:
            cur.append(row(s[i:i + 1]))
            i += 1
    subs.append(cur)
    if any(not sp for sp in subs):
        raise GrammarError(E_INVALID, "empty sub-pattern")
    lo = [gaps[t][0] + len(subs[t]) for t in range(len(gaps))]
    hi = [gaps[t][1] + len(subs[t]) for t in range(len(gaps))]
    return subs, lo, hi, len(subs[-1])
