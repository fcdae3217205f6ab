"""The reference's on-disk format of csa_wt<wt_int<>, d, isa_d, sa_order_sa_sampling<>, isa_sampling<>, int_alphabet<>> restated in
Python, independently of the library: a reader that takes a file apart member by member, and a writer that assembles one from given
members (csa_wt.hpp:374-393, wt_int.hpp:708-732, csa_alphabet_strategy.hpp:470-590, sd_vector.hpp:192-230, 404-416,
select_support_mcl.hpp:424-494, rank_support_v.hpp:67-106, rrr_vector.hpp:349-372).  Used by test_int_sdsl_cpu.py and
test_gpu_int_sdsl.py."""
import struct
from math import comb

import numpy as np


def hi(x):
    """bits::hi: index of the highest set bit (0 for 0)"""
    return max(int(x).bit_length() - 1, 0)


def levels_of(largest):
    return hi(max(int(largest), 1)) + 1


def pack(values, width):
    """int_vector words of `values` at `width` bits each"""
    v = np.asarray([int(x) for x in values], dtype=np.uint64)
    if width == 64:
        return v.tobytes()
    bits = ((v[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return bits_to_words(bits).tobytes()


def unpack(raw, count, width):
    w = np.frombuffer(raw, dtype=np.uint64)
    if width == 64:
        return [int(x) for x in w[:count]]
    bits = words_to_bits(w, count * width).reshape(count, width).astype(np.uint64)
    vals = np.zeros(count, dtype=np.uint64)
    for k in range(width):
        vals |= bits[:, k] << np.uint64(k)
    return [int(x) for x in vals]


def bits_to_words(bits):
    b = np.asarray(bits, dtype=np.uint8)
    pad = (-len(b)) % 64
    return np.packbits(np.concatenate([b, np.zeros(pad, np.uint8)]), bitorder="little").view(np.uint64)


def words_to_bits(words, nbits):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8), bitorder="little")[:nbits]


# ---- writer ---------------------------------------------------------------------------------------------------------------------
class Out:
    def __init__(self):
        self.parts = []

    def u64(self, v):
        self.parts.append(struct.pack("<Q", int(v)))

    def u32(self, v):
        self.parts.append(struct.pack("<I", int(v)))

    def u8(self, v):
        self.parts.append(struct.pack("<B", int(v)))

    def int_vector(self, values, width, width_in_stream=True):
        self.u64(len(values) * width)
        if width_in_stream:
            self.u8(width)
        self.parts.append(pack(values, width))

    def bit_vector(self, bits):
        self.u64(len(bits))
        self.parts.append(bits_to_words(bits).tobytes())

    def raw(self, b):
        self.parts.append(bytes(b))

    def data(self):
        return b"".join(self.parts)


def rank_v_blocks(bits):
    """rank_support_v<1>'s m_basic_block (rank_support_v.hpp:67-106), restated"""
    words = bits_to_words(bits)
    nbits = len(bits)
    if nbits == 0:
        return [0, 0]
    cap = (nbits + 63) // 64
    bb = [0] * ((((cap * 64) >> 9) + 1) << 1)
    j, s, second = 0, bin(int(words[0])).count("1"), 0
    i = 1
    while i < cap:
        if not (i & 7):
            j += 2
            bb[j - 1] = second
            bb[j] = bb[j - 2] + s
            second = s = 0
        else:
            second |= s << (63 - 9 * (i & 7))
        s += bin(int(words[i])).count("1")
        i += 1
    if i & 7:
        second |= s << (63 - 9 * (i & 7))
        bb[j + 1] = second
    else:
        j += 2
        bb[j - 1] = second
        bb[j] = bb[j - 2] + s
        bb[j + 1] = 0
    return [v & ((1 << 64) - 1) for v in bb]


def select_mcl(out, bits, ones):
    """a select_support_mcl<b> as init_slow builds it (select_support_mcl.hpp:203-262): long super-blocks keep every position,
    mini ones every 64th offset"""
    pos = np.flatnonzero(np.asarray(bits, dtype=np.uint8) == (1 if ones else 0))
    cnt = len(pos)
    out.u64(cnt)
    if not cnt:
        return
    capacity = ((len(bits) + 63) // 64) * 64
    logn = hi(capacity) + 1
    logn4 = logn ** 4
    sb = (cnt + 4095) // 4096
    starts, payloads, minis = [], [], []
    for s in range(sb):
        p = pos[s * 4096:(s + 1) * 4096].tolist()
        starts.append(p[0])
        diff = p[-1] - p[0]
        if diff > logn4:
            minis.append(False)
            payloads.append((p + [0] * (4096 - len(p)), hi(p[-1]) + 1))
        else:
            minis.append(True)
            payloads.append(([x - p[0] for x in p[::64]] + [0] * (64 - len(p[::64])), hi(diff) + 1))
    out.int_vector(starts, logn)
    out.bit_vector([1 if m else 0 for m in minis] if not all(minis) else [])
    for vals, w in payloads:
        out.int_vector(vals, w)


_BINOM = [[comb(n, k) for k in range(64)] for n in range(64)]
_SPACE = [0 if comb(63, k) == 1 else (comb(63, k)).bit_length() for k in range(64)]


def rrr63(out, bits):
    """rrr_vector<63> (rrr_vector.hpp:349-372): size, block classes (6 bits), offsets, pointer and rank samples per 32 blocks,
    inversion bits (all clear); a block's offset numbers it among the blocks of its class (rrr_helper.hpp:304-320)"""
    n = len(bits)
    nb = (n + 63) // 63                                   # (m_size + t_bs) / t_bs blocks
    b = np.concatenate([np.asarray(bits, np.uint8), np.zeros(nb * 63 - n, np.uint8)])
    classes, offs, ptr, rnk = [], [], [], []
    pos, ones = 0, 0
    for i in range(nb):
        if i % 32 == 0:
            ptr.append(pos)
            rnk.append(ones)
        blk = b[i * 63:(i + 1) * 63]
        k = int(blk.sum())
        classes.append(k)
        nr, kk = 0, k
        for j in range(63):
            if blk[j]:
                nr += _BINOM[62 - j][kk]
                kk -= 1
        offs.append((nr, _SPACE[k]))
        pos += _SPACE[k]
        ones += k
    ptr.append(pos)
    rnk.append(ones)
    out.u64(n)
    out.int_vector(classes, 6)
    acc, at = 0, 0
    for v, w in offs:
        acc |= v << at
        at += w
    out.u64(at)
    nw = (at + 63) // 64
    out.raw(acc.to_bytes(nw * 8, "little") if nw else b"")
    wp = hi(max(pos, 1)) + 1
    out.int_vector(ptr, wp)
    out.int_vector(rnk, hi(max(ones, 1)) + 1)
    out.bit_vector([0] * ((nb + 31) // 32))


def sd_vector(out, symbols):
    """sd_vector<>(bit_vector with ones at `symbols`), sd_vector.hpp:192-230"""
    size, m = int(symbols[-1]) + 1, len(symbols)
    logm, logn = hi(m) + 1, hi(size) + 1
    if logm == logn:
        logm -= 1
    wl = logn - logm
    high = [0] * (m + (1 << logm))
    for j, s in enumerate(symbols):
        high[(int(s) >> wl) + j] = 1
    out.u64(size)
    out.u8(wl)
    out.int_vector([int(s) & ((1 << wl) - 1) for s in symbols], wl)
    out.bit_vector(high)
    select_mcl(out, high, True)
    select_mcl(out, high, False)


def write_file(path, n, tree_bits_2d, C, comp2char, samples, isa, rank_blocks=None, rrr=False, sigma=None, max_level=None):
    """Assemble a csa_wt<wt_int<>> file from members: tree_bits_2d = [levels][n] bits of wt_int::tree"""
    tb = np.asarray(tree_bits_2d, dtype=np.uint8).reshape(-1)
    L = len(tree_bits_2d) if max_level is None else max_level
    sg = len(comp2char) if sigma is None else sigma
    o = Out()
    o.u64(n)
    o.u64(sg)
    if rrr:
        rrr63(o, tb)
    else:
        o.bit_vector(tb)
        o.int_vector(rank_v_blocks(tb) if rank_blocks is None else [int(x) for x in rank_blocks], 64, False)
        select_mcl(o, tb, True)
        select_mcl(o, tb, False)
    o.u32(L)
    w = hi(n) + 1
    o.int_vector(samples, w)
    o.int_vector(isa, w)
    c2c = [int(x) for x in comp2char]
    if c2c[-1] + 1 == len(c2c):
        o.u64(0), o.u8(0), o.u64(0), o.u8(64), o.u64(0), o.u64(0), o.u64(0)
    else:
        sd_vector(o, c2c)
    o.int_vector([int(x) for x in C], w)
    o.u64(len(c2c))
    data = o.data()
    with open(path, "wb") as f:
        f.write(data)
    return data


def members(n, bwt, sa, dens, isa_dens, ref_levels=None):
    """the members of the file of the text with BWT `bwt` (original symbols, sentinel 0) and suffix array `sa`, computed here"""
    bwt = [int(x) for x in bwt]
    syms = sorted(set(bwt))
    L = levels_of(syms[-1])
    cur = list(bwt)
    rows = []
    for lv in range(L):
        bit = L - 1 - lv
        rows.append([(x >> bit) & 1 for x in cur])
        # stable partition inside each node of the top lv bits (wt_int.hpp:221-252) == sort by the top lv + 1 bits
        cur = sorted(cur, key=lambda x: x >> bit)
    counts = {s: 0 for s in syms}
    for x in bwt:
        counts[x] += 1
    C = [0]
    for s in syms:
        C.append(C[-1] + counts[s])
    isa = [0] * ((n - 1) // isa_dens + 1)
    for i, v in enumerate(sa):
        if v % isa_dens == 0:
            isa[v // isa_dens] = i
    return {"tree": np.array(rows, dtype=np.uint8).reshape(L, n), "C": C, "comp2char": syms, "samples": [int(sa[j]) for j in range(0, n, dens)],
            "isa": isa, "levels": L}


# ---- reader ---------------------------------------------------------------------------------------------------------------------
class In:
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, k):
        assert self.p + k <= len(self.d), "truncated"
        r = self.d[self.p:self.p + k]
        self.p += k
        return r

    def u64(self):
        return struct.unpack("<Q", self.take(8))[0]

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def u8(self):
        return self.take(1)[0]

    def int_vector(self, fixed=0):
        bits = self.u64()
        w = fixed or self.u8()
        raw = self.take(((bits + 63) // 64) * 8)
        return bits, w, raw

    def values(self, fixed=0):
        bits, w, raw = self.int_vector(fixed)
        return w, unpack(raw, bits // w if w else 0, w)

    def select_mcl(self):
        cnt = self.u64()
        if not cnt:
            return {"cnt": 0}
        sb = (cnt + 4095) // 4096
        sbw, starts = self.values()
        bits, _, raw = self.int_vector(1)
        mol = words_to_bits(np.frombuffer(raw, np.uint64), bits) if bits else None
        blocks = []
        for i in range(sb):
            w, vals = self.values()
            blocks.append(("long" if mol is not None and not mol[i] else "mini", vals))
        return {"cnt": cnt, "starts": starts, "blocks": blocks, "width": sbw}


def select_at(sel, i):
    """select(i), 1-based, answered by the section alone where it can be: every rank of a long super-block, ranks 64 j + 1 of a mini one"""
    s, off = (i - 1) // 4096, (i - 1) % 4096
    kind, vals = sel["blocks"][s]
    if kind == "long":
        return vals[off]
    assert off % 64 == 0
    return sel["starts"][s] + vals[off // 64]


def read_file(path):
    d = open(path, "rb").read()
    r = In(d)
    f = {"size": r.u64(), "sigma": r.u64()}
    bits, _, raw = r.int_vector(1)
    f["tree_bits"] = bits
    f["tree_words"] = np.frombuffer(raw, np.uint64).copy()
    _, f["rank_blocks"] = r.values(64)
    f["sel1"], f["sel0"] = r.select_mcl(), r.select_mcl()
    f["max_level"] = r.u32()
    f["sa_width"], f["samples"] = r.values()
    f["isa_width"], f["isa"] = r.values()
    sd = {"size": r.u64(), "wl": r.u8()}
    sd["low_width"], sd["low"] = r.values()
    hb, _, hraw = r.int_vector(1)
    sd["high"] = words_to_bits(np.frombuffer(hraw, np.uint64), hb) if hb else np.zeros(0, np.uint8)
    sd["sel1"], sd["sel0"] = r.select_mcl(), r.select_mcl()
    f["m_char"] = sd
    f["C_width"], f["C"] = r.values()
    f["m_sigma"] = r.u64()
    f["unread"] = len(d) - r.p
    if sd["size"] == 0:
        f["comp2char"] = list(range(f["m_sigma"]))
    else:
        ones = np.flatnonzero(sd["high"])
        f["comp2char"] = [((int(p) - j) << sd["wl"]) | sd["low"][j] for j, p in enumerate(ones)]
    return f
