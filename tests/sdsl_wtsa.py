"""The reference's on-disk format of the paper's index, vlg_index<alphabet_tag, wt_int<bit_vector_il<>, rank_support_il<>>>, restated in
Python, independently of the library: vlg_index::serialize (vlg_index.hpp:181-198: m_text, then m_wt), wt_int::serialize
(wt_int.hpp:708-732), bit_vector_il<512>'s constructor and serialize (bit_vector_il.hpp:113-150, 201-213) with init_rank_samples
(:87-104), int_vector<8> / int_vector<0> (int_vector.hpp:584-600).  Used by test_wtsa_sdsl_cpu.py and test_gpu_wtsa_sdsl.py."""
import struct
from collections import deque

import numpy as np

from sdsl_int import bits_to_words, hi, pack


def levels_of_n(n):
    """wt_int over a suffix array of n values: max_level = hi(max(n - 1, 1)) + 1 (wt_int.hpp:194-204)"""
    return hi(max(int(n) - 1, 1)) + 1


def suffix_array(text):
    """suffix array of text + sentinel (the sentinel smaller than every symbol), by sorting suffixes"""
    t = [int(x) for x in text]
    return sorted(range(len(t) + 1), key=lambda i: t[i:] + [-1])


def wt_levels(sa):
    """wt_int's levels over the values `sa` (wt_int.hpp:215-255): level l is the arrangement stably sorted by the top l bits, its bit
    the (L - 1 - l)-th of every value -> list of L uint8 arrays of n bits"""
    v = np.asarray(sa, dtype=np.uint64)
    L = levels_of_n(len(v))
    out = []
    for lvl in range(L):
        order = np.argsort(v >> np.uint64(L - lvl), kind="stable")
        out.append(((v[order] >> np.uint64(L - 1 - lvl)) & np.uint64(1)).astype(np.uint8))
    return out


def shape(n, L):
    S = n * L
    data_words = (S + 64) // 64
    superblocks = (S + 512) // 512
    block_num = data_words + superblocks + 1
    rank_samples = min(1024, 1 << hi(superblocks)) if block_num > 1024 * 64 else 0
    return S, data_words, superblocks, block_num, rank_samples


def il_members(level_bits):
    """bit_vector_il<512> of the concatenated levels: (size, block_num, superblocks, m_data as uint64, m_rank_samples as uint64)"""
    L = len(level_bits)
    n = len(level_bits[0])
    S, data_words, superblocks, block_num, n_rs = shape(n, L)
    bits = np.concatenate([np.asarray(b, dtype=np.uint8) for b in level_bits] + [np.zeros(64, np.uint8)])
    words = bits_to_words(bits)[:data_words]
    words = np.concatenate([words, np.zeros(data_words - len(words), np.uint64)])
    data = np.zeros(block_num, dtype=np.uint64)
    j = 0
    cum = 0
    pops = [bin(int(x)).count("1") for x in words]
    for i in range(data_words):                        # the constructor's loop (bit_vector_il.hpp:131-141)
        if i % 8 == 0:
            data[j] = cum
            j += 1
        data[j] = words[i]
        cum += pops[i]
        j += 1
    data[j] = cum
    assert j + 1 == block_num
    rs = np.zeros(n_rs, dtype=np.uint64)             # init_rank_samples (bit_vector_il.hpp:87-104)
    q = deque([(0, superblocks)])
    idx = 0
    while q:
        lb, rb = q.popleft()
        if idx < n_rs:
            mid = lb + (rb - lb) // 2
            rs[idx] = data[(mid << 3) + mid]
            idx += 1
            q.append((lb, mid))
            q.append((mid + 1, rb))
    return S, block_num, superblocks, data, rs


def text_member(text, int_tag, width):
    """int_vector<8> (byte_alphabet_tag) or int_vector<0> of `width` bits (int_alphabet_tag)"""
    count = len(text)
    if not int_tag:
        raw = bytes(np.asarray(text, dtype=np.uint8).tobytes())
        raw += b"\0" * (-len(raw) % 8)
        return struct.pack("<Q", 8 * count) + raw
    raw = pack(text, width) if count else b""
    return struct.pack("<QB", width * count, width) + raw


def file_bytes(text, level_bits, int_tag=False, width=8, **over):
    """the whole file; `over` replaces header fields (size, sigma, il_size, block_num, superblocks, block_shift, max_level) or the
    arrays (data, rank_samples) -- for the refusal tests"""
    n = len(text) + 1
    S, block_num, superblocks, data, rs = il_members(level_bits)
    f = dict(size=n, sigma=n, il_size=S, block_num=block_num, superblocks=superblocks, block_shift=9, max_level=len(level_bits),
             data=data, rank_samples=rs)
    f.update(over)
    out = text_member(text, int_tag, width)
    out += struct.pack("<QQ", f["size"], f["sigma"])
    out += struct.pack("<QQQQ", f["il_size"], f["block_num"], f["superblocks"], f["block_shift"])
    d = np.asarray(f["data"], dtype=np.uint64)
    out += struct.pack("<Q", 64 * len(d)) + d.tobytes()
    r = np.asarray(f["rank_samples"], dtype=np.uint64)
    out += struct.pack("<Q", 64 * len(r)) + r.tobytes()
    out += struct.pack("<I", f["max_level"])
    return out


def file_of_text(text, int_tag=False, width=8, **over):
    """the file stock sdsl writes for `text` (suffix array by sorting: small texts)"""
    return file_bytes(text, wt_levels(suffix_array(text)), int_tag, width, **over)
