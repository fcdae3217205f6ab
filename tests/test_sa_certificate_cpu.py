"""The suffix-array certificate (tests/sa_certificate.py) that the full-size GPU tests rest on, checked on the CPU: it accepts the
oracle's suffix arrays and rejects every corruption that a faulty sorter could produce; the BWT, alphabet, sample and rank checks
built on it agree with the oracle's index."""
import numpy as np
import pytest
import torch

from sa_certificate import RankCounter, bwt_from_sa, certify_suffix_array, check_byte_parts, rank_probe_positions
from util import dna_text


def _sa(oracle, text):
    return torch.from_numpy(oracle.suffix_array(np.concatenate([text, [0]]).astype(np.uint8)).view(np.int64))


def _int_sa(text):
    """suffix array of an integer text + sentinel (smaller than every symbol), by plain sorting (small texts only)"""
    t = [int(x) for x in text] + [-1]
    return torch.tensor(sorted(range(len(t)), key=lambda i: t[i:]), dtype=torch.int64)


def _fib(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


BYTE_TEXTS = {
    "dna": lambda: dna_text(5000, 3),
    "periodic": lambda: np.frombuffer(b"abcabcabd" * 300, np.uint8),
    "single": lambda: np.frombuffer(b"a" * 777, np.uint8),
    "one": lambda: np.frombuffer(b"z", np.uint8),
    "fibonacci": lambda: np.frombuffer(_fib(3000), np.uint8),
    "high_bytes": lambda: np.frombuffer(b"\xff" * 300 + b"\x01" + b"\x80\xff" * 50, np.uint8),
}


@pytest.mark.parametrize("name", list(BYTE_TEXTS))
def test_accepts_oracle_suffix_arrays(oracle, name):
    text = BYTE_TEXTS[name]()
    certify_suffix_array(torch.from_numpy(text.copy()), _sa(oracle, text), chunk=1000)


def test_accepts_empty_text(oracle):
    certify_suffix_array(torch.zeros(0, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("dtype", [np.uint32, np.int64])
def test_accepts_integer_text(dtype):
    rng = np.random.default_rng(4)
    vocab = np.array([1, 2, 255, 256, 65536, 1 << 24, (1 << 32) - 1], dtype=np.int64)
    text = np.concatenate([vocab[rng.integers(0, len(vocab), 400)], np.full(100, 256), np.tile([65536, 1], 80)]).astype(dtype)
    certify_suffix_array(torch.from_numpy(text), _int_sa(text.astype(np.int64)), chunk=64)
    # zero is an ordinary symbol (the paper's integer index): the sentinel is still smaller
    text0 = np.array([0, 3, 0, 0, 3, 0, 1, 0], dtype=dtype)
    certify_suffix_array(torch.from_numpy(text0), _int_sa(text0.astype(np.int64)))


def _rejects(text, sa):
    with pytest.raises(AssertionError):
        certify_suffix_array(text, sa, chunk=7)


@pytest.mark.parametrize("name", ["mississippi", "aaaa", "abab", "dna"])
def test_rejects_every_adjacent_swap(oracle, name):
    text = {"mississippi": np.frombuffer(b"mississippi", np.uint8), "aaaa": np.frombuffer(b"aaaaaaaa", np.uint8),
            "abab": np.frombuffer(b"abababab", np.uint8), "dna": dna_text(40, 8)}[name]
    t = torch.from_numpy(text.copy())
    sa = _sa(oracle, text)
    for i in range(len(sa) - 1):
        bad = sa.clone()
        bad[i], bad[i + 1] = sa[i + 1], sa[i]
        _rejects(t, bad)


def test_rejects_duplicate_missing_sentinel_and_rotation(oracle):
    text = dna_text(300, 9)
    t = torch.from_numpy(text.copy())
    sa = _sa(oracle, text)
    certify_suffix_array(t, sa, chunk=7)
    for i, j in ((5, 6), (1, 200), (299, 3)):                    # a duplicated entry: one position is missing
        bad = sa.clone()
        bad[i] = sa[j]
        _rejects(t, bad)
    bad = sa.clone()                                             # the sentinel suffix not first (swapped with its neighbour)
    bad[0], bad[1] = sa[1], sa[0]
    _rejects(t, bad)
    bad = torch.cat([sa[1:], sa[:1]])                            # the sentinel moved to the end
    _rejects(t, bad)
    for r in (1, 2, 150):                                        # a rotated SA (after the sentinel, and the whole array)
        _rejects(t, torch.cat([sa[:1], torch.roll(sa[1:], r)]))
        _rejects(t, torch.roll(sa, r))
    _rejects(t, torch.where(sa == 0, torch.full_like(sa, len(sa)), sa))   # out of range
    _rejects(t, torch.flip(sa, [0]))


def test_rejects_wrong_integer_order():
    text = np.array([256, 1, 256, 65536, 256, 1], dtype=np.uint32)
    sa = _int_sa(text.astype(np.int64))
    certify_suffix_array(torch.from_numpy(text), sa)
    for i in range(len(sa) - 1):
        bad = sa.clone()
        bad[i], bad[i + 1] = sa[i + 1], sa[i]
        _rejects(torch.from_numpy(text), bad)
    # the same SA is wrong for a text whose symbols compare as bytes: 256 = 0x100 vs 1
    _rejects(torch.from_numpy(np.array([0, 1, 0, 0, 0, 1], dtype=np.uint32)), sa)


@pytest.mark.parametrize("dens", [1, 4, 32])
def test_derived_parts_and_ranks_equal_the_oracle(oracle, dens):
    text = np.concatenate([dna_text(20000, 6), np.frombuffer(b"\xfe" * 500 + b"Q", np.uint8)])
    t = torch.from_numpy(text.copy())
    sa = _sa(oracle, text)
    o = oracle.Index.from_text(text.tobytes(), dens)
    parts = o.parts()
    bwt = bwt_from_sa(t, sa, chunk=999)
    assert (bwt.numpy() == o.bwt()).all()
    check_byte_parts(t, sa, bwt, parts)
    for key, bad in (("C", lambda p: p.__setitem__("C", p["C"] + np.uint64(1))),
                     ("samples", lambda p: p["samples"].__setitem__(-1, p["samples"][-1] + np.uint64(1)))):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in parts.items()}
        bad(p)
        with pytest.raises(AssertionError):
            check_byte_parts(t, sa, bwt, p)
    rc = RankCounter(bwt, block=64, chunk=1000)
    grid, rnd = rank_probe_positions(len(sa), step=997, window=40, n_random=500, seed=3)
    assert int(grid.max()) == len(sa) and int(grid.min()) == 0
    for c in (0, ord("A"), ord("T"), 0xFE, ord("Q"), ord("Z")):
        pos = torch.cat([grid, rnd])
        got = rc.rank(pos, torch.full_like(pos, c), batch=300)
        assert got.tolist() == [o.wt_rank(int(p), c) for p in pos], c
