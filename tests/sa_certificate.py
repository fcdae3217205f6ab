"""Exact checks of a suffix array and of what an FM-index derives from it, independent of any second suffix sorter.

certify_suffix_array (Burkhardt & Kaerkkaeinen 2003, the O(n) check): SA is the suffix array of T' = text + sentinel iff
  * SA[0] is the sentinel suffix,
  * SA is a permutation of [0, n),
  * for every neighbouring pair a = SA[i], b = SA[i + 1] (i >= 1): T'[a] < T'[b], or T'[a] == T'[b] and ISA[a + 1] < ISA[b + 1].
(Induction on the suffix length: the order of the shorter suffixes a + 1, b + 1 is the one SA itself gives them.)

Everything else the byte FM-index builder emits then follows from a certified SA by plain array operations: the BWT, the symbol
histogram (C, char2comp), the SA samples, and wavelet-tree ranks (RankCounter).  Plain torch, on whatever device the tensors are
on, int64 throughout (positions reach 2^32 at full size), in chunks so that temporaries stay bounded."""
import numpy as np
import torch

CHUNK = 1 << 27


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def _symbols(text, n):
    """p (int64 positions in [0, n)) -> T'[p] as int64, the sentinel (p == n - 1) as -1: smaller than every symbol, 0 included"""
    def at(p):
        v = text[p.clamp(max=max(n - 2, 0))].to(torch.int64) if n > 1 else torch.zeros_like(p)
        return torch.where(p == n - 1, torch.full_like(v, -1), v)
    return at


def hbm_used():
    """bytes of device memory in use on the current GPU (every allocator's, not only torch's)"""
    free, total = torch.cuda.mem_get_info()
    return total - free


def certify_suffix_array(text, sa, chunk=CHUNK, stats=None):
    """Assert that `sa` (int64, n = len(text) + 1 entries) is the suffix array of text + sentinel.  `text`: uint8 tensor, or for an
    integer text a uint32 / int64 tensor, without the sentinel; both on the same device.  Raises AssertionError.  stats (a dict, GPU
    tensors): "hbm_peak" is raised to the device memory in use while the ISA and the first chunk's temporaries are alive."""
    text, sa = _t(text), _t(sa)
    assert sa.dtype == torch.int64 and sa.dim() == 1, sa.dtype
    if text.dtype not in (torch.uint8, torch.int64):
        text = text.to(torch.int64)                       # uint32 and friends: integer texts are small
    n = sa.numel()
    assert text.numel() + 1 == n, (text.numel(), n)
    assert int(sa[0]) == n - 1, "the sentinel suffix must sort first"
    assert int(sa.min()) >= 0 and int(sa.max()) < n, "SA value out of range"
    isa = torch.full((n,), -1, dtype=torch.int64, device=sa.device)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        isa[sa[s:e]] = torch.arange(s, e, dtype=torch.int64, device=sa.device)
    assert int(isa.min()) >= 0, "SA is not a permutation of [0, n)"
    at = _symbols(text, n)
    for s in range(1, n - 1, chunk):
        e = min(n - 1, s + chunk)
        a, b = sa[s:e], sa[s + 1:e + 1]
        ta, tb = at(a), at(b)
        ok = ta < tb
        eq = ta == tb
        ok |= eq & (isa[(a + 1).clamp(max=n - 1)] < isa[(b + 1).clamp(max=n - 1)])
        if stats is not None and s == 1 and sa.is_cuda:
            stats["hbm_peak"] = max(stats.get("hbm_peak", 0), hbm_used())
        if not bool(ok.all()):
            i = s + int(torch.nonzero(~ok)[0, 0])
            raise AssertionError("suffixes SA[%d] = %d and SA[%d] = %d are out of order" % (i, int(sa[i]), i + 1, int(sa[i + 1])))
    del isa


def bwt_from_sa(text, sa, chunk=CHUNK):
    """BWT[i] = T'[(SA[i] - 1) mod n] of a byte text (the sentinel is 0) -> uint8 tensor on sa's device"""
    text, sa = _t(text), _t(sa)
    n = sa.numel()
    out = torch.empty(n, dtype=torch.uint8, device=sa.device)
    for s in range(0, n, chunk):
        p = sa[s:s + chunk] - 1
        v = text[p.clamp(min=0, max=max(n - 2, 0))] if n > 1 else torch.zeros_like(p, dtype=torch.uint8)
        out[s:s + chunk] = torch.where(p < 0, torch.zeros_like(v), v)
    return out


def histogram(seq, chunk=CHUNK):
    """byte histogram (int64[256]) of a uint8 tensor"""
    h = torch.zeros(256, dtype=torch.int64, device=seq.device)
    for s in range(0, seq.numel(), chunk):
        h += torch.bincount(seq[s:s + chunk].to(torch.int64), minlength=256)
    return h


def check_byte_parts(text, sa, bwt, parts):
    """n, sigma, char2comp, C (byte_alphabet of the BWT) and the SA-order samples SA[j * dens] of an exported byte index equal what
    the certified `sa` implies."""
    n = sa.numel()
    assert parts["n"] == n
    hist = histogram(bwt).cpu().numpy()
    assert hist.sum() == n and hist[0] == 1
    present = hist > 0
    assert parts["sigma"] == int(present.sum())
    c2c = np.where(present, np.cumsum(present) - 1, 0).astype(np.uint8)
    assert (np.asarray(parts["char2comp"]) == c2c).all(), "char2comp"
    want_C = np.concatenate([[0], np.cumsum(hist[present])]).astype(np.uint64)
    assert (np.asarray(parts["C"], dtype=np.uint64) == want_C).all(), "C"
    dens = int(parts["dens"])
    smp = np.asarray(parts["samples"], dtype=np.uint64)
    assert len(smp) == (n + dens - 1) // dens, (len(smp), n, dens)
    want = sa[::dens]
    got = torch.from_numpy(smp.view(np.int64)).to(sa.device)
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, "samples[%d] != SA[%d]" % (int(bad[0, 0]), int(bad[0, 0]) * dens)
    return hist


class RankCounter:
    """Exact rank(i, c) = #{j < i : BWT[j] == c} from a (certified) byte BWT on the device: per-block histograms, their prefix sums,
    and a count inside the probe's block."""

    def __init__(self, bwt, block=4096, chunk=CHUNK):
        self.bwt, self.block, self.n = bwt, block, bwt.numel()
        dev = bwt.device
        hist = histogram(bwt)
        self.symbols = torch.nonzero(hist).flatten()                          # present byte values, ascending
        S = self.symbols.numel()
        self.code = torch.full((256,), -1, dtype=torch.int64, device=dev)
        self.code[self.symbols] = torch.arange(S, dtype=torch.int64, device=dev)
        nblocks = (self.n + block - 1) // block
        counts = torch.zeros(nblocks + 1, S, dtype=torch.int64, device=dev)  # counts[k + 1] = histogram of block k
        chunk = max(block, chunk // block * block)
        for s in range(0, self.n, chunk):
            e = min(self.n, s + chunk)
            key = self.code[bwt[s:e].to(torch.int64)] + S * (torch.arange(e - s, dtype=torch.int64, device=dev) // block)
            nb = (e - s + block - 1) // block
            counts[1 + s // block: 1 + s // block + nb] = torch.bincount(key, minlength=nb * S).view(nb, S)
            del key
        self.cum = torch.cumsum(counts, dim=0)                                 # cum[k] = histogram of BWT[0, k * block)

    def rank(self, pos, sym, batch=4096):
        """pos: int64 tensor of positions in [0, n]; sym: byte values (any tensor) -> int64 ranks"""
        dev = self.bwt.device
        pos, sym = pos.to(dev, torch.int64), sym.to(dev, torch.int64)
        out = torch.zeros_like(pos)
        j = torch.arange(self.block, dtype=torch.int64, device=dev)
        for s in range(0, pos.numel(), batch):
            p, c = pos[s:s + batch], self.code[sym[s:s + batch]]
            k = p // self.block
            base = k * self.block
            win = self.bwt[(base[:, None] + j[None, :]).clamp(max=self.n - 1)].to(torch.int64)
            local = ((self.code[win] == c[:, None]) & (j[None, :] < (p - base)[:, None])).sum(1)
            r = self.cum[k, c.clamp(min=0)] + local
            out[s:s + batch] = torch.where(c < 0, torch.zeros_like(r), r)
        return out


def rank_probe_positions(n, step=1 << 20, window=256, n_random=100000, seed=0):
    """positions in [0, n] where the wavelet tree is probed: every `step`-th, every position in windows around 2^31, 2^32 and the
    end of the text, and n_random random ones -> (grid: int64 tensor, random: int64 tensor), both on the CPU"""
    grid = [np.arange(0, n + 1, step, dtype=np.int64)]
    for mid in (1 << 31, 1 << 32, n):
        if mid - window <= n:
            grid.append(np.arange(max(0, mid - window), min(n, mid + window) + 1, dtype=np.int64))
    grid = np.unique(np.concatenate(grid))
    rnd = np.random.default_rng(seed).integers(0, n + 1, n_random).astype(np.int64)
    return torch.from_numpy(grid), torch.from_numpy(rnd)


def check_wt_ranks(V, idx, counter, grid, rnd, seed=0):
    """vlg_wt_rank_batch of `idx` equals the exact counts: every present symbol (and one absent one) at every grid position, one
    random present symbol at every random position.  -> number of probes"""
    dev = counter.bwt.device
    syms = counter.symbols.cpu()
    present = set(syms.tolist())
    absent = [c for c in range(1, 256) if c not in present][:1]
    all_syms = torch.cat([syms, torch.tensor(absent, dtype=torch.int64)])
    pos = torch.cat([grid.repeat_interleave(len(all_syms)), rnd])
    g = torch.Generator().manual_seed(seed)
    sym = torch.cat([all_syms.repeat(len(grid)), syms[torch.randint(0, len(syms), (len(rnd),), generator=g)]])
    want = counter.rank(pos, sym)
    d_pos, d_sym = pos.to(dev), sym.to(torch.uint8).to(dev)
    d_out = torch.zeros_like(d_pos)
    V.capi.check(V.lib().vlg_wt_rank_batch(idx._h, d_pos.data_ptr(), d_sym.data_ptr(), d_out.data_ptr(), len(pos), None))
    torch.cuda.synchronize()
    bad = torch.nonzero(d_out != want)
    if bad.numel():
        b = int(bad[0, 0])
        raise AssertionError("wt rank(%d, %d): device %d, exact %d (%d of %d probes differ)"
                             % (int(pos[b]), int(sym[b]), int(d_out[b]), int(want[b]), bad.numel(), len(pos)))
    return len(pos)


def check_index_against_sa(V, d_text, d_sa, indexes, seed=0, parts=None):
    """An FM-index built on the device against a certified SA of its text: C, char2comp and the samples of indexes[0] (plain, SA
    order; `parts`: its export_parts() when the caller already has them), and wavelet-tree rank probes on every index (plain and
    rrr).  -> (number of rank positions, number of rank probes per index)"""
    bwt = bwt_from_sa(d_text, d_sa)
    check_byte_parts(d_text, d_sa, bwt, parts if parts is not None else indexes[0].export_parts())
    counter = RankCounter(bwt)
    grid, rnd = rank_probe_positions(d_sa.numel(), seed=seed)
    probes = [check_wt_ranks(V, idx, counter, grid, rnd, seed) for idx in indexes]
    return len(grid) + len(rnd), probes
