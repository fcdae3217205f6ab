// CPU check of the tree collapse behind the quad image (vlg_matching_amd/csrc/quad_code.hpp: quad_collapse), built and run by
// tests/test_quad_code.py.  For Huffman-shaped trees over several count vectors: every symbol's code, taken two bits at a time through
// the quad node table, ends in the symbol's leaf; the levels a walk would count equal the code length; a digit that cannot occur
// leads nowhere; every quad node is reached by exactly one digit; the nodes' blocks follow each other as size / 80 + 1.
#include "quad_code.hpp"
#include <algorithm>
#include <cstdio>
#include <functional>
#include <queue>
#include <string>
#include <vector>
using namespace vlg;

struct Node { uint32_t base; uint32_t child[2]; };            // (the device layout's fields that the collapse reads)

struct Tree {
    std::vector<Node> dn;
    std::vector<uint64_t> size;                                // bits of an inner node
    std::vector<uint64_t> leaf_count;                          // by compact symbol
    std::vector<std::vector<uint32_t>> code;                   // by compact symbol: the bits from the root
};

// Huffman shape by a min-heap on (frequency, creation order), numbered breadth first: what the index's tree builder does
static Tree huffman(const std::vector<uint64_t>& counts)
{
    struct Tmp { uint64_t freq; int64_t sym, child[2]; };
    std::vector<Tmp> tmp;
    typedef std::pair<uint64_t, uint64_t> P;
    std::priority_queue<P, std::vector<P>, std::greater<P>> pq;
    for (size_t c = 0; c < counts.size(); ++c) { pq.push(P(counts[c], tmp.size())); tmp.push_back(Tmp{counts[c], (int64_t)c, {-1, -1}}); }
    while (pq.size() > 1) {
        const P a = pq.top(); pq.pop();
        const P b = pq.top(); pq.pop();
        pq.push(P(a.first + b.first, tmp.size()));
        tmp.push_back(Tmp{a.first + b.first, -1, {(int64_t)a.second, (int64_t)b.second}});
    }
    Tree t;
    const uint32_t nn = (uint32_t)tmp.size();
    t.dn.assign(nn, Node{0, {0, 0}});
    t.size.assign(nn, 0);
    t.leaf_count = counts;
    t.code.assign(counts.size(), {});
    std::vector<int64_t> src(nn);
    std::vector<std::vector<uint32_t>> path(nn);
    src[0] = (int64_t)nn - 1;
    uint32_t next = 1;
    for (uint32_t v = 0; v < nn; ++v) {
        const Tmp& s = tmp[src[v]];
        if (s.child[0] < 0) { t.code[s.sym] = path[v]; continue; }
        t.size[v] = s.freq;
        for (uint32_t k = 0; k < 2; ++k) {
            src[next] = s.child[k];
            path[next] = path[v];
            path[next].push_back(k);
            const Tmp& ch = tmp[s.child[k]];
            t.dn[v].child[k] = ch.child[0] < 0 ? (kQuadLeaf | (uint32_t)ch.sym) : next;
            ++next;
        }
    }
    return t;
}

static unsigned long long checks = 0;

static bool check(const char* name, const std::vector<uint64_t>& counts)
{
    const Tree t = huffman(counts);
    QuadPlan q;
    if (!quad_collapse(t.dn.data(), t.size.data(), (uint32_t)t.dn.size(), t.leaf_count.data(), q) || !q.fits) { printf("%s: no plan\n", name); return false; }
    const uint32_t nq = (uint32_t)q.nodes.size();
    size_t longest = 0;
    for (size_t c = 0; c < counts.size(); ++c) {
        const std::vector<uint32_t>& code = t.code[c];
        longest = std::max(longest, code.size());
        uint32_t v = 0, levels = 0;
        size_t at = 0;
        for (;;) {
            if (at >= code.size()) { printf("%s: symbol %zu: the code ran out inside the tree\n", name, c); return false; }
            const uint32_t b1 = code[at], b2 = at + 1 < code.size() ? code[at + 1] : 0u;      // (a first bit that ends in a leaf: the digit b1 << 1)
            const uint32_t ch = q.nodes[v].child[b1 << 1 | b2];
            if (ch == kQuadNone) { printf("%s: symbol %zu: a digit of its code leads nowhere\n", name, c); return false; }
            const uint32_t spent = 2u - ((ch >> 30) & 1u);
            levels += spent;
            at += spent;
            if (ch & kQuadLeaf) {
                if ((ch & ~(kQuadLeaf | kQuadOne)) != c) { printf("%s: symbol %zu ends in leaf %u\n", name, c, ch & ~(kQuadLeaf | kQuadOne)); return false; }
                break;
            }
            if (ch >= nq) { printf("%s: child out of range\n", name); return false; }
            v = ch;
        }
        if (at != code.size() || levels != code.size()) { printf("%s: symbol %zu: %u levels for a code of %zu bits\n", name, c, levels, code.size()); return false; }
        ++checks;
    }
    // the table itself: unused digits exactly where the first bit ends in a leaf, every node but the root reached once, blocks in a row
    std::vector<uint32_t> reached(nq, 0);
    uint64_t blk = 0;
    for (uint32_t k = 0; k < nq; ++k) {
        const Node& v = t.dn[q.bin[k]];
        if (q.nodes[k].base != blk || q.size[k] != t.size[q.bin[k]]) { printf("%s: node %u starts at block %u, want %llu\n", name, k, q.nodes[k].base, (unsigned long long)blk); return false; }
        blk += q.size[k] / kQuadDigits + 1;
        for (uint32_t b1 = 0; b1 < 2; ++b1) {
            const bool leaf1 = (v.child[b1] & kQuadLeaf) != 0;
            const uint32_t c0 = q.nodes[k].child[b1 << 1], c1 = q.nodes[k].child[b1 << 1 | 1];
            if (leaf1 != (c1 == kQuadNone) || c0 == kQuadNone) { printf("%s: node %u: unused digits are wrong\n", name, k); return false; }
            if (leaf1 != ((c0 & kQuadOne) != 0 && (c0 & kQuadLeaf) != 0)) { printf("%s: node %u: one-level mark is wrong\n", name, k); return false; }
            for (uint32_t ch : {c0, c1})
                if (ch != kQuadNone && !(ch & kQuadLeaf)) { if (ch >= nq) return false; ++reached[ch]; }
            ++checks;
        }
    }
    for (uint32_t k = 0; k < nq; ++k)
        if (reached[k] != (k ? 1u : 0u)) { printf("%s: node %u reached %u times\n", name, k, reached[k]); return false; }
    if (blk != q.n_blocks) { printf("%s: block total\n", name); return false; }
    printf("%s ok: %zu symbols, longest code %zu, %zu inner nodes -> %u quad nodes\n", name, counts.size(), longest, t.dn.size() / 2, nq);
    return true;
}

int main()
{
    if (!check("sigma2", {5, 3})) return 1;
    if (!check("sigma3", {5, 3, 1})) return 1;
    {   // a spine: counts 1, 1, 2, 4, 8, ... -- a leaf at every depth down to 12
        std::vector<uint64_t> c{1, 1};
        for (int i = 1; i <= 11; ++i) c.push_back(1ull << i);
        if (!check("spine", c)) return 1;
    }
    if (!check("equal256", std::vector<uint64_t>(256, 1000))) return 1;
    // the flagship text's 28 symbols (sentinel first): counts of its first 2^20 characters
    if (!check("flagship28", {1, 155176, 41623, 39052, 41789, 49966, 24542, 28602, 37366, 29315, 39903, 38075, 40642, 26914, 32246, 36225, 23769, 29332, 35893,
                              33861, 35673, 30031, 33472, 31345, 38216, 24409, 35764, 35375})) return 1;
    {   // a count beyond 32 bits: the plan says the image does not fit
        const Tree t = huffman({1ull << 33, 5, 3});
        QuadPlan q;
        if (!quad_collapse(t.dn.data(), t.size.data(), (uint32_t)t.dn.size(), t.leaf_count.data(), q) || q.fits) { printf("a 2^33 count must not fit\n"); return 1; }
        const Tree one = huffman({7});
        if (quad_collapse(one.dn.data(), one.size.data(), (uint32_t)one.dn.size(), one.leaf_count.data(), q)) { printf("sigma = 1 has no image\n"); return 1; }
    }
    printf("ok %llu checks\n", checks);
    return 0;
}
