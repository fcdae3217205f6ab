// csrc/window_cut.hpp alone, on the CPU: the keys of a window and the cut of a sorted list against a brute-force filter of the list
// (an occurrence v of m symbols lies inside [begin, end) of a text of n positions iff begin <= v and v + m <= min(end, n)).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "window_cut.hpp"

using namespace vlg;

static uint64_t g_checked = 0;

static void fail(const char* what, uint64_t b, uint64_t e, uint64_t m, uint64_t n)
{
    printf("FAILED %s: begin %llu end %llu m %llu n %llu\n", what, (unsigned long long)b, (unsigned long long)e, (unsigned long long)m, (unsigned long long)n);
    exit(1);
}

// inside(v) without the arithmetic under test: 128-bit, nothing can wrap
static bool inside(uint64_t v, uint64_t b, uint64_t e, uint64_t m, uint64_t n)
{
    const unsigned __int128 E = e < n ? e : n;
    return b <= v && (unsigned __int128)v + m <= E;
}

template <typename pos_t>
static void check_list(const std::vector<pos_t>& list, uint64_t b, uint64_t e, uint64_t m, uint64_t n)
{
    const WindowKeys k = window_keys(b, e, m, n);
    size_t lo = 0, hi = 0;
    window_cut_host(list.data(), list.size(), k, &lo, &hi);
    if (lo > hi || hi > list.size()) fail("cut out of order", b, e, m, n);
    for (size_t i = 0; i < list.size(); ++i)
        if (inside(list[i], b, e, m, n) != (i >= lo && i < hi)) fail("cut differs from the filter", b, e, m, n);
    ++g_checked;
}

// the keys themselves: every position of the text (and a few behind it) is inside iff klo <= v < khi
static void check_keys(uint64_t b, uint64_t e, uint64_t m, uint64_t n, const std::vector<uint64_t>& probes)
{
    if (!m) return;                                                    // (a sub-pattern is never empty)
    const WindowKeys k = window_keys(b, e, m, n);
    if (!k.empty && !(k.klo < k.khi)) fail("keys out of order", b, e, m, n);
    for (uint64_t v : probes) {
        const bool in = !k.empty && k.klo <= v && v < k.khi;
        if (in != inside(v, b, e, m, n)) fail("keys differ from the filter", b, e, m, n);
    }
    ++g_checked;
}

int main()
{
    // exhaustively on small texts: every window, every sub-pattern length, every position
    for (uint64_t n = 0; n <= 12; ++n) {
        std::vector<uint64_t> all;
        for (uint64_t v = 0; v < n + 2; ++v) all.push_back(v);
        for (uint64_t b = 0; b <= n + 2; ++b)
            for (uint64_t e = 0; e <= n + 2; ++e)
                for (uint64_t m = 1; m <= n + 2; ++m) {
                    check_keys(b, e, m, n, all);
                    std::vector<uint32_t> every, odd;                  // every position an occurrence can stand at; every other one
                    for (uint64_t v = 0; v + m <= n; ++v) { every.push_back((uint32_t)v); if (v & 1) odd.push_back((uint32_t)v); }
                    check_list(every, b, e, m, n);
                    check_list(odd, b, e, m, n);
                }
    }
    // the edge values, all combinations
    const uint64_t P32 = 1ull << 32, MAX = ~0ull;
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)1000, P32 - 1, P32, P32 + 1, MAX}) {
        std::vector<uint64_t> vals = {0, 1, n - 1, n, n + 1, P32 - 1, P32, MAX};
        for (uint64_t b : vals)
            for (uint64_t e : vals)
                for (uint64_t m : vals) check_keys(b, e, m, n, vals);
    }
    // khi = 2^32 over 32-bit positions (n = 2^32 one-symbol occurrences at most: the largest position is 2^32 - 1)
    {
        const WindowKeys k = window_keys(5, MAX, 1, P32);
        if (k.empty || k.klo != 5 || k.khi != P32) fail("khi = 2^32", 5, MAX, 1, P32);
        std::vector<uint32_t> list = {0, 5, 6, 0xFFFFFFFEu, 0xFFFFFFFFu};
        size_t lo, hi;
        window_cut_host(list.data(), list.size(), k, &lo, &hi);
        if (lo != 1 || hi != 5) fail("cut at 2^32", 5, MAX, 1, P32);
        check_list(list, 5, MAX, 1, P32);
        check_list(list, 6, P32 - 1, 1, P32);
    }
    // sorted lists of length 0, 1, 63, 64, 65 (with equal neighbours), windows on, before and behind every element
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (size_t len : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65}) {
        for (int rep = 0; rep < 4; ++rep) {
            const uint64_t n = 400;
            std::vector<uint32_t> l32;
            std::vector<uint64_t> l64;
            uint64_t v = rnd() % 3;
            for (size_t i = 0; i < len; ++i) { l32.push_back((uint32_t)v); l64.push_back(v); v += 1 + rnd() % 5; }
            for (uint64_t m : {(uint64_t)1, (uint64_t)3})
                for (uint64_t b = 0; b <= v + 2; ++b)
                    for (uint64_t e = b; e <= v + 4; e += 1 + (rep & 1)) { check_list(l32, b, e, m, n); check_list(l64, b, e, m, n); }
            check_list(l32, 0, MAX, 1, n);
            check_list(l64, MAX, MAX, 1, n);
        }
    }
    printf("ok %llu windows checked\n", (unsigned long long)g_checked);
    return 0;
}
