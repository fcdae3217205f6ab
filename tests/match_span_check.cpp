// Stand-alone check of csrc/match_span.hpp (match texts) against naive loops: the range a match stands for -- the core is never cut,
// the flanks stop at the text's or the document's ends, a core that crosses its document's end keeps itself and gets no right flank --
// with flanks of 0, 1, UINT64_MAX and larger than the text, positions of 0, n_text - 1 and around 2^62, documents of one symbol,
// saturation everywhere; the symbols of a query's last sub-pattern and the tuple bases inside the pieces of a result.  Compiled and run
// on the CPU by tests/test_match_texts_cpu.py, also under ASan + UBSan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "match_span.hpp"

using namespace vlg;
typedef std::vector<uint64_t> vec;
typedef unsigned __int128 wide;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint64_t checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint64_t kMax = ~0ull;

// the definition, one symbol at a time: walk left from p0 while the flank lasts and the bound is not reached, right from ce likewise
// (small numbers only)
static MatchSpan by_steps(uint64_t p0, uint64_t ce, uint64_t B0, uint64_t B1, uint64_t fl, uint64_t fr, uint64_t reach)
{
    MatchSpan s{p0, ce};
    for (uint64_t i = 0; i < fl && i <= reach && s.b > B0; ++i) --s.b;
    for (uint64_t i = 0; i < fr && i <= reach && s.e < B1; ++i) ++s.e;
    return s;
}
// ... and in 128-bit arithmetic, where nothing can wrap (any numbers)
static MatchSpan by_wide(uint64_t p0, uint64_t ce, uint64_t B0, uint64_t B1, uint64_t fl, uint64_t fr)
{
    const wide lo = std::min<wide>(p0, B0), hi = std::max<wide>(B1, ce);
    const wide b = (wide)p0 >= (wide)fl + lo ? (wide)p0 - fl : lo;
    const wide e = std::min<wide>((wide)ce + fr, hi);
    return MatchSpan{(uint64_t)b, (uint64_t)e};
}

static int check_one(uint64_t p0, uint64_t ce, uint64_t B0, uint64_t B1, uint64_t fl, uint64_t fr)
{
    const MatchSpan s = match_span(p0, ce, B0, B1, fl, fr), w = by_wide(p0, ce, B0, B1, fl, fr);
    CHECK(s.b == w.b && s.e == w.e);
    CHECK(s.b <= p0 && s.e >= ce);                                              // the core is never cut
    CHECK(p0 - s.b <= fl && s.e - ce <= fr);                                    // no flank is longer than asked
    CHECK(s.b >= std::min(p0, B0) && s.e <= std::max(B1, ce));                  // ... or leaves the bounds
    if (ce >= B1) CHECK(s.e == ce);                                             // a core that ends on, or crosses, the end: no right flank
    if (p0 < ce) CHECK(s.b < s.e);
    return 0;
}

static int small_cases()
{
    // every placement on a text of 12 symbols, every document [B0, B1) around p0, cores that end inside, on and behind B1
    const uint64_t n = 12, flanks[] = {0, 1, 2, 5, 11, 12, 13, 1000, kMax - 1, kMax};
    for (uint64_t B0 = 0; B0 < n; ++B0)
        for (uint64_t B1 = B0 + 1; B1 <= n; ++B1)                              // (B1 = B0 + 1: a document of one symbol)
            for (uint64_t p0 = B0; p0 < B1; ++p0)
                for (uint64_t ce = p0 + 1; ce <= n; ++ce)
                    for (uint64_t fl : flanks)
                        for (uint64_t fr : flanks) {
                            const MatchSpan s = match_span(p0, ce, B0, B1, fl, fr), t = by_steps(p0, ce, B0, B1, fl, fr, n);
                            CHECK(s.b == t.b && s.e == t.e);
                            if (check_one(p0, ce, B0, B1, fl, fr)) return 1;
                            if (fl == kMax) CHECK(s.b == B0);                   // "to the bound"
                            if (fr == kMax) CHECK(s.e == std::max(B1, ce));
                            if (!fl && !fr) CHECK(s.b == p0 && s.e == ce);
                        }
    return 0;
}

static int large_cases()
{
    const uint64_t H = 1ull << 62;
    const uint64_t pts[] = {0, 1, 2, H - 2, H - 1, H, H + 1, 2 * H - 1, 2 * H, 3 * H, kMax - 2, kMax - 1, kMax};
    const uint64_t flanks[] = {0, 1, H - 1, H, H + 1, 2 * H, kMax - 1, kMax};
    for (uint64_t B0 : pts)
        for (uint64_t B1 : pts) {
            if (B1 <= B0) continue;
            for (uint64_t p0 : pts) {
                if (p0 < B0 || p0 >= B1) continue;
                for (uint64_t ce : pts) {
                    if (ce <= p0) continue;
                    for (uint64_t fl : flanks)
                        for (uint64_t fr : flanks)
                            if (check_one(p0, ce, B0, B1, fl, fr)) return 1;
                }
            }
        }
    // the text's ends: position 0 and a core that ends at n_text, for texts of 1 symbol and of 2^62 and 2^64 - 1 symbols
    for (uint64_t n_text : {(uint64_t)1, (uint64_t)20000, H, kMax}) {
        for (uint64_t fl : flanks)
            for (uint64_t fr : flanks) {
                MatchSpan s = match_span(0, 1, 0, n_text, fl, fr);
                CHECK(s.b == 0 && s.e == 1 + std::min(fr, n_text - 1));
                s = match_span(n_text - 1, n_text, 0, n_text, fl, fr);
                CHECK(s.e == n_text && s.b == n_text - 1 - std::min(fl, n_text - 1));
                if (check_one(0, 1, 0, n_text, fl, fr) || check_one(n_text - 1, n_text, 0, n_text, fl, fr)) return 1;
            }
    }
    for (int i = 0; i < 200000; ++i) {                                          // anything, bounds that do not even hold p0 included
        const uint64_t sh = rnd() % 64, p0 = std::min(rnd() >> sh, kMax - 1), ce = p0 + 1 + (rnd() >> (rnd() % 64)) % (kMax - p0);
        uint64_t B0 = rnd() >> (rnd() % 64), B1 = rnd() >> (rnd() % 64);
        if (B0 > B1) std::swap(B0, B1);
        const uint64_t fl = i % 7 == 0 ? kMax : rnd() >> (rnd() % 64), fr = i % 5 == 0 ? kMax : rnd() >> (rnd() % 64);
        const MatchSpan s = match_span(p0, ce, B0, B1, fl, fr), w = by_wide(p0, ce, B0, B1, fl, fr);
        CHECK(s.b == w.b && s.e == w.e && s.b <= p0 && s.e >= ce);
    }
    return 0;
}

static int core_cases()
{
    // ce = pl + m_last saturates; a core is one of the text iff p0 < ce <= n_text
    CHECK(match_core_end(0, 0) == 0 && match_core_end(5, 3) == 8);
    CHECK(match_core_end(kMax, 0) == kMax && match_core_end(kMax, 1) == kMax && match_core_end(kMax - 1, 1) == kMax);
    CHECK(match_core_end(1ull << 63, 1ull << 63) == kMax && match_core_end(kMax, kMax) == kMax);
    CHECK(span_sat_add(kMax - 3, 3) == kMax && span_sat_add(kMax - 3, 4) == kMax && span_sat_add(3, kMax - 3) == kMax && span_sat_add(0, 0) == 0);
    CHECK(match_core_ok(0, 1, 1) && !match_core_ok(0, 2, 1) && !match_core_ok(0, 0, 5) && !match_core_ok(3, 2, 5));
    CHECK(match_core_ok(4, 5, 5) && !match_core_ok(5, 6, 5) && !match_core_ok(7, kMax, kMax - 1) && match_core_ok(7, kMax, kMax));
    const uint64_t H = 1ull << 62;
    CHECK(match_core_ok(H - 1, H, H) && !match_core_ok(H, H + 1, H) && match_core_ok(H - 1, match_core_end(H - 1, 1), H));
    CHECK(!match_core_ok(H, match_core_end(3 * H, 2 * H), kMax - 1));          // (saturated: behind every text but the longest)

    // symbols of the last sub-pattern: bytes of the blob over bytes per symbol; a query without sub-patterns has none
    const uint64_t suboff[] = {0, 3, 4, 12, 12, 40};
    CHECK(match_last_symbols(suboff, 0, 1, 1) == 3 && match_last_symbols(suboff, 0, 2, 1) == 1 && match_last_symbols(suboff, 0, 3, 1) == 8);
    CHECK(match_last_symbols(suboff, 2, 3, 4) == 2 && match_last_symbols(suboff, 3, 5, 4) == 7 && match_last_symbols(suboff, 3, 4, 4) == 0);
    CHECK(match_last_symbols(suboff, 2, 2, 1) == 0 && match_last_symbols(suboff, 5, 5, 4) == 0);
    return 0;
}

// tuple bases against a naive walk over the pieces: random counts and k, pieces cut at random query borders, empty queries and
// pieces without matches (which a result does not list) anywhere
static int base_cases()
{
    for (int round = 0; round < 3000; ++round) {
        const uint64_t nq = 1 + rnd() % 40;
        vec off(nq + 1, 0);
        std::vector<uint32_t> k(nq);
        for (uint64_t q = 0; q < nq; ++q) {
            const uint64_t c = rnd() % 3 == 0 ? 0 : rnd() % 9;
            off[q + 1] = off[q] + c;
            k[q] = (uint32_t)(rnd() % 6);
        }
        vec cuts{0};
        for (uint64_t q = 1; q < nq; ++q) if (rnd() % 4 == 0) cuts.push_back(q);
        cuts.push_back(nq);
        vec first, want(nq, 0);
        for (size_t j = 0; j + 1 < cuts.size(); ++j) {
            uint64_t acc = 0;
            for (uint64_t q = cuts[j]; q < cuts[j + 1]; ++q) { want[q] = acc; acc += (off[q + 1] - off[q]) * k[q]; }
            if (off[cuts[j + 1]] > off[cuts[j]]) first.push_back(off[cuts[j]]);
        }
        const uint64_t np = first.size();
        first.push_back(off[nq]);
        vec got(nq, 77);
        match_tuple_bases(off.data(), k.data(), nq, first.data(), np, got.data());
        for (uint64_t q = 0; q < nq; ++q)
            if (off[q + 1] > off[q]) CHECK(got[q] == want[q]);                   // (the base of a query without matches is never read)
    }
    return 0;
}

int main()
{
    if (small_cases() || large_cases() || core_cases() || base_cases()) return 1;
    printf("ok %llu checks\n", (unsigned long long)checks);
    return 0;
}
