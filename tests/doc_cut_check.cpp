// Stand-alone check of csrc/doc_cut.hpp (document boundaries) against naive loops: nb, the straddle test, the capped window, the capped
// restart and the validation of the starts.  Compiled and run on the CPU by tests/test_documents_cpu.py, also under ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "doc_cut.hpp"

using namespace vlg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint64_t checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// document of a position by a linear scan (d starts, B[d] = n_text)
static uint64_t naive_doc(const std::vector<uint64_t>& B, uint64_t x)
{
    uint64_t j = 0;
    while (j + 2 < B.size() && B[j + 1] <= x) ++j;
    return j;
}

static int check_set(const std::vector<uint64_t>& starts, uint64_t n_text, const std::vector<uint64_t>& ms, const std::vector<uint64_t>& his)
{
    CHECK(doc_starts_invalid(starts.data(), starts.size(), n_text) == 0);
    std::vector<uint64_t> B(starts);
    B.push_back(n_text);
    const uint64_t d = starts.size();
    std::vector<uint64_t> xs;
    if (n_text <= 400) for (uint64_t x = 0; x < n_text; ++x) xs.push_back(x);
    else {
        for (uint64_t j = 0; j < d; ++j) { xs.push_back(B[j]); if (B[j]) xs.push_back(B[j] - 1); if (B[j] + 1 < n_text) xs.push_back(B[j] + 1); }
        xs.push_back(n_text - 1);
        for (int i = 0; i < 200; ++i) xs.push_back(rnd() % n_text);
    }
    for (uint64_t x : xs) {
        const uint64_t j = naive_doc(B, x), nb = B[j + 1];
        CHECK(doc_next_boundary(B.data(), d, x) == nb);
        CHECK(doc_upper_bound(B.data(), 0, d + 1, x) == j + 1);
        for (uint64_t m : ms) {
            // inside iff doc(x) == doc(x + m - 1), the last symbol still in the text
            bool inside = m >= 1 && x + m - 1 >= x && x + m - 1 < n_text && naive_doc(B, x + m - 1) == j;
            if (m == 0) inside = true;
            CHECK(doc_straddles(x, m, nb) == !inside);
            for (uint64_t hi : his) {
                const uint64_t xh = x + hi < x ? ~0ull : x + hi;                        // saturated, as the join passes it
                uint64_t thi = xh;
                const bool any = doc_cap_window(x, m, nb, thi);
                // naive: the largest y in [x, xh] with y + m <= nb (y in x's document, not crossing)
                const bool fits = m <= nb - x;
                CHECK(any == fits);
                if (any) {
                    uint64_t want = nb - m < xh ? nb - m : xh;
                    CHECK(thi == want);
                    CHECK(thi >= x && thi + m <= nb);
                    if (thi < xh) CHECK(thi + 1 > nb || m > nb - (thi + 1));            // the cap is tight: one further crosses
                }
            }
            // restart: end in x's document, end_len = m
            const uint64_t end = x + (nb - 1 - x) / 2;
            uint64_t k = doc_cap_restart(end, m, nb);
            CHECK(k <= nb && k >= end);
            CHECK(k ==((end + m < end || end + m > nb) ? nb : end + m));
        }
    }
    return 0;
}

int main()
{
    const std::vector<uint64_t> ms = {0, 1, 2, 3, 7, 64, 1000, 1ull << 40, ~0ull};
    const std::vector<uint64_t> his = {0, 1, 5, 100, (1ull << 62) - 1, (1ull << 63) - 1, 1ull << 63, ~0ull - 1, ~0ull};
    // one document; two; documents of one symbol; every position its own document
    if (check_set({0}, 1, ms, his)) return 1;
    if (check_set({0}, 300, ms, his)) return 1;
    if (check_set({0, 150}, 300, ms, his)) return 1;
    if (check_set({0, 1, 2, 9, 10, 11, 299}, 300, ms, his)) return 1;
    { std::vector<uint64_t> s; for (uint64_t i = 0; i < 130; ++i) s.push_back(i); if (check_set(s, 130, ms, his)) return 1; }
    { std::vector<uint64_t> s; for (uint64_t i = 0; i < 300; i += 7) s.push_back(i); if (check_set(s, 300, ms, his)) return 1; }
    // 64 and 65 documents (one block of fences), random starts, texts near 2^32 and near 2^64
    for (uint64_t d : std::vector<uint64_t>{64, 65, 129}) {
        for (uint64_t n_text : std::vector<uint64_t>{400, (1ull << 32) + 1, ~0ull}) {
            std::vector<uint64_t> s(1, 0);
            while (s.size() < d) {
                const uint64_t step = 1 + rnd() % (n_text / d > 1 ? n_text / d - 1 : 1);
                if (s.back() + step >= n_text || s.back() + step < s.back()) break;
                s.push_back(s.back() + step);
            }
            if (check_set(s, n_text, ms, his)) return 1;
        }
    }
    for (int it = 0; it < 200; ++it) {
        const uint64_t n_text = 2 + rnd() % 399;
        std::vector<uint64_t> s(1, 0);
        for (uint64_t x = 1; x < n_text; ++x) if (rnd() % 8 == 0) s.push_back(x);
        if (check_set(s, n_text, ms, his)) return 1;
    }
    // what create refuses
    const uint64_t a[] = {0, 5, 5}, b[] = {1, 2}, c[] = {0, 5, 4}, e[] = {0, 10};
    CHECK(doc_starts_invalid(nullptr, 1, 10) != 0);
    CHECK(doc_starts_invalid(a, 0, 10) != 0);
    CHECK(doc_starts_invalid(a, 3, 10) == 3);
    CHECK(doc_starts_invalid(b, 2, 10) != 0);
    CHECK(doc_starts_invalid(c, 3, 10) == 3);
    CHECK(doc_starts_invalid(e, 2, 10) == 2);
    CHECK(doc_starts_invalid(e, 1, 0) != 0);
    CHECK(doc_starts_invalid(e, 2, 11) == 0);
    printf("ok %llu checks\n", (unsigned long long)checks);
    return 0;
}
