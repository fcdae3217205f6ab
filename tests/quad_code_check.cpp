// CPU check of the quad block code (vlg_matching_amd/csrc/quad_code.hpp), built and run by tests/test_quad_code.py: the header the HIP
// kernels compile, against a digit-by-digit loop.  Every one of the 80 offsets of a block, for random words, words of one digit
// (each of the four) and blocks whose counts make digit 3's derived count the one in use.
#include "quad_code.hpp"
#include <cstdio>
#include <random>
using namespace vlg;

static unsigned long long checks = 0;

static uint32_t digit_at(const uint32_t w[5], uint32_t off) { return (w[off >> 4] >> ((off & 15u) * 2u)) & 3u; }

// cnt[d] = digits d of the node before the block (all four known here; the block stores three), start = their sum
template <typename pos_t>
static bool check_block(const uint32_t w[5], const uint64_t cnt[4])
{
    const uint64_t start = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    uint64_t seen[4] = {cnt[0], cnt[1], cnt[2], cnt[3]};
    for (uint32_t off = 0; off < kQuadDigits; ++off) {
        const uint32_t want_d = digit_at(w, off);
        uint32_t d = 9;
        const pos_t got = quad_rank_digit<pos_t>((uint32_t)cnt[0], (uint32_t)cnt[1], (uint32_t)cnt[2], w[0], w[1], w[2], w[3], w[4], (pos_t)start, off, d);
        if (d != want_d || got != (pos_t)seen[want_d]) {
            printf("off %u: digit %u (want %u), rank %llu (want %llu)\n", off, d, want_d, (unsigned long long)got, (unsigned long long)seen[want_d]);
            return false;
        }
        ++seen[want_d];
        ++checks;
    }
    return true;
}

int main()
{
    std::mt19937_64 rng(15);
    uint32_t w[5];
    const uint64_t zero[4] = {0, 0, 0, 0};
    for (uint32_t d = 0; d < 4; ++d) {                         // all-equal words, each digit: every offset ranks itself
        for (int i = 0; i < 5; ++i) w[i] = d * 0x55555555u;
        if (!check_block<uint32_t>(w, zero) || !check_block<uint64_t>(w, zero)) return 1;
        const uint64_t some[4] = {7, 80 * 3, 1, 160 - 8};      // ... with counts in front (a block start that is a multiple of 80)
        if (!check_block<uint32_t>(w, some) || !check_block<uint64_t>(w, some)) return 1;
    }
    printf("all-equal ok\n");
    {   // only digit 3 anywhere in the node: the derived count is the whole block start, up to the edge of 32 bits
        for (int i = 0; i < 5; ++i) w[i] = 0xFFFFFFFFu;
        const uint64_t big[4] = {0, 0, 0, 0xFFFFFFFFull / 80 * 80 - 80};
        if (!check_block<uint32_t>(w, big) || !check_block<uint64_t>(w, big)) return 1;
        const uint64_t wide[4] = {0xFFFFFFF0ull, 0xFFFFFFF0ull, 0xFFFFFFF0ull, 0xFFFFFFF0ull};     // a start beyond 32 bits, every count inside
        if (!check_block<uint64_t>(w, wide)) return 1;
    }
    printf("digit 3 ok\n");
    for (int it = 0; it < 200000; ++it) {
        for (int i = 0; i < 5; ++i) {
            uint32_t x = (uint32_t)rng();
            const int mode = it % 4;
            if (mode == 1) x &= (uint32_t)rng();               // mostly digit 0
            if (mode == 2) x |= (uint32_t)rng();               // mostly digit 3
            if (mode == 3) x &= 0x55555555u;                   // digits 0 and 1 only
            w[i] = x;
        }
        uint64_t cnt[4];
        for (int d = 0; d < 4; ++d) cnt[d] = rng() % (it % 2 ? 1000u : 0x3FFFFFFFu);
        if (!check_block<uint32_t>(w, cnt) || !check_block<uint64_t>(w, cnt)) return 1;
    }
    printf("random ok\n");
    printf("ok %llu checks\n", checks);
    return 0;
}
