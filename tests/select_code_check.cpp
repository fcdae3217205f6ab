// CPU check of the in-block select code (vlg_matching_amd/csrc/select_code.hpp), built and run by tests/test_select_code.py: the header the
// HIP kernels compile, against a bit-by-bit loop.
//   select224: every k of all-ones, all-zeros, single-bit and alternating blocks and of 10^5 random blocks, for ones and zeros
//   rrr_select63: every class, 10^3 random blocks each, through rrr_enc63 and back, for ones and zeros
//   rrr_select63_seq: the same through the reference's bit-by-bit numbering (rrr_helper.hpp:304-320)
#include "select_code.hpp"
#include <cstdio>
#include <random>
#include <vector>
using namespace vlg;

static unsigned long long checks = 0;

// the k-th `bit` among the first nbits of w[], bit by bit; -1 when there are fewer
static int naive_select(const uint32_t* w, int nbits, uint32_t bit, uint32_t k)
{
    uint32_t seen = 0;
    for (int p = 0; p < nbits; ++p)
        if (((w[p >> 5] >> (p & 31)) & 1u) == bit && ++seen == k) return p;
    return -1;
}

static bool check224(const uint32_t w[7])
{
    for (uint32_t bit = 0; bit < 2; ++bit) {
        const uint32_t m = bit ? 0u : ~0u;
        int want[224];                                        // the positions of the bit, by one loop over the 224 bits
        uint32_t have = 0;
        for (int p = 0; p < 224; ++p)
            if (((w[p >> 5] >> (p & 31)) & 1u) == bit) want[have++] = p;
        uint32_t pop = 0;
        for (int i = 0; i < 7; ++i) pop += (uint32_t)__builtin_popcount(w[i] ^ m);
        if (pop != have) { printf("count mismatch\n"); return false; }
        for (uint32_t k = 1; k <= have; ++k) {
            const uint32_t got = select224(w[0] ^ m, w[1] ^ m, w[2] ^ m, w[3] ^ m, w[4] ^ m, w[5] ^ m, w[6] ^ m, k);
            if ((int)got != want[k - 1]) { printf("select224 bit=%u k=%u got %u want %d\n", bit, k, got, want[k - 1]); return false; }
            ++checks;
        }
        if (have && naive_select(w, 224, bit, have) != want[have - 1]) { printf("loop mismatch\n"); return false; }
    }
    return true;
}

int main()
{
    std::mt19937_64 rng(11);
    // ---- the 224-bit block -----------------------------------------------------------------------------------------------------------
    {
        uint32_t w[7];
        for (int i = 0; i < 7; ++i) w[i] = ~0u;
        if (!check224(w)) return 1;
        for (int i = 0; i < 7; ++i) w[i] = 0;
        if (!check224(w)) return 1;
        for (int p = 0; p < 224; ++p) {                       // a single one, a single zero
            for (int i = 0; i < 7; ++i) w[i] = 0;
            w[p >> 5] = 1u << (p & 31);
            if (!check224(w)) return 1;
            for (int i = 0; i < 7; ++i) w[i] = ~w[i];
            if (!check224(w)) return 1;
        }
        for (int i = 0; i < 7; ++i) w[i] = 0x55555555u;
        if (!check224(w)) return 1;
        for (int i = 0; i < 7; ++i) w[i] = 0xAAAAAAAAu;
        if (!check224(w)) return 1;
        for (int it = 0; it < 100000; ++it) {
            for (int i = 0; i < 7; ++i) {
                uint32_t x = (uint32_t)rng();
                const int mode = it % 5;
                if (mode == 1) x &= (uint32_t)rng();
                if (mode == 2) x |= (uint32_t)rng();
                if (mode == 3) x &= (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
                if (mode == 4) x |= (uint32_t)rng() | (uint32_t)rng() | (uint32_t)rng();
                w[i] = x;
            }
            if (!check224(w)) return 1;
        }
        for (uint32_t x : {1u, 0x80000000u, 0xFFFFFFFFu, 0x00010000u, 0x8001u})
            for (uint32_t k = 1; k <= (uint32_t)__builtin_popcount(x); ++k)
                if ((int)select32(x, k) != naive_select(&x, 32, 1, k)) { printf("select32 %x %u\n", x, k); return 1; }
        printf("select224 ok\n");
    }
    // ---- the 63-bit rrr blocks ---------------------------------------------------------------------------------------------------------
    static RrrTables t;
    build_rrr_tables(t);
    static uint64_t binom[64 * 64];                            // rrr_helper.hpp:173-207
    for (int n = 0; n < 64; ++n) binom[n * 64] = 1;
    for (int n = 1; n < 64; ++n)
        for (int k = 1; k < 64; ++k) binom[n * 64 + k] = k == n ? 1 : (k > n ? 0 : binom[(n - 1) * 64 + k - 1] + binom[(n - 1) * 64 + k]);
    for (uint32_t cls = 0; cls <= 63; ++cls) {
        for (int it = 0; it < 1000; ++it) {
            // a random block of the class: cls distinct positions
            uint64_t x = 0;
            std::vector<int> pos(63);
            for (int i = 0; i < 63; ++i) pos[i] = i;
            for (uint32_t i = 0; i < cls; ++i) { const int j = (int)i + (int)(rng() % (63 - i)); std::swap(pos[i], pos[j]); x |= 1ull << pos[i]; }
            uint32_t k_enc;
            const uint64_t o = rrr_enc63(t, x, k_enc);
            if (k_enc != cls) { printf("class mismatch\n"); return 1; }
            uint64_t nr = 0;                                   // bin_to_nr: rrr_helper.hpp:304-320
            { uint64_t b = x; uint32_t kk = cls, nn = 63; while (b) { if (b & 1) { nr += binom[(nn - 1) * 64 + kk]; --kk; } b >>= 1; --nn; } }
            const uint32_t w[2] = {(uint32_t)x, (uint32_t)(x >> 32)};
            for (uint32_t bit = 0; bit < 2; ++bit) {
                const uint32_t have = bit ? cls : 63 - cls;
                for (uint32_t k = 1; k <= have; ++k) {
                    const int want = naive_select(w, 63, bit, k);
                    const uint32_t got = rrr_select63(t, cls, o, bit, k), got_seq = rrr_select63_seq(binom, cls, nr, bit, k);
                    if ((int)got != want || (int)got_seq != want) {
                        printf("rrr select x=%llx class=%u bit=%u k=%u got %u / %u want %d\n", (unsigned long long)x, cls, bit, k, got, got_seq, want);
                        return 1;
                    }
                    ++checks;
                }
            }
        }
    }
    printf("rrr_select63 ok: 64 classes\n");
    printf("ok %llu checks\n", checks);
    return 0;
}
