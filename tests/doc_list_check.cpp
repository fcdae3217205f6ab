// Stand-alone check of csrc/doc_list_math.hpp (document listing) against naive loops: the head rule, the padded layout of the pieces,
// head ranks from per-run counts and head bits, df from ranks at query borders, counts from consecutive heads closed at the query's
// end.  Compiled and run on the CPU by tests/test_doc_listing_cpu.py, also under ASan + UBSan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "doc_cut.hpp"
#include "doc_list_math.hpp"

using namespace vlg;
typedef std::vector<uint64_t> vec;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint64_t checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Listing { vec df, docs, counts, first_match; };

// the definition: per query, maximal runs of equal documents, by linear scans
static Listing naive(const vec& pos, const vec& off, const vec& B)
{
    Listing l;
    for (size_t q = 0; q + 1 < off.size(); ++q) {
        uint64_t n = 0;
        for (uint64_t i = off[q]; i < off[q + 1]; ++i) {
            uint64_t j = 0;
            while (j + 2 < B.size() && B[j + 1] <= pos[i]) ++j;
            if (i > off[q] && l.docs.back() == j) { ++l.counts.back(); continue; }
            l.docs.push_back(j); l.counts.push_back(1); l.first_match.push_back(i);
            ++n;
        }
        l.df.push_back(n);
    }
    return l;
}

// the passes of the device, in plain loops over the header's arithmetic: pieces cut at the query borders `cuts`, runs of `run`
static int by_passes(const vec& pos, const vec& off, const vec& B, const vec& cuts, uint64_t run, Listing& l)
{
    const uint64_t nq = off.size() - 1, M = off[nq];
    vec piece_m;
    for (size_t k = 0; k + 1 < cuts.size(); ++k)
        if (off[cuts[k + 1]] > off[cuts[k]]) piece_m.push_back(off[cuts[k + 1]] - off[cuts[k]]);      // pieces without matches are left out
    const uint64_t np = piece_m.size();
    vec first(np + 1), pad(np + 1);
    doclist_layout(piece_m.data(), np, run, first.data(), pad.data());
    CHECK(first[np] == M && pad[np] % run == 0);
    for (uint64_t k = 0; k < np; ++k) {
        CHECK(pad[k] % run == 0 && std::binary_search(off.begin(), off.end(), first[k]));
        CHECK(pad[k + 1] - pad[k] >= piece_m[k] && pad[k + 1] - pad[k] < piece_m[k] + run);
        for (uint64_t e : {(uint64_t)0, piece_m[k] / 2, piece_m[k] - 1}) CHECK(doclist_piece_of(first.data(), np, first[k] + e) == k);
    }
    // head pass: garbage where no match stands, as on the device -- no rank may read it
    vec bits(pad[np] / 64 + 1, 0), heads(pad[np] / run + 1, 0);
    for (auto& w : bits) w = rnd();
    uint64_t q = 0;
    for (uint64_t k = 0; k < np; ++k)
        for (uint64_t e = 0; e < piece_m[k]; ++e) {
            const uint64_t g = first[k] + e, at = pad[k] + e;
            while (off[q + 1] <= g) ++q;
            const uint64_t d = doc_upper_bound(B.data(), 0, B.size(), pos[g]) - 1;
            const uint64_t dp = g ? doc_upper_bound(B.data(), 0, B.size(), pos[g - 1]) - 1 : ~0ull;
            const bool head = doclist_head(g == off[q], d, dp);
            if (at % 64 == 0) bits[at / 64] = 0;                                 // a step writes its word whole
            if (head) { bits[at / 64] |= 1ull << (at % 64); ++heads[at / run]; }
        }
    // scan (exclusive; the entry behind the last run becomes the total)
    uint64_t acc = 0;
    for (auto& h : heads) { const uint64_t c = h; h = acc; acc += c; }
    const uint64_t n_pairs = heads.back();
    // borders
    vec pair_off(nq + 1);
    for (uint64_t i = 0; i <= nq; ++i) pair_off[i] = doclist_rank_of_match(first.data(), pad.data(), np, heads.data(), bits.data(), run, off[i]);
    CHECK(pair_off[0] == 0 && pair_off[nq] == n_pairs);
    l.df.clear();
    for (uint64_t i = 0; i < nq; ++i) { CHECK(pair_off[i] <= pair_off[i + 1]); l.df.push_back(pair_off[i + 1] - pair_off[i]); }
    // scatter
    l.docs.assign(n_pairs, ~0ull); l.first_match.assign(n_pairs, ~0ull); l.counts.assign(n_pairs, ~0ull);
    for (uint64_t k = 0; k < np; ++k)
        for (uint64_t e = 0; e < piece_m[k]; ++e) {
            const uint64_t at = pad[k] + e;
            if (!((bits[at / 64] >> (at % 64)) & 1)) continue;
            const uint64_t slot = doclist_rank(heads.data(), bits.data(), run, at);
            CHECK(slot < n_pairs && l.docs[slot] == ~0ull);
            l.docs[slot] = doc_upper_bound(B.data(), 0, B.size(), pos[first[k] + e]) - 1;
            l.first_match[slot] = first[k] + e;
        }
    doclist_counts(off.data(), pair_off.data(), nq, l.first_match.data(), l.counts.data());
    return 0;
}

static int check_case(const vec& pos, const vec& off, const vec& starts, uint64_t n_text, const vec& cuts, const char* name)
{
    vec B(starts);
    B.push_back(n_text);
    const Listing want = naive(pos, off, B);
    uint64_t total = 0;
    for (uint64_t c : want.counts) total += c;
    CHECK(total == pos.size());
    for (uint64_t run : {(uint64_t)64, (uint64_t)192, (uint64_t)2048}) {
        Listing got;
        if (by_passes(pos, off, B, cuts, run, got)) { printf("  in case %s, run %llu\n", name, (unsigned long long)run); return 1; }
        CHECK(got.df == want.df);
        CHECK(got.docs == want.docs);
        CHECK(got.first_match == want.first_match);
        CHECK(got.counts == want.counts);
    }
    return 0;
}

// counts[q] ascending positions per query
static void fill(const vec& counts, uint64_t n_text, vec& pos, vec& off)
{
    pos.clear(); off.assign(1, 0);
    for (uint64_t c : counts) {
        vec p;
        for (uint64_t i = 0; i < c; ++i) p.push_back(rnd() % n_text);
        std::sort(p.begin(), p.end());
        pos.insert(pos.end(), p.begin(), p.end());
        off.push_back(pos.size());
    }
}

int main()
{
    const uint64_t n_text = 5000;
    vec every(n_text), random_starts(1, 0), pos, off;
    for (uint64_t i = 0; i < n_text; ++i) every[i] = i;
    for (uint64_t x = 1; x < n_text; ++x) if (rnd() % 40 == 0) random_starts.push_back(x);
    const struct { const char* name; vec starts; } docs[] = {{"one document", {0}}, {"every position its own document", every}, {"random", random_starts},
                                                             {"two", {0, 2500}}};
    // empty queries at the front, in the middle, several in a row, at the end; long and one-match queries
    const vec shapes[] = {
        {0, 0, 700, 0, 1, 0, 0, 0, 300, 1, 1, 1, 0},
        {5000},
        {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
        {63, 1, 64, 0, 65, 127, 0, 0, 192, 2048, 1, 2047},
        {0, 0, 0},
        {0, 3, 0},
    };
    int n_cases = 0;
    for (const auto& d : docs)
        for (const auto& shape : shapes)
            for (int rep = 0; rep < 3; ++rep) {
                fill(shape, n_text, pos, off);
                const uint64_t nq = shape.size();
                // query borders inside a document: with one or two documents every border is one; check it where it can fail
                if (d.starts.size() <= 2 && nq > 4 && pos.size() > 100) {
                    bool inside = false;
                    for (uint64_t q = 1; q < nq; ++q)
                        if (off[q] > 0 && off[q] < pos.size() && off[q] > off[q - 1] && (d.starts.size() == 1 || (pos[off[q] - 1] < 2500) == (pos[off[q]] < 2500))) inside = true;
                    CHECK(inside);
                }
                // pieces: one, one per query, and random cuts (piece borders inside documents, pieces without matches)
                vec one = {0, nq}, each, some(1, 0);
                for (uint64_t q = 0; q <= nq; ++q) each.push_back(q);
                for (uint64_t q = 1; q < nq; ++q) if (rnd() % 3 == 0) some.push_back(q);
                some.push_back(nq);
                if (check_case(pos, off, d.starts, n_text, one, d.name) || check_case(pos, off, d.starts, n_text, each, d.name) ||
                    check_case(pos, off, d.starts, n_text, some, d.name)) return 1;
                n_cases += 3;
            }
    // the head rule itself
    CHECK(doclist_head(true, 3, 3) && doclist_head(false, 3, 4) && !doclist_head(false, 3, 3) && doclist_head(true, 3, 4));
    CHECK(doclist_runs(0, 64) == 0 && doclist_runs(1, 64) == 1 && doclist_runs(64, 64) == 1 && doclist_runs(65, 64) == 2);
    printf("ok %d cases, %llu checks\n", n_cases, (unsigned long long)checks);
    return 0;
}
