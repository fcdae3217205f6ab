// index_fm_gpu::search_batch_windows (host/index_fm_gpu.hpp) against positions computed here by brute force: pattern j on the window
// [B, E) has the matches of the same pattern on the stand-alone text T[B, E), shifted by B.
//     fm_window_host_check        builds its own text, prints "ok <windows> <matches>"; a window that begins behind its end must throw
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "index_fm_gpu.hpp"

namespace vh = vlg_host;

// first positions of the lazy, left-most, non-overlapping matches of `re` (benchmark dialect) on `text`, by their definition: an
// element of list i is live when a live element of list i + 1 lies inside its gap window; a match is the least live x_0 >= restart
// followed by the least live partner list by list; the next one starts at its last position + end_len
static std::vector<uint64_t> brute(const std::string& text, const std::string& re)
{
    vlg_parsed_query q;
    vh::check(vlg_parse_query(re.data(), re.size(), VLG_DIALECT_BENCHMARK, &q));
    std::vector<std::vector<uint64_t>> L(q.k);
    for (uint32_t i = 0; i < q.k; ++i) {
        const std::string sub = re.substr(q.sub_off[i], q.sub_len[i]);
        for (size_t at = text.find(sub); at != std::string::npos; at = text.find(sub, at + 1)) L[i].push_back(at);
        if (L[i].empty()) return {};
    }
    std::vector<std::vector<uint64_t>> live(q.k);
    live[q.k - 1] = L[q.k - 1];
    for (int i = (int)q.k - 2; i >= 0; --i)
        for (uint64_t x : L[i]) {
            auto p = std::lower_bound(live[i + 1].begin(), live[i + 1].end(), x + q.lo[i + 1]);
            if (p != live[i + 1].end() && *p <= x + q.hi[i + 1]) live[i].push_back(x);
        }
    std::vector<uint64_t> out;
    uint64_t restart = 0;
    for (;;) {
        auto p = std::lower_bound(live[0].begin(), live[0].end(), restart);
        if (p == live[0].end()) break;
        uint64_t x = *p;
        out.push_back(x);
        for (uint32_t i = 1; i < q.k; ++i) x = *std::lower_bound(live[i].begin(), live[i].end(), x + q.lo[i]);
        restart = x + q.end_len;
    }
    return out;
}

int main()
{
    try {
        std::string text;
        uint64_t x = 2463534242ull;
        for (int i = 0; i < 6000; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; text += "ACGT"[(x >> 20) & 3]; }
        const uint64_t n = text.size();
        vh::index_fm_gpu idx(std::vector<uint8_t>(text.begin(), text.end()));
        const std::vector<std::string> res = {"AC", "AC.{0,9}G", "GT.{2,20}TTA.{0,5}C", "A.{1,1}A", "TTTTTTTTTTTTTTTT"};
        const std::vector<std::pair<uint64_t, uint64_t>> wins = {{0, n}, {0, ~0ull}, {0, 0}, {n, n}, {n + 5, ~0ull}, {500, 3500}, {1234, 1300},
                                                                 {1234, 1235}, {1, n - 1}, {2999, 3002}, {4096, 4160}};
        std::vector<vh::gapped_pattern> pats;
        std::vector<uint64_t> begins, ends;
        for (const std::string& re : res)
            for (const auto& w : wins) { pats.emplace_back(re); begins.push_back(w.first); ends.push_back(w.second); }
        vlg_result_summary sum;
        const std::vector<vh::gapped_search_result> got = idx.search_batch_windows(pats, begins, ends, VLG_DIALECT_BENCHMARK, &sum);
        uint64_t matches = 0;
        for (size_t i = 0; i < pats.size(); ++i) {
            const uint64_t E = std::min<uint64_t>(ends[i], n), B = std::min<uint64_t>(begins[i], E);
            std::vector<uint64_t> want = brute(text.substr(B, E - B), pats[i].raw_regexp);
            for (uint64_t& v : want) v += B;
            if (got[i].positions != want) {
                std::fprintf(stderr, "pattern %s on [%llu, %llu): %zu positions, %zu expected\n", pats[i].raw_regexp.c_str(), (unsigned long long)begins[i],
                             (unsigned long long)ends[i], got[i].positions.size(), want.size());
                return 1;
            }
            matches += want.size();
        }
        if (sum.n_matches != matches || matches < 500) { std::fprintf(stderr, "n_matches %llu, counted %llu\n", (unsigned long long)sum.n_matches, (unsigned long long)matches); return 1; }
        // the unwindowed batch afterwards is the search of before
        std::vector<vh::gapped_pattern> plain;
        for (const std::string& re : res) plain.emplace_back(re);
        const std::vector<vh::gapped_search_result> whole = idx.search_batch(plain);
        for (size_t i = 0; i < res.size(); ++i) if (whole[i].positions != brute(text, res[i])) { std::fprintf(stderr, "unwindowed search differs\n"); return 1; }
        bool thrown = false;
        try { begins[3] = 9; ends[3] = 8; (void)idx.search_batch_windows(pats, begins, ends); }
        catch (const std::invalid_argument&) { thrown = true; }
        if (!thrown) { std::fprintf(stderr, "begin > end did not throw\n"); return 1; }
        std::printf("ok %zu %llu\n", pats.size(), (unsigned long long)matches);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
