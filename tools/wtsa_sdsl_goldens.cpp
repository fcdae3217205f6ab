// tools/wtsa_sdsl_goldens.cpp -- writes tests/golden/wtsa_sdsl/: files of the paper's index, vlg_index<alphabet_tag,
// wt_int<bit_vector_il<>, rank_support_il<>>>, made by the reference's own serializers, and manifest.json (text and sizes per file).
// No build step or test runs it; the fixtures it wrote are committed.
//
// The reference's vlg_index.hpp cannot be instantiated here (it pulls construct_sa.hpp and divsufsort), so the generator does what
// vlg_index::serialize does (include/sdsl/vlg_index.hpp:181-198): m_text.serialize(out); m_wt.serialize(out).  The tree is the
// reference's wt_int built from the suffix array by its own int_vector_buffer constructor, as construct(wts, KEY_SA file) does
// (vlg_index.hpp:386-387); the suffix array of text + sentinel is sorted here by comparing suffixes (the sentinel is smaller than
// every symbol).  The text is int_vector<8> for byte_alphabet_tag and int_vector<0> of the given width for int_alphabet_tag.
//
// Compiled and run from the repository root, with the reference's sources at $REF:
//   g++ -std=c++11 -O2 -DNDEBUG -w -I$REF/include tools/wtsa_sdsl_goldens.cpp \
//       $REF/lib/{bits,util,io,memory_management,ram_fs,ram_filebuf,sfstream,config}.cpp -o /tmp/wtsa_sdsl_goldens
//   /tmp/wtsa_sdsl_goldens tests/golden/wtsa_sdsl
// and, for the rank-sample branch (more than 65 536 words of m_data, too large for a fixture):
//   /tmp/wtsa_sdsl_goldens --big <file.sdsl> <byte|int> <n> <seed>
#include <sdsl/int_vector.hpp>
#include <sdsl/int_vector_buffer.hpp>
#include <sdsl/bit_vector_il.hpp>
#include <sdsl/wt_int.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

using namespace sdsl;
typedef wt_int<bit_vector_il<>, rank_support_il<>> wt_type;

static int g_seq = 0;

// suffix array of text + sentinel, the sentinel smaller than every symbol
static std::vector<uint64_t> suffix_array(const std::vector<uint64_t>& t)
{
    const uint64_t n = t.size();
    std::vector<uint64_t> sa(n + 1);
    for (uint64_t i = 0; i <= n; ++i) sa[i] = i;
    std::sort(sa.begin(), sa.end(), [&](uint64_t a, uint64_t b) {
        while (a < n && b < n) {
            if (t[a] != t[b]) return t[a] < t[b];
            ++a; ++b;
        }
        return a == n && b != n;
    });
    return sa;
}

static void write_index(const std::string& path, const std::vector<uint64_t>& t, bool int_tag, uint8_t width)
{
    const std::vector<uint64_t> sa = suffix_array(t);
    std::string f = "@wtsa_sa_" + std::to_string(g_seq++);
    {
        int_vector<> v(sa.size(), 0, 64);
        for (uint64_t i = 0; i < sa.size(); ++i) v[i] = sa[i];
        store_to_file(v, f);
    }
    wt_type wt;
    {
        int_vector_buffer<> buf(f);
        wt = wt_type(buf, sa.size());
    }
    sdsl::remove(f);
    std::ofstream out(path, std::ios::binary | std::ios::trunc);
    if (int_tag) {
        int_vector<0> text(t.size(), 0, width);
        for (uint64_t i = 0; i < t.size(); ++i) text[i] = t[i];
        text.serialize(out);
    } else {
        int_vector<8> text(t.size());
        for (uint64_t i = 0; i < t.size(); ++i) text[i] = t[i];
        text.serialize(out);
    }
    wt.serialize(out);
}

static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

struct Case { std::string name; bool int_tag; uint8_t width; std::vector<uint64_t> text; };

static std::vector<uint64_t> bytes_of(const std::string& s) { return std::vector<uint64_t>(s.begin(), s.end()); }

int main(int argc, char** argv)
{
    if (argc == 6 && std::string(argv[1]) == "--big") {
        const bool int_tag = std::string(argv[3]) == "int";
        const uint64_t n = strtoull(argv[4], nullptr, 10);
        uint64_t seed = strtoull(argv[5], nullptr, 10);
        std::vector<uint64_t> t(n);
        for (auto& c : t) c = int_tag ? 1 + lcg(seed) % 1000 : "acgt"[lcg(seed) % 4];
        write_index(argv[2], t, int_tag, 64);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s <dir> | --big <file> <byte|int> <n> <seed>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<Case> cases;
    cases.push_back({"abracadabrasimsalabim", false, 8, bytes_of("abracadabrasimsalabim")});
    cases.push_back({"abracadabrasimsalabim_int64", true, 64, bytes_of("abracadabrasimsalabim")});   // construct_im of an int_vector<>
    {
        std::vector<uint64_t> t(300);
        uint64_t s = 17;
        for (auto& c : t) c = 1 + lcg(s) % ((1u << 17) - 1);
        t[5] = (1u << 17) - 1;
        cases.push_back({"int_width17", true, 17, t});
    }
    {
        std::vector<uint64_t> t(3000);
        uint64_t s = 4;
        for (auto& c : t) c = "ACGT"[lcg(s) % 4];
        cases.push_back({"dna_3000", false, 8, t});
    }
    {
        std::vector<uint64_t> t(511);                                                                  // n = 512, L = 9: S = 9 * 512
        uint64_t s = 9;
        for (auto& c : t) c = 'a' + lcg(s) % 26;
        cases.push_back({"s_multiple_of_512", false, 8, t});
    }
    cases.push_back({"empty", false, 8, {}});
    cases.push_back({"a", false, 8, bytes_of("a")});
    std::string manifest = "{\n";
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case& c = cases[k];
        write_index(dir + "/" + c.name + ".sdsl", c.text, c.int_tag, c.width);
        const uint64_t n = c.text.size() + 1;
        const uint32_t L = bits::hi(std::max<uint64_t>(n - 1, 1)) + 1;
        manifest += "  \"" + c.name + ".sdsl\": {\"alphabet\": \"" + (c.int_tag ? "int" : "byte") + "\", \"width\": " + std::to_string(c.width) +
                    ", \"n\": " + std::to_string(n) + ", \"levels\": " + std::to_string(L) + ", \"text\": ";
        if (c.int_tag) {
            manifest += "[";
            for (size_t i = 0; i < c.text.size(); ++i) manifest += (i ? ", " : "") + std::to_string(c.text[i]);
            manifest += "]";
        } else {
            manifest += "\"" + std::string(c.text.begin(), c.text.end()) + "\"";
        }
        manifest += std::string("}") + (k + 1 < cases.size() ? ",\n" : "\n");
    }
    manifest += "}\n";
    std::ofstream(dir + "/manifest.json") << manifest;
    return 0;
}
