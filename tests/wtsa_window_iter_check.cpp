// vlg_iterator_gpu on a text window: locate(idx, query, begin, end) of vlg_index_gpu.hpp, run to its end (it asks the device for 16
// matches, then for three times what it holds, every request beginning where the one before stopped).
//     wtsa_window_iter_check <file> <query> <begin> <end>     one line per match: the positions of its sub-patterns
#include <cstdio>
#include <cstdlib>
#include <string>
#include "vlg_index_gpu.hpp"

namespace vh = vlg_host;

int main(int argc, char* argv[])
{
    if (argc != 5) return 2;
    try {
        vh::vlg_index_gpu<vh::byte_alphabet_tag> idx;
        vh::construct(idx, argv[1], 1);
        auto matches = vh::locate(idx, argv[2], std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
        for (auto m = matches.begin(); m != matches.end(); ++m) {
            std::string line;
            for (size_t s = 0; s < m.size(); ++s) line += (s ? " " : "") + std::to_string(m[(int)s]);
            std::puts(line.c_str());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
