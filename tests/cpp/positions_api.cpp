// tests/cpp/positions_api.cpp -- the C++17 mirror's search_positions (include/cobs_gpu_search.hpp) used the way a caller
// of ClassicSearch::search would use it; prints what a Python test compares with the checker.
//   positions_api Z THRESHOLD LIMIT QUERY INDEX [INDEX ...]
// Output: one line per result, "doc_name<TAB>score<TAB>word,word,..." (hex), then "search <n>" = the size of the plain
// search()'s result for the same arguments (the two calls must agree).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cobs_gpu_search.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    try {
        std::vector<std::string> paths(argv + 5, argv + argc);
        cobs_gpu::ClassicSearch s(paths);
        s.set_findere((unsigned)std::atoi(argv[1]));
        const double threshold = std::atof(argv[2]);
        const size_t limit = (size_t)std::strtoull(argv[3], nullptr, 10);
        const std::string query = argv[4];
        std::vector<cobs_gpu::SearchResult> result, plain;
        std::vector<std::vector<uint64_t>> positions;
        s.search_positions(query, result, positions, threshold, limit);
        if (positions.size() != result.size()) return 3;
        for (size_t i = 0; i < result.size(); ++i) {
            std::printf("%s\t%u\t", result[i].doc_name, result[i].score);
            for (size_t w = 0; w < positions[i].size(); ++w)
                std::printf("%s%llx", w ? "," : "", (unsigned long long)positions[i][w]);
            std::printf("\n");
        }
        s.search(query, plain, threshold, limit);
        for (size_t i = 0; i < plain.size() && i < result.size(); ++i)
            if (std::string(plain[i].doc_name) != result[i].doc_name || plain[i].score != result[i].score) return 4;
        std::printf("search %zu\n", plain.size());
    } catch (const cobs_gpu::Error& e) {
        std::printf("error %d %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
