// tests/cpp/best_api.cpp -- the C++17 mirror's search_best (include/cobs_gpu_search.hpp) used the way a caller of
// ClassicSearch::search would use it; prints what a Python test compares with the Python mirror.
//   best_api Z THRESHOLD LIMIT GROUP_SIZE INDEX QUERY [QUERY ...]
// Output: per group "group <g> <n>", then one line per record "doc_name<TAB>query<TAB>score<TAB>positions<TAB>ties".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cobs_gpu_search.hpp"

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    try {
        cobs_gpu::ClassicSearch s(std::vector<std::string>{argv[5]});
        s.set_findere((unsigned)std::atoi(argv[1]));
        const double threshold = std::atof(argv[2]);
        const size_t limit = (size_t)std::strtoull(argv[3], nullptr, 10);
        const size_t step = (size_t)std::strtoull(argv[4], nullptr, 10);
        if (step == 0) return 2;
        const std::vector<std::string> queries(argv + 6, argv + argc);
        std::vector<size_t> offs{0};
        for (size_t q = 0; q < queries.size(); q += step) offs.push_back(std::min(q + step, queries.size()));
        std::vector<std::vector<cobs_gpu::ClassicSearch::BestResult>> results;
        s.search_best(queries, offs, results, threshold, limit);
        if (results.size() + 1 != offs.size()) return 3;
        for (size_t g = 0; g < results.size(); ++g) {
            std::printf("group %zu %zu\n", g, results[g].size());
            for (const auto& r : results[g]) std::printf("%s\t%u\t%u\t%u\t%u\n", r.doc_name, r.query, r.score, r.positions, r.ties);
        }
    } catch (const cobs_gpu::Error& e) {
        std::printf("error %d %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
