// cobs_amd/csrc/cobs_gpu_query.cpp -- command-line caller of the GPU query path with
// the flags and output format of the reference's `cobs query` sub-tool
// (reference src/cobs.cpp:471-527 flags, :410-469 query-file parsing and output):
//
//   cobs_gpu_query -i IDX [-i IDX2 ...] [-t 0.8] [-l N] (QUERY | -f QUERYFILE)
//
// Output: "doc_name<TAB>score" per hit; in file mode each query is preceded by
// "*comment<TAB>number-of-hits".  Lines starting with '>' or ';' delimit queries,
// sequence lines are concatenated.  Default threshold 0.8 (src/cobs.cpp:481-484).
// Unlike the reference, which runs the queries of a file one after the other, the
// whole file is one device batch.
#include <algorithm>
#include <cstdio>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/cobs_gpu_batch.h"          // cobs_gpu_write_synthetic (the generator sub-tool)
#include "../../include/cobs_gpu_construct.h"
#include "../../include/cobs_gpu_search.hpp"

static void usage() {
    std::fprintf(stderr,
                 "usage: cobs_gpu_query -i INDEX [-i INDEX ...] [-t THRESHOLD] [-l LIMIT] "
                 "[-d DEVICE[,DEVICE...]] [--hbm-budget GIB] [--findere Z] [--invalid-bases MODE] [--positions] [--prevalence] [--weighted] [--coverage] [--window N] [--fpr-adjust] [--sets FILE.tsv [--sets-by any|all | --sets-quorum X | --sets-profile]] (QUERY | -f QUERY_FILE)\n"
                 "       cobs_gpu_query doc-stats INDEX [--fill-above X]\n"
                 "         one line per document: file, name, sub-index, S_p, bits set in its filter, fill = bits / S_p, fpr = fill^H\n"
                 "       cobs_gpu_query doc-similarity INDEX --like NAME[,NAME...] [--min-jaccard J] [-l N]\n"
                 "       cobs_gpu_query doc-similarity INDEX --all-pairs --min-jaccard J\n"
                 "         the documents that share filter bits, by the Bloom-filter estimate of the Jaccard index of their k-mer sets;\n"
                 "         one line per pair: ref, doc, sub-index, shared bits, bit_jaccard, jaccard, containment_ref_in_doc,\n"
                 "         containment_doc_in_ref.  --like: per named document the others of ITS sub-index, best first (-l N: the\n"
                 "         first N); --all-pairs: every pair a < b of one sub-index whose estimate reaches J, in (a, b) order.\n"
                 "         Documents of different sub-indexes of a compact index are never compared.\n"
                 "       --fpr-adjust: every result line gets expected_fp (the positions the document's fill alone is expected to\n"
                 "         hit) and adjusted (the estimate of the truly shared positions) appended\n"
                 "       [--group N|all] [--read-threshold X]\n"
                 "       --group N: every N consecutive records of the query file are one group (all: the whole file); per group\n"
                 "        one line *<name of its first record><TAB><hits>, then doc_name<TAB>sum<TAB>votes for the documents whose\n"
                 "        summed score reaches -t of the group's positions; votes = the group's records that reach\n"
                 "        --read-threshold X (default 0) in the document; not with several devices or --hbm-budget\n"
                 "       [--best N|all | --best-by-name SEP]\n"
                 "       --best N: typing -- every N consecutive records of the query file are one group (all: the whole file), the\n"
                 "        alleles of a locus; per group one line *<name of its first record><TAB><hits>, then per document\n"
                 "        doc_name<TAB>best record's name<TAB>score<TAB>positions<TAB>ties: the record of the group that fits the\n"
                 "        document best (the largest score / positions), for the documents where it reaches -t of its own positions;\n"
                 "        ties = the group's records that fit equally well (honours -l, --findere and --invalid-bases)\n"
                 "       --best-by-name SEP: the same with the groups formed from the names: the maximal runs of consecutive records\n"
                 "        whose name up to the last SEP (one character) is equal (adk_1 adk_2 fumC_1: two groups with _); a name\n"
                 "        without SEP is its own group; the header line carries *<that prefix>.  Neither with several devices,\n"
                 "        --hbm-budget, --group, --sets, --weighted, --coverage, --window, --prevalence, --positions or --fpr-adjust.\n"
                 "       --positions: every result line gets a tab and one character per position of the query in that\n"
                 "        document, position 0 first: 1 = the k-mer there (with --findere Z: all Z + 1 from there) is present;\n"
                 "        the number of 1s is the score.  Not with several devices or --hbm-budget.\n"
                 "       --prevalence: instead of results, per query its *comment line (with the number of index files) and one\n"
                 "        line per index file: file_no<TAB>num_docs<TAB>n<TAB>c0 c1 ... c(n-1), c_p = the documents of the file\n"
                 "        that hold position p of the query (honours --findere and --invalid-bases).  Not with several devices\n"
                 "        or --hbm-budget.\n"
                 "       --weighted: IDF-weighted search -- a k-mer held by c of a file's D documents weighs 1 + min(14,\n"
                 "        floor(log2(D / c))) (0 when nobody holds it), a document scores the sum of the weights of the k-mers it\n"
                 "        holds and is a hit when that reaches -t of the query's total weight; same output as a plain query with\n"
                 "        the weighted score in place of the count (honours -l, --findere and --invalid-bases).  Not with several\n"
                 "        devices or --hbm-budget.\n"
                 "       --coverage: coverage search -- a document scores the query BASES that lie inside a k-mer it holds (with\n"
                 "        --findere Z: inside a window of Z + 1 present k-mers) and is a hit when that reaches -t of the query's\n"
                 "        length: a read with one substitution keeps all but one of its bases; same output as a plain query\n"
                 "        with the covered bases in place of the count (honours -l, --findere and --invalid-bases).  Not with\n"
                 "        several devices or --hbm-budget.\n"
                 "       --window N: window search -- a document scores the most positions it holds in any N (1 .. 4095) consecutive\n"
                 "        positions of the query and is a hit when that reaches -t of N (of the query's positions, if fewer): for a\n"
                 "        long query whose documents hold a stretch of it; same output as --coverage with that number as the score\n"
                 "        (honours -l, --findere and --invalid-bases); with --positions every line also gets the 0/1 string and the\n"
                 "        window's first start.  Not with several devices, --hbm-budget, --coverage, --prevalence, --weighted,\n"
                 "        --sets, --group or --fpr-adjust.\n"
                 "       --sets FILE.tsv: score every query against SETS of documents; the file holds lines\n"
                 "        document name<TAB>set name (a document it does not name is in no set; a name the index does not hold\n"
                 "        is an error).  Per query its *comment line (with the number of sets), then set_name<TAB>any<TAB>all for\n"
                 "        the sets that reach -t: any = the positions at least one member holds, all = the positions every\n"
                 "        member holds; ordered by --sets-by any|all (default any), cut by -l (honours --findere and\n"
                 "        --invalid-bases).  Not with several devices or --hbm-budget.\n"
                 "       --sets FILE.tsv --sets-quorum X (0 < X <= 1): the soft core -- per query its *comment line, then\n"
                 "        set_name<TAB>core<TAB>any<TAB>members for the sets that reach -t: core = the positions at least\n"
                 "        max(1, ceil(X * members)) members hold; ordered by core, cut by -l.\n"
                 "       --sets FILE.tsv --sets-profile: per query its *comment line, then per set one line\n"
                 "        set_name<TAB>members<TAB>c0 c1 ... c(n-1), c_p = the members that hold position p of the query.\n"
                 "       --findere Z (0..7): a k-mer position scores only when Z + 1 consecutive k-mers are all present\n"
                 "        (findere, beyond `cobs query`: far fewer false-positive k-mers; a query needs k + Z characters)\n"
                 "       --invalid-bases error|miss|skip: a character outside ACGT fails the call (error, the default, as `cobs query`\n"
                 "        does), or its k-mers count as absent (miss), or they also leave the threshold's denominator (skip:\n"
                 "        reads with an N are answered over their valid k-mers)\n"
                 "       -d 0,1,2,3: the index is sharded by sub-index block over the listed GPUs, every search is\n"
                 "        one scan per GPU + one RCCL exchange (same results as on one GPU)\n"
                 "       (--load-complete and -T/--threads of `cobs query` are accepted and ignored: the index\n"
                 "        always lives in HBM, or is streamed through it under --hbm-budget)\n"
                 "       cobs_gpu_query classic-construct | compact-construct | classic-combine | compact-construct-combine ...\n"
                 "        (the construction sub-tools of `cobs`, same arguments; see cobs_gpu_tools.cpp)\n"
                 "       cobs_gpu_query generate-queries PATH [-k K] [-p N] [-n N] [-N] [-s SIZE] [-S SEED] [-o OUT]\n"
                 "                      [--file-type T] [--canonical] [-d DEVICE]   (`cobs generate-queries`, same flags)\n"
                 "       cobs_gpu_query --benchmark -i INDEX [-k KMERS] [-q QUERIES] [-w WARMUP] [--seed S] [--dist]\n"
                 "       cobs_gpu_query benchmark-fpr INDEX [-k KMERS] [-q QUERIES] [-w WARMUP] [-d|--dist] [--seed S] [--device N[,M..]]\n"
                 "                      [--findere Z] [--invalid-bases MODE]\n"
                 "        (`cobs benchmark-fpr`, same flags: -d / --dist adds the distribution of all scores,\n"
                 "         RESULT name=benchmark_fpr fpr=<score> dist=<count> lines; --findere Z adds findere=Z and\n"
                 "         fpr=<scoring positions / all positions of the timed queries in all documents> to the RESULT line)\n"
                 "       cobs_gpu_query --write-synthetic OUT (--classic -n DOCS -s ROWS | --compact -n DOCS -p PAGE_SIZE\n"
                 "                      -s ROWS_0,ROWS_1,...) [--num-hashes H] [--seed S] [-d DEVICE]\n"
                 "        (a random-bit index file, density 0.3, for benchmarks of any size)\n"
                 "       cobs_gpu_query --construct-random OUT [-s SIGNATURE_SIZE] [-n DOCS] [-m DOCUMENT_SIZE]\n"
                 "                      [--num-hashes H] [--seed S]    (`cobs classic-construct-random`, same flags and defaults)\n");
}

// `cobs benchmark-fpr` (reference src/cobs.cpp:605-730): random ACGT queries of
// num_kmers + 30 characters from one std::mt19937(seed), default threshold 0 and
// num_results 0, one RESULT line.  Here the queries run as one device batch; the
// reference's t_io / t_and / t_add phases are one scan kernel (t_scan).
// --dist (src/cobs.cpp:627-632, 664-670): the reference tallies counts[r.score]++ over every result of every query on
// the host; here every shard's score rows are tallied on the device (cobs_gpu_batch_score_histogram), pass by pass.
static bool score_distribution(const std::vector<cobs_gpu_index*>& shards, const std::vector<std::string>& queries,
                               unsigned num_kmers, std::vector<uint64_t>& hist) {
    hist.assign((size_t)num_kmers + 31, 0);
    for (cobs_gpu_index* ix : shards) {
        const uint64_t slots = std::max<uint64_t>(cobs_gpu_local_counts(ix), 1);
        const size_t per_pass = (size_t)std::max<uint64_t>(1, (4ull << 30) / (slots * 4));      // <= 4 GiB of score rows per pass
        cobs_gpu_batch* b = nullptr;
        if (cobs_gpu_batch_create(ix, 0, 0, &b) != COBS_GPU_OK) return false;
        bool ok = true;
        for (size_t q0 = 0; q0 < queries.size() && ok; q0 += per_pass) {
            const size_t n = std::min(per_pass, queries.size() - q0);
            std::vector<const char*> qp(n);
            std::vector<size_t> ql(n);
            for (size_t i = 0; i < n; ++i) { qp[i] = queries[q0 + i].data(); ql[i] = queries[q0 + i].size(); }
            size_t bad = 0;
            ok = cobs_gpu_batch_set_queries(b, qp.data(), ql.data(), n) == COBS_GPU_OK &&
                 cobs_gpu_batch_run(b, 0.0, nullptr) == COBS_GPU_OK && cobs_gpu_batch_sync(b, nullptr, &bad) == COBS_GPU_OK &&
                 cobs_gpu_batch_score_histogram(b, hist.data(), hist.size()) == COBS_GPU_OK;
        }
        cobs_gpu_batch_destroy(b);
        if (!ok) return false;
    }
    return true;
}

static int benchmark(cobs_gpu::BatchSearch& s, const std::string& index, unsigned num_kmers,
                     unsigned num_queries, unsigned num_warmup, size_t seed, bool dist = false, int findere = -1) {
    static const char basepairs[4] = {'A', 'C', 'G', 'T'};
    std::mt19937 rng(seed);
    auto make = [&](unsigned n) {
        std::vector<std::string> v(n);
        for (auto& q : v) {
            q.resize(num_kmers + 30);
            for (auto& c : q) c = basepairs[rng() % 4];
        }
        return v;
    };
    std::vector<std::string> warm = make(num_warmup), queries = make(num_queries);
    std::vector<std::vector<cobs_gpu::SearchResult>> results;
    if (!warm.empty()) s.search_batch(warm, results);
    s.timer().reset();                       // (as benchmark_fpr_run does, src/cobs.cpp:623)
    const auto t0 = std::chrono::steady_clock::now();
    s.search_batch(queries, results);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const cobs_gpu::Timer t = s.timer();     // a copy is a snapshot (:644)
    // the reference's line (src/cobs.cpp:645-661) with its own keys -- t_io is the scan kernel (gather + AND + count are
    // one kernel: t_and / t_add read 0), sse2 / aio do not apply -- and, behind them, the GPU path's own phases
    std::cout << "RESULT name=benchmark  index=" << index << " kmer_queries=" << num_kmers
              << " queries=" << num_queries << " warmup=" << num_warmup
              << " results=" << (results.empty() ? 0 : results.back().size()) << " sse2=off aio=off"
              << " t_hashes=" << t.get("hashes") << " t_io=" << t.get("io") << " t_and=" << t.get("and rows")
              << " t_add=" << t.get("add rows") << " t_sort=" << t.get("sort results") << " backend=gpu"
              << " t_scan=" << t.get("scan") << " t_h2d=" << t.get("h2d") << " t_d2h=" << t.get("d2h")
              << " t_rank=" << t.get("rank") << " t_total=" << wall << " queries_per_s=" << num_queries / wall;
    if (findere >= 0) {
        // the false-positive rate of random queries: scoring positions over all positions (T_f - z per document of file f)
        double scored = 0, positions = 0;
        for (const auto& r : results)
            for (const auto& h : r) scored += (double)h.score;
        cobs_gpu_index* ix = s.handle();
        for (size_t f = 0; f < cobs_gpu_num_files(ix); ++f) {
            cobs_gpu_index_info in{};
            if (cobs_gpu_info(ix, f, &in) != COBS_GPU_OK) continue;
            const double T = (double)(num_kmers + 30) - (double)in.term_size + 1.0 - (double)findere;
            positions += (double)num_queries * (double)in.num_docs * std::max(T, 0.0);
        }
        std::cout << " findere=" << findere << " fpr=" << (positions > 0 ? scored / positions : 0.0);
    }
    std::cout << std::endl;
    if (dist) {
        results.clear();
        results.shrink_to_fit();
        std::vector<cobs_gpu_index*> shards;
        if (auto* sh = dynamic_cast<cobs_gpu::ShardedClassicSearch*>(&s)) shards = sh->shard_handles();
        else shards.push_back(s.handle());
        std::vector<uint64_t> hist;
        if (!score_distribution(shards, queries, num_kmers, hist)) {
            std::fprintf(stderr, "EXCEPTION: %s\n", cobs_gpu_last_error());
            return 1;
        }
        for (size_t sc = 0; sc < hist.size(); ++sc)      // std::map order: ascending scores, those that occur
            if (hist[sc]) std::cout << "RESULT name=benchmark_fpr fpr=" << sc << " dist=" << hist[sc] << std::endl;
    }
    return 0;
}

// `s.timer().print("search")` of the reference's process_query (src/cobs.cpp:468, cobs/util/timer.cpp:77-85):
// one "TIMER info=search name=seconds ... total=seconds" line on stderr.  The reference's phases are hashes / io /
// and rows (/ add rows); here: hashes (K1), h2d (query text), scan (K2: gather + AND + count), d2h, rank.
static void print_timer(const cobs_gpu::BatchSearch& s) { s.timer().print("search"); }

// --positions: the words of one result as n characters 0 / 1, position 0 first
static std::string position_string(const std::vector<uint64_t>& words, size_t n) {
    std::string out(n, '0');
    for (size_t p = 0; p < n && p / 64 < words.size(); ++p)
        if ((words[p / 64] >> (p % 64)) & 1u) out[p] = '1';
    return out;
}

// the queries of a `query` call with --positions: the result lines of `cobs query`, each with its 0/1 string appended
static std::vector<cobs_gpu::ClassicSearch::Adjusted> adjusted_of(cobs_gpu::ClassicSearch& s, const std::string& query,
                                                                  const std::vector<cobs_gpu::SearchResult>& result);
static std::string adjusted_columns(const cobs_gpu::ClassicSearch::Adjusted& a);

static void print_with_positions(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries,
                                 const std::vector<std::string>* comments, double threshold, size_t num_results, bool fpr_adjust) {
    std::vector<std::vector<cobs_gpu::SearchResult>> results;
    std::vector<std::vector<std::vector<uint64_t>>> pos;
    std::vector<std::vector<size_t>> npos;
    s.search_batch_positions(queries, results, pos, threshold, num_results, &npos);
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << results[q].size() << '\n';
        std::vector<cobs_gpu::ClassicSearch::Adjusted> adj;
        if (fpr_adjust) adj = adjusted_of(s, queries[q], results[q]);
        for (size_t i = 0; i < results[q].size(); ++i)
            std::cout << results[q][i].doc_name << '\t' << results[q][i].score << '\t'
                      << position_string(pos[q][i], npos[q][i]) << (fpr_adjust ? adjusted_columns(adj[i]) : std::string()) << '\n';
    }
}

// --window: the lines of --coverage with the best window's count as the score; with --positions every line gets the 0/1
// string of --positions and the first start of a window that reaches the score (cobs_gpu_best_window over the bitmap)
static void print_window(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries, const std::vector<std::string>* comments,
                         uint32_t window, double threshold, size_t num_results, bool positions) {
    std::vector<std::vector<cobs_gpu::SearchResult>> results;
    std::vector<std::vector<std::vector<uint64_t>>> pos;
    std::vector<std::vector<size_t>> npos;
    s.search_window(queries, window, results, threshold, num_results, positions ? &pos : nullptr, positions ? &npos : nullptr);
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << results[q].size() << '\n';
        for (size_t i = 0; i < results[q].size(); ++i) {
            std::cout << results[q][i].doc_name << '\t' << results[q][i].score;
            if (positions) {
                size_t start = 0;
                (void)cobs_gpu::best_window(pos[q][i], npos[q][i], window, &start);
                std::cout << '\t' << position_string(pos[q][i], npos[q][i]) << '\t' << start;
            }
            std::cout << '\n';
        }
    }
}

// --prevalence: per query its comment line and one line per index file: file_no, documents, positions, the counts
static void print_prevalence(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries, const std::vector<std::string>* comments) {
    std::vector<uint32_t> counts;
    std::vector<size_t> offs;
    s.prevalence(queries, counts, offs);
    const size_t nf = cobs_gpu_num_files(s.handle());
    std::vector<uint64_t> num_docs(nf);
    for (size_t f = 0; f < nf; ++f) {
        cobs_gpu_index_info info;
        if (cobs_gpu_info(s.handle(), f, &info) != COBS_GPU_OK) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
        num_docs[f] = info.num_docs;
    }
    std::string line;
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << nf << '\n';
        for (size_t f = 0; f < nf; ++f) {
            const size_t a = offs[q * nf + f], b = offs[q * nf + f + 1];
            line = std::to_string(f) + '\t' + std::to_string(num_docs[f]) + '\t' + std::to_string(b - a) + '\t';
            for (size_t i = a; i < b; ++i) {
                if (i > a) line += ' ';
                line += std::to_string(counts[i]);
            }
            std::cout << line << '\n';
        }
    }
}

// --sets FILE.tsv: lines `document name<TAB>set name`, read before the index is opened; false (with a message) for a file
// that cannot be read or a line that is not of that form, or a document named twice with different sets
static bool read_sets_tsv(const std::string& path, std::vector<std::pair<std::string, std::string>>& rows) {
    std::ifstream in(path);
    if (!in.good()) { std::fprintf(stderr, "--sets: could not open %s\n", path.c_str()); return false; }
    std::unordered_map<std::string, std::string> seen;
    std::string line;
    for (size_t no = 1; std::getline(in, line); ++no) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 == line.size() || line.find('\t', tab + 1) != std::string::npos) {
            std::fprintf(stderr, "--sets: line %zu of %s: expected document name<TAB>set name\n", no, path.c_str());
            return false;
        }
        const std::string doc = line.substr(0, tab), set = line.substr(tab + 1);
        const auto it = seen.find(doc);
        if (it != seen.end() && it->second != set) {
            std::fprintf(stderr, "--sets: line %zu of %s: document %s is already in set %s\n", no, path.c_str(), doc.c_str(), it->second.c_str());
            return false;
        }
        if (it == seen.end()) {
            seen.emplace(doc, set);
            rows.emplace_back(doc, set);
        }
    }
    return true;
}

// ... and its rows as labels of every index file: the set names numbered in sorted order (-> names), a document name the
// index does not hold is an error that names it
static void label_doc_sets(cobs_gpu::ClassicSearch& s, const std::vector<std::pair<std::string, std::string>>& rows,
                           std::vector<std::string>& names) {
    names.clear();
    for (const auto& r : rows) names.push_back(r.second);
    std::sort(names.begin(), names.end());
    names.erase(std::unique(names.begin(), names.end()), names.end());
    std::unordered_map<std::string, std::string> set_of(rows.begin(), rows.end());
    std::unordered_map<std::string, bool> found;
    const size_t nf = cobs_gpu_num_files(s.handle());
    for (size_t f = 0; f < nf; ++f) {
        cobs_gpu_index_info info;
        if (cobs_gpu_info(s.handle(), f, &info) != COBS_GPU_OK) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
        std::vector<uint32_t> labels(info.num_docs, COBS_GPU_NO_SET);
        bool any = false;
        for (uint64_t d = 0; d < info.num_docs; ++d) {
            const auto it = set_of.find(cobs_gpu_doc_name(s.handle(), f, d));
            if (it == set_of.end()) continue;
            labels[d] = (uint32_t)(std::lower_bound(names.begin(), names.end(), it->second) - names.begin());
            found[it->first] = true;
            any = true;
        }
        if (any) s.set_doc_sets(labels, (uint32_t)names.size(), f);
    }
    for (const auto& r : rows)
        if (!found.count(r.first)) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, "--sets: the index holds no document named " + r.first);
}

static void print_sets(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries, const std::vector<std::string>* comments,
                       const std::vector<std::string>& names, double threshold, uint32_t rank_by, size_t num_results) {
    std::vector<std::vector<cobs_gpu::ClassicSearch::SetResult>> results;
    s.search_sets(queries, results, threshold, rank_by, num_results);
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << results[q].size() << '\n';
        for (const auto& r : results[q]) std::cout << names[r.set] << '\t' << r.any << '\t' << r.all << '\n';
    }
}

// members of every set of every file, [file][set number]
static std::vector<std::vector<uint32_t>> set_members(cobs_gpu::ClassicSearch& s) {
    const size_t nf = cobs_gpu_num_files(s.handle());
    std::vector<std::vector<uint32_t>> members(nf);
    for (size_t f = 0; f < nf; ++f) {
        uint32_t n = 0;
        if (cobs_gpu_get_doc_sets(s.handle(), f, &n, nullptr, 0) != COBS_GPU_OK) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
        members[f].assign(n, 0);
        if (n && cobs_gpu_get_doc_sets(s.handle(), f, &n, members[f].data(), n) != COBS_GPU_OK)
            throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
    }
    return members;
}

// --sets-quorum X: per query its comment line, then set_name, core, any, members
static void print_sets_quorum(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries, const std::vector<std::string>* comments,
                              const std::vector<std::string>& names, double quorum, double threshold, size_t num_results) {
    std::vector<std::vector<cobs_gpu::ClassicSearch::SetQuorumResult>> results;
    s.search_sets_quorum(queries, results, quorum, threshold, num_results);
    const std::vector<std::vector<uint32_t>> members = set_members(s);
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << results[q].size() << '\n';
        for (const auto& r : results[q])
            std::cout << names[r.set] << '\t' << r.core << '\t' << r.any << '\t' << members[r.file_no][r.set] << '\n';
    }
}

// --sets-profile: per query its comment line, then per non-empty set of every labelled file: set_name, members, the counts
static void print_sets_profile(cobs_gpu::ClassicSearch& s, const std::vector<std::string>& queries, const std::vector<std::string>* comments,
                               const std::vector<std::string>& names) {
    std::vector<uint32_t> counts;
    std::vector<size_t> offs;
    s.set_prevalence(queries, counts, offs);
    const std::vector<std::vector<uint32_t>> members = set_members(s);
    const size_t nf = members.size();
    size_t lines = 0;
    for (const auto& m : members) lines += (size_t)std::count_if(m.begin(), m.end(), [](uint32_t v) { return v != 0; });
    std::string line;
    for (size_t q = 0; q < queries.size(); ++q) {
        if (comments) std::cout << (*comments)[q] << '\t' << lines << '\n';
        for (size_t f = 0; f < nf; ++f) {
            const size_t sets = (size_t)std::count_if(members[f].begin(), members[f].end(), [](uint32_t v) { return v != 0; });
            if (sets == 0) continue;
            const size_t n = (offs[q * nf + f + 1] - offs[q * nf + f]) / sets;
            size_t at = offs[q * nf + f];
            for (size_t c = 0; c < members[f].size(); ++c) {
                if (members[f][c] == 0) continue;
                line = names[c] + '\t' + std::to_string(members[f][c]) + '\t';
                for (size_t i = 0; i < n; ++i) {
                    if (i) line += ' ';
                    line += std::to_string(counts[at + i]);
                }
                at += n;
                std::cout << line << '\n';
            }
        }
    }
}

// --fpr-adjust: "\texpected_fp\tadjusted" of every result of one query.  Under --invalid-bases skip the positions are the
// query's valid ones per file, read from a device batch of that one query (cobs_gpu_batch_scored_positions).
static std::vector<cobs_gpu::ClassicSearch::Adjusted> adjusted_of(cobs_gpu::ClassicSearch& s, const std::string& query,
                                                                  const std::vector<cobs_gpu::SearchResult>& result) {
    if (s.invalid_bases() != COBS_GPU_INVALID_SKIP) return s.adjust(result, query.size());
    const size_t nf = cobs_gpu_num_files(s.handle());
    std::vector<uint64_t> valid(nf, 0);
    cobs_gpu_batch* b = nullptr;
    auto check = [&](cobs_gpu_status st) {
        if (st == COBS_GPU_OK) return;
        if (b) cobs_gpu_batch_destroy(b);
        throw cobs_gpu::Error(st, cobs_gpu_last_error());
    };
    check(cobs_gpu_batch_create(s.handle(), 1, query.size(), &b));
    const char* qp = query.data();
    const size_t ql = query.size();
    size_t bad = 0;
    check(cobs_gpu_batch_set_queries(b, &qp, &ql, 1));
    check(cobs_gpu_batch_run(b, 0.0, nullptr));
    check(cobs_gpu_batch_sync(b, nullptr, &bad));
    for (size_t f = 0; f < nf; ++f) {
        uint32_t v = 0;
        check(cobs_gpu_batch_scored_positions(b, f, &v));
        valid[f] = v;
    }
    cobs_gpu_batch_destroy(b);
    return s.adjust(result, query.size(), &valid);
}

static std::string adjusted_columns(const cobs_gpu::ClassicSearch::Adjusted& a) {
    char buf[96];
    std::snprintf(buf, sizeof buf, "\t%.2f\t%.2f", a.expected_fp, a.adjusted);
    return buf;
}

// `doc-stats INDEX [--fill-above X]`: file  doc_name  sub_index  S_p  bits  fill  fpr, one line per real document
static int doc_stats(int argc, char** argv) {
    std::string path;
    double above = -1.0;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--fill-above" && i + 1 < argc) above = std::atof(argv[++i]);
        else if (!a.empty() && a[0] != '-' && path.empty()) path = a;
        else { usage(); return 1; }
    }
    if (path.empty()) { usage(); return 1; }
    try {
        cobs_gpu::ClassicSearch s(path);
        for (size_t f = 0; f < cobs_gpu_num_files(s.handle()); ++f) {
            cobs_gpu_index_info info;
            if (cobs_gpu_info(s.handle(), f, &info) != COBS_GPU_OK) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
            const std::vector<uint64_t> bits = s.doc_bits(f);
            const std::vector<double> fill = s.doc_fill(f);
            for (uint64_t d = 0; d < info.num_docs; ++d) {
                if (!(fill[d] > above)) continue;
                const uint32_t page = info.kind == 0 ? 0u : (uint32_t)(d / (8 * info.page_size));
                std::printf("%zu\t%s\t%u\t%llu\t%llu\t%.6f\t%.6f\n", f, cobs_gpu_doc_name(s.handle(), f, d), page,
                            (unsigned long long)cobs_gpu_signature_size(s.handle(), f, page), (unsigned long long)bits[d], fill[d],
                            std::pow(fill[d], (double)info.num_hashes));
            }
        }
    } catch (const cobs_gpu::Error& e) {
        std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
        return 1;
    }
    return 0;
}

// `doc-similarity INDEX (--like NAME[,NAME...] [--min-jaccard J] [-l N] | --all-pairs --min-jaccard J)`: one line per pair,
//   ref  doc  sub_index  shared  bit_jaccard  jaccard  containment_ref_in_doc  containment_doc_in_ref
// (the floats with 17 significant digits, so that they read back as computed; a saturated filter's estimates are nan)
static void similarity_line(const char* ref, const cobs_gpu::ClassicSearch::SimilarDocument& r) {
    auto num = [](double v) {
        char buf[40];
        if (std::isnan(v)) return std::string("nan");
        std::snprintf(buf, sizeof buf, "%.17g", v);
        return std::string(buf);
    };
    std::printf("%s\t%s\t%u\t%llu\t%s\t%s\t%s\t%s\n", ref, r.doc_name, r.sub_index, (unsigned long long)r.shared, num(r.bit_jaccard).c_str(),
                num(r.jaccard).c_str(), num(r.containment_ref_in_doc).c_str(), num(r.containment_doc_in_ref).c_str());
}

static int doc_similarity(int argc, char** argv) {
    std::string path, like;
    bool all_pairs = false, have_min = false, have_limit = false;
    double min_jaccard = 0.0;
    size_t limit = 0;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--like" && i + 1 < argc) like = argv[++i];
        else if (a == "--min-jaccard" && i + 1 < argc) { min_jaccard = std::atof(argv[++i]); have_min = true; }
        else if ((a == "-l" || a == "--limit") && i + 1 < argc) { limit = (size_t)std::strtoull(argv[++i], nullptr, 10); have_limit = true; }
        else if (a == "--all-pairs") all_pairs = true;
        else if (!a.empty() && a[0] != '-' && path.empty()) path = a;
        else { usage(); return 1; }
    }
    if (path.empty() || all_pairs == !like.empty()) { usage(); return 1; }
    if (all_pairs && !have_min) {
        std::fprintf(stderr, "doc-similarity --all-pairs needs --min-jaccard J: the list of all pairs grows with the square of the documents\n");
        return 1;
    }
    if (all_pairs && have_limit) {
        std::fprintf(stderr, "doc-similarity: -l cuts the list of one --like reference, not --all-pairs\n");
        return 1;
    }
    try {
        cobs_gpu::ClassicSearch s(path);
        cobs_gpu_index_info info;
        if (cobs_gpu_info(s.handle(), 0, &info) != COBS_GPU_OK) throw cobs_gpu::Error(COBS_GPU_ERR_ARG, cobs_gpu_last_error());
        if (!all_pairs) {
            std::unordered_map<std::string, uint32_t> doc_of;
            for (uint64_t d = info.num_docs; d-- > 0;) doc_of[cobs_gpu_doc_name(s.handle(), 0, d)] = (uint32_t)d;    // (the first of equal names)
            std::vector<uint32_t> refs;
            for (size_t at = 0; at <= like.size();) {
                const size_t end = std::min(like.find(',', at), like.size());
                const std::string name = like.substr(at, end - at);
                const auto it = doc_of.find(name);
                if (it == doc_of.end()) {
                    std::fprintf(stderr, "doc-similarity: no document named %s in %s\n", name.c_str(), path.c_str());
                    return 1;
                }
                refs.push_back(it->second);
                at = end + 1;
            }
            const auto lists = s.similar_documents(refs, 0, min_jaccard, limit);
            for (size_t i = 0; i < refs.size(); ++i)
                for (const auto& r : lists[i]) similarity_line(cobs_gpu_doc_name(s.handle(), 0, refs[i]), r);
            return 0;
        }
        // every pair a < b of one sub-index, sub-index by sub-index: kChunk references per call (the library sweeps them panel
        // by panel), so the host holds kChunk rows of cells at a time and never a D x D buffer
        constexpr uint64_t kChunk = 64;
        const std::vector<uint64_t> bits = s.doc_bits(0);
        const uint64_t per = info.kind == 0 ? info.counts_size : 8 * info.page_size;
        for (uint64_t d0 = 0, pg = 0; d0 < info.num_docs; d0 += per, ++pg) {
            const uint64_t live = std::min<uint64_t>(per, info.num_docs - d0), sig = cobs_gpu_signature_size(s.handle(), 0, (uint32_t)pg);
            for (uint64_t a0 = 0; a0 + 1 < live; a0 += kChunk) {
                std::vector<uint32_t> refs;
                for (uint64_t a = a0; a < std::min(a0 + kChunk, live - 1); ++a) refs.push_back((uint32_t)(d0 + a));
                const auto shared = s.doc_shared_bits(refs, 0);
                for (size_t i = 0; i < refs.size(); ++i) {
                    const uint64_t a = refs[i];
                    for (uint64_t b = a + 1; b < d0 + live; ++b) {
                        const uint64_t c = shared[i][b - d0];
                        const auto e = cobs_gpu::ClassicSearch::jaccard_estimate(sig, (uint32_t)info.num_hashes, bits[a], bits[b], c);
                        if (!cobs_gpu::ClassicSearch::reaches(e.jaccard, min_jaccard)) continue;
                        similarity_line(cobs_gpu_doc_name(s.handle(), 0, a),
                                        cobs_gpu::ClassicSearch::SimilarDocument{cobs_gpu_doc_name(s.handle(), 0, b), b, (uint32_t)pg, c, e.bit_jaccard,
                                                                                 e.jaccard, e.containment_a_in_b, e.containment_b_in_a});
                    }
                }
            }
        }
    } catch (const cobs_gpu::Error& e) {
        std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
        return 1;
    }
    return 0;
}

int cobs_gpu_tools_main(int argc, char** argv);      // cobs_gpu_tools.cpp: *-construct, classic-combine, compact-construct-combine

int main(int argc, char** argv) {
    {
        const int rc = cobs_gpu_tools_main(argc, argv);
        if (rc >= 0) return rc;
        if (argc > 1 && std::string(argv[1]) == "query") { ++argv; --argc; }       // `cobs query ...`
        if (argc > 1 && std::string(argv[1]) == "doc-stats") return doc_stats(argc, argv);
        if (argc > 1 && std::string(argv[1]) == "doc-similarity") return doc_similarity(argc, argv);
    }
    // `cobs benchmark-fpr IN_FILE [-k N] [-q N] [-w N] [-d|--dist] [--seed S]` (src/cobs.cpp:672-730): the index is the
    // positional argument and -d means --dist, as there; the device list of this tool is spelled --device in this mode
    const bool fpr_mode = argc > 1 && std::string(argv[1]) == "benchmark-fpr";
    if (fpr_mode) { ++argv; --argc; }
    std::vector<std::string> index_paths;
    std::string query_line, query_file;
    double threshold = 0.8;
    size_t num_results = 0;
    std::vector<int> devices;
    uint64_t hbm_budget = 0;
    std::string synth_out, synth_rows, random_out;
    uint64_t document_size = 1000000;
    bool synth_compact = false, force_sharded = false;
    uint64_t synth_docs = 10000, synth_page = 0, synth_hashes = 1;
    bool bench = fpr_mode, dist = false;
    int findere = -1;                        // --findere Z; -1: not given (the handle's default, 0)
    unsigned invalid_bases = COBS_GPU_INVALID_ERROR;   // --invalid-bases MODE
    bool positions = false;                  // --positions
    bool prevalence = false;                 // --prevalence
    bool weighted = false;                   // --weighted
    bool coverage = false;                   // --coverage
    std::string window_arg;                  // --window N
    bool fpr_adjust = false;                 // --fpr-adjust
    std::string sets_file, sets_by;          // --sets FILE.tsv, --sets-by any|all
    std::string sets_quorum;                 // --sets-quorum X
    bool have_quorum = false;
    bool sets_profile = false;               // --sets-profile
    std::string group;                       // --group N|all
    double read_threshold = 0.0;             // --read-threshold X
    std::string best, best_sep;              // --best N|all, --best-by-name SEP
    bool best_by_name = false;
    unsigned num_kmers = 1000, num_queries = 10000, num_warmup = 100;
    size_t seed = std::random_device{}();
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", what); usage(); std::exit(1); }
            return argv[++i];
        };
        if (a == "-i" || a == "--index") index_paths.push_back(need("-i"));
        else if (a == "-f" || a == "--file") query_file = need("-f");
        else if (a == "-t" || a == "--threshold") threshold = std::atof(need("-t"));
        else if (a == "-l" || a == "--limit") num_results = (size_t)std::strtoull(need("-l"), nullptr, 10);
        else if (a == "--dist" || (fpr_mode && a == "-d")) dist = true;
        else if (a == "-d" || a == "--device") {
            const std::string v = need("-d");
            for (size_t p = 0; p < v.size();) {
                size_t e = v.find(',', p);
                if (e == std::string::npos) e = v.size();
                devices.push_back(std::atoi(v.substr(p, e - p).c_str()));
                p = e + 1;
            }
        }
        else if (a == "--sharded") force_sharded = true;        // the multi-GPU code path even for one device
        else if (a == "--write-synthetic") synth_out = need("--write-synthetic");
        else if (a == "--construct-random") random_out = need("--construct-random");
        else if (a == "-m" || a == "--document-size") document_size = std::strtoull(need("-m"), nullptr, 10);
        else if (a == "--classic") synth_compact = false;
        else if (a == "--compact") synth_compact = true;
        else if (a == "-n" || a == "--num-documents") synth_docs = std::strtoull(need("-n"), nullptr, 10);
        else if (a == "-s" || a == "--signature-size") synth_rows = need("-s");
        else if (a == "-p" || a == "--page-size") synth_page = std::strtoull(need("-p"), nullptr, 10);
        else if (a == "--num-hashes") synth_hashes = std::strtoull(need("--num-hashes"), nullptr, 10);
        else if (a == "--hbm-budget") hbm_budget = (uint64_t)(std::atof(need("--hbm-budget")) * 1073741824.0);
        else if (a == "--load-complete") {}                  // reference flags without a meaning here
        else if (a == "-T" || a == "--threads") (void)need("-T");
        else if (a == "--benchmark") bench = true;
        else if (a == "-k" || a == "--num-kmers") num_kmers = (unsigned)std::atoi(need("-k"));
        else if (a == "-q" || a == "--queries") num_queries = (unsigned)std::atoi(need("-q"));
        else if (a == "-w" || a == "--warmup") num_warmup = (unsigned)std::atoi(need("-w"));
        else if (a == "--seed") seed = (size_t)std::strtoull(need("--seed"), nullptr, 10);
        else if (a == "--findere") {
            const std::string v = need("--findere");
            char* end = nullptr;
            const long z = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || z < 0 || z > 7) { std::fprintf(stderr, "--findere: 0 .. 7\n"); return 1; }
            findere = (int)z;
        }
        else if (a == "--invalid-bases") {
            const std::string v = need("--invalid-bases");
            if (v == "error") invalid_bases = COBS_GPU_INVALID_ERROR;
            else if (v == "miss") invalid_bases = COBS_GPU_INVALID_MISS;
            else if (v == "skip") invalid_bases = COBS_GPU_INVALID_SKIP;
            else { std::fprintf(stderr, "--invalid-bases: error, miss or skip\n"); return 1; }
        }
        else if (a == "--positions") positions = true;
        else if (a == "--prevalence") prevalence = true;
        else if (a == "--weighted") weighted = true;
        else if (a == "--coverage") coverage = true;
        else if (a == "--window") window_arg = need("--window");
        else if (a == "--fpr-adjust") fpr_adjust = true;
        else if (a == "--sets") sets_file = need("--sets");
        else if (a == "--sets-by") sets_by = need("--sets-by");
        else if (a == "--sets-quorum") { sets_quorum = need("--sets-quorum"); have_quorum = true; }
        else if (a == "--sets-profile") sets_profile = true;
        else if (a == "--group") group = need("--group");
        else if (a == "--read-threshold") read_threshold = std::atof(need("--read-threshold"));
        else if (a == "--best") best = need("--best");
        else if (a == "--best-by-name") { best_sep = need("--best-by-name"); best_by_name = true; }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (!a.empty() && a[0] == '-') { std::fprintf(stderr, "unknown flag %s\n", a.c_str()); usage(); return 1; }
        else if (fpr_mode && index_paths.empty()) index_paths.push_back(a);
        else query_line = a;
    }
    const int device = devices.empty() ? -1 : devices[0];
    if (positions && (devices.size() > 1 || force_sharded || hbm_budget != 0)) {
        std::fprintf(stderr, "--positions: not with several devices (-d A,B / --sharded) or --hbm-budget: "
                             "the rows of a document have to be resident on one GPU\n");
        return 1;
    }
    if (prevalence && (devices.size() > 1 || force_sharded || hbm_budget != 0 || positions || fpr_adjust || !group.empty())) {
        std::fprintf(stderr, "--prevalence: not with several devices (-d A,B / --sharded) or --hbm-budget (the rows have to be "
                             "resident on one GPU), nor with --positions, --fpr-adjust or --group\n");
        return 1;
    }
    if (weighted && (devices.size() > 1 || force_sharded || hbm_budget != 0 || positions || prevalence || fpr_adjust || !group.empty())) {
        std::fprintf(stderr, "--weighted: not with several devices (-d A,B / --sharded: the weights need every shard's counts) or "
                             "--hbm-budget (the rows have to be resident on one GPU), nor with --positions, --prevalence, "
                             "--fpr-adjust or --group\n");
        return 1;
    }
    uint32_t window = 0;
    if (!window_arg.empty()) {
        char* end = nullptr;
        const unsigned long long n = std::strtoull(window_arg.c_str(), &end, 10);
        if (*end != '\0' || n == 0 || n > 4095) { std::fprintf(stderr, "--window: a number of positions, 1 .. 4095\n"); return 1; }
        window = (uint32_t)n;
        if (devices.size() > 1 || force_sharded || hbm_budget != 0 || coverage || prevalence || weighted || fpr_adjust || !group.empty() ||
            !sets_file.empty()) {
            std::fprintf(stderr, "--window: not with several devices (-d A,B / --sharded) or --hbm-budget (the rows have to be "
                                 "resident on one GPU), nor with --coverage, --prevalence, --weighted, --sets, --fpr-adjust or --group\n");
            return 1;
        }
    }
    if (coverage && (devices.size() > 1 || force_sharded || hbm_budget != 0 || positions || prevalence || weighted || fpr_adjust ||
                     !group.empty() || !sets_file.empty())) {
        std::fprintf(stderr, "--coverage: not with several devices (-d A,B / --sharded) or --hbm-budget (the rows have to be "
                             "resident on one GPU), nor with --positions, --prevalence, --weighted, --sets, --fpr-adjust or --group\n");
        return 1;
    }
    size_t best_size = 0;                    // 0 with --best all and --best-by-name
    if (!best.empty() || best_by_name) {
        char* end = nullptr;
        const unsigned long long n = std::strtoull(best.c_str(), &end, 10);
        if (!best.empty() && best != "all" && (*end != '\0' || n == 0)) { std::fprintf(stderr, "--best: a number of records > 0, or all\n"); return 1; }
        if (best_by_name && best_sep.size() != 1) { std::fprintf(stderr, "--best-by-name: one separator character\n"); return 1; }
        best_size = best.empty() || best == "all" ? 0 : (size_t)n;
        if ((!best.empty() && best_by_name) || devices.size() > 1 || force_sharded || hbm_budget != 0 || query_file.empty() || !group.empty() ||
            !sets_file.empty() || weighted || coverage || window || prevalence || positions || fpr_adjust) {
            std::fprintf(stderr, "--best / --best-by-name: one of the two; needs a query file (-f); not with several devices (-d A,B / "
                                 "--sharded) or --hbm-budget, nor with --group, --sets, --weighted, --coverage, --window, --prevalence, "
                                 "--positions or --fpr-adjust\n");
            return 1;
        }
    }
    if (!sets_by.empty() && sets_by != "any" && sets_by != "all") { std::fprintf(stderr, "--sets-by: any or all\n"); return 1; }
    if (!sets_by.empty() && sets_file.empty()) { std::fprintf(stderr, "--sets-by: needs --sets FILE.tsv\n"); return 1; }
    double quorum = 0.0;
    if (have_quorum) {
        char* end = nullptr;
        quorum = std::strtod(sets_quorum.c_str(), &end);
        if (sets_quorum.empty() || *end != '\0' || !(quorum > 0.0 && quorum <= 1.0)) { std::fprintf(stderr, "--sets-quorum: a number in (0, 1]\n"); return 1; }
        if (sets_file.empty()) { std::fprintf(stderr, "--sets-quorum: needs --sets FILE.tsv\n"); return 1; }
        if (!sets_by.empty() || sets_profile) { std::fprintf(stderr, "--sets-quorum: not with --sets-by or --sets-profile\n"); return 1; }
    }
    if (sets_profile) {
        if (sets_file.empty()) { std::fprintf(stderr, "--sets-profile: needs --sets FILE.tsv\n"); return 1; }
        if (!sets_by.empty()) { std::fprintf(stderr, "--sets-profile: not with --sets-by\n"); return 1; }
    }
    if (!sets_file.empty() && (devices.size() > 1 || force_sharded || hbm_budget != 0 || positions || prevalence || weighted ||
                               fpr_adjust || !group.empty())) {
        std::fprintf(stderr, "--sets: not with several devices (-d A,B / --sharded: any and all are not additive over shards) or "
                             "--hbm-budget (the rows have to be resident on one GPU), nor with --positions, --prevalence, "
                             "--weighted, --fpr-adjust or --group\n");
        return 1;
    }
    std::vector<std::pair<std::string, std::string>> set_rows;
    if (!sets_file.empty() && !read_sets_tsv(sets_file, set_rows)) return 1;
    const uint32_t sets_rank_by = sets_by == "all" ? COBS_GPU_SETS_BY_ALL : COBS_GPU_SETS_BY_ANY;
    size_t group_size = 0;                   // 0 with --group all
    if (fpr_adjust && (devices.size() > 1 || force_sharded || !group.empty())) {
        std::fprintf(stderr, "--fpr-adjust: not with several devices (-d A,B / --sharded: a document's filter lives on one rank) or --group\n");
        return 1;
    }
    if (!group.empty()) {
        char* end = nullptr;
        const unsigned long long n = std::strtoull(group.c_str(), &end, 10);
        if (group != "all" && (*end != '\0' || n == 0)) { std::fprintf(stderr, "--group: a number of records > 0, or all\n"); return 1; }
        group_size = group == "all" ? 0 : (size_t)n;
        if (devices.size() > 1 || force_sharded || hbm_budget != 0 || positions || query_file.empty()) {
            std::fprintf(stderr, "--group: needs a query file (-f); not with several devices (-d A,B / --sharded), --hbm-budget "
                                 "or --positions\n");
            return 1;
        }
    }
    auto open_index = [&]() -> std::unique_ptr<cobs_gpu::BatchSearch> {
        // stdout carries the results in `cobs query` format and nothing else: RCCL prints a
        // version banner there when a communicator is created, so stdout points at stderr
        // while the index is opened
        struct StdoutToStderr {
            int saved;
            StdoutToStderr() { std::fflush(stdout); saved = dup(1); dup2(2, 1); }
            ~StdoutToStderr() { std::fflush(stdout); dup2(saved, 1); close(saved); }
        } quiet;
        if (devices.size() > 1 || force_sharded) {
            auto* sh = new cobs_gpu::ShardedClassicSearch(index_paths, devices.empty() ? std::vector<int>{0} : devices, hbm_budget);
            std::unique_ptr<cobs_gpu::BatchSearch> keep(sh);
            if (findere > 0) sh->set_findere((unsigned)findere);
            if (invalid_bases != COBS_GPU_INVALID_ERROR) sh->set_invalid_bases(invalid_bases);
            return keep;
        }
        auto* cs = new cobs_gpu::ClassicSearch(index_paths, device, hbm_budget);
        std::unique_ptr<cobs_gpu::BatchSearch> keep(cs);
        if (findere > 0) cs->set_findere((unsigned)findere);
        if (invalid_bases != COBS_GPU_INVALID_ERROR) cs->set_invalid_bases(invalid_bases);
        return keep;
    };
    if (!random_out.empty()) {
        // `cobs classic-construct-random` (reference src/cobs.cpp:243-291): same flags and defaults
        const uint64_t sig = synth_rows.empty() ? 2ull * 1024 * 1024 : std::strtoull(synth_rows.c_str(), nullptr, 10);
        if (cobs_gpu_construct_random(random_out.c_str(), sig, synth_docs, document_size, synth_hashes, seed, device) != COBS_GPU_OK) {
            std::fprintf(stderr, "EXCEPTION: %s\n", cobs_gpu_last_error());
            return 1;
        }
        return 0;
    }
    if (!synth_out.empty()) {
        std::vector<uint64_t> sigs;
        for (size_t p = 0; p < synth_rows.size();) {
            size_t e = synth_rows.find(',', p);
            if (e == std::string::npos) e = synth_rows.size();
            sigs.push_back(std::strtoull(synth_rows.substr(p, e - p).c_str(), nullptr, 10));
            p = e + 1;
        }
        if (sigs.empty()) sigs.push_back(2 * 1024 * 1024);      // default of `cobs classic-construct-random -s`
        cobs_gpu_synth d{};
        d.kind = synth_compact ? 1 : 0;
        d.term_size = 31;
        d.canonicalize = 1;
        d.num_pages = (uint32_t)sigs.size();
        d.num_hashes = synth_hashes;
        d.page_size = synth_page;
        d.num_docs = synth_docs;
        d.seed = seed;
        d.signature_sizes = sigs.data();
        if (cobs_gpu_write_synthetic(&d, synth_out.c_str(), device) != COBS_GPU_OK) {
            std::fprintf(stderr, "EXCEPTION: %s\n", cobs_gpu_last_error());
            return 1;
        }
        return 0;
    }
    if (bench && !index_paths.empty()) {
        try {
            std::unique_ptr<cobs_gpu::BatchSearch> sp = open_index();
            cobs_gpu::BatchSearch& s = *sp;
            return benchmark(s, index_paths[0], num_kmers, num_queries, num_warmup, seed, dist, findere);
        } catch (const cobs_gpu::Error& e) {
            std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
            return 1;
        }
    }
    if (index_paths.empty() || (query_line.empty() && query_file.empty())) {
        if (!index_paths.empty()) std::fprintf(stderr, "Pass a verbatim query or a query file.\n");
        usage();
        return 1;
    }
    try {
        std::unique_ptr<cobs_gpu::BatchSearch> sp = open_index();
        cobs_gpu::BatchSearch& s = *sp;
        std::vector<std::string> set_names;
        if (!sets_file.empty()) label_doc_sets(dynamic_cast<cobs_gpu::ClassicSearch&>(s), set_rows, set_names);
        if (!query_line.empty() && !sets_file.empty()) {
            cobs_gpu::ClassicSearch& cs = dynamic_cast<cobs_gpu::ClassicSearch&>(s);
            if (have_quorum) print_sets_quorum(cs, {query_line}, nullptr, set_names, quorum, threshold, num_results);
            else if (sets_profile) print_sets_profile(cs, {query_line}, nullptr, set_names);
            else print_sets(cs, {query_line}, nullptr, set_names, threshold, sets_rank_by, num_results);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty() && prevalence) {
            print_prevalence(dynamic_cast<cobs_gpu::ClassicSearch&>(s), {query_line}, nullptr);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty() && coverage) {
            std::vector<std::vector<cobs_gpu::SearchResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_coverage({query_line}, results, threshold, num_results);
            for (const auto& r : results[0]) std::cout << r.doc_name << '\t' << r.score << '\n';
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty() && window) {
            print_window(dynamic_cast<cobs_gpu::ClassicSearch&>(s), {query_line}, nullptr, window, threshold, num_results, positions);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty() && weighted) {
            std::vector<std::vector<cobs_gpu::SearchResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_weighted({query_line}, results, threshold, num_results);
            for (const auto& r : results[0]) std::cout << r.doc_name << '\t' << r.score << '\n';
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty() && positions) {
            print_with_positions(dynamic_cast<cobs_gpu::ClassicSearch&>(s), {query_line}, nullptr, threshold, num_results, fpr_adjust);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!query_line.empty()) {
            std::vector<cobs_gpu::SearchResult> result;
            s.search(query_line, result, threshold, num_results);
            std::vector<cobs_gpu::ClassicSearch::Adjusted> adj;
            if (fpr_adjust) adj = adjusted_of(dynamic_cast<cobs_gpu::ClassicSearch&>(s), query_line, result);
            for (size_t i = 0; i < result.size(); ++i)
                std::cout << result[i].doc_name << '\t' << result[i].score << (fpr_adjust ? adjusted_columns(adj[i]) : std::string()) << '\n';
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        std::ifstream qf(query_file);
        if (!qf.good()) { std::fprintf(stderr, "could not open query file %s\n", query_file.c_str()); return 1; }
        std::vector<std::string> queries, comments;
        std::string line, query, comment;
        while (std::getline(qf, line)) {
            if (line.empty()) continue;
            if (line[0] == '>' || line[0] == ';') {
                if (!query.empty()) { queries.push_back(query); comments.push_back(comment); }
                line[0] = '*';
                query.clear();
                comment = line;
            } else {
                query += line;
            }
        }
        if (!query.empty()) { queries.push_back(query); comments.push_back(comment); }
        if (!sets_file.empty()) {
            cobs_gpu::ClassicSearch& cs = dynamic_cast<cobs_gpu::ClassicSearch&>(s);
            if (have_quorum) print_sets_quorum(cs, queries, &comments, set_names, quorum, threshold, num_results);
            else if (sets_profile) print_sets_profile(cs, queries, &comments, set_names);
            else print_sets(cs, queries, &comments, set_names, threshold, sets_rank_by, num_results);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (prevalence) {
            print_prevalence(dynamic_cast<cobs_gpu::ClassicSearch&>(s), queries, &comments);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (coverage) {
            std::vector<std::vector<cobs_gpu::SearchResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_coverage(queries, results, threshold, num_results);
            for (size_t q = 0; q < queries.size(); ++q) {
                std::cout << comments[q] << '\t' << results[q].size() << '\n';
                for (const auto& r : results[q]) std::cout << r.doc_name << '\t' << r.score << '\n';
            }
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (window) {
            print_window(dynamic_cast<cobs_gpu::ClassicSearch&>(s), queries, &comments, window, threshold, num_results, positions);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (weighted) {
            std::vector<std::vector<cobs_gpu::SearchResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_weighted(queries, results, threshold, num_results);
            for (size_t q = 0; q < queries.size(); ++q) {
                std::cout << comments[q] << '\t' << results[q].size() << '\n';
                for (const auto& r : results[q]) std::cout << r.doc_name << '\t' << r.score << '\n';
            }
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!group.empty()) {
            std::vector<size_t> offs{0};
            const size_t step = group_size ? group_size : std::max<size_t>(queries.size(), 1);
            for (size_t q = 0; q < queries.size(); q += step) offs.push_back(std::min(q + step, queries.size()));
            std::vector<std::vector<cobs_gpu::ClassicSearch::GroupResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_groups(queries, offs, results, threshold, read_threshold, num_results);
            for (size_t g = 0; g + 1 < offs.size(); ++g) {
                std::cout << comments[offs[g]] << '\t' << results[g].size() << '\n';
                for (const auto& r : results[g]) std::cout << r.doc_name << '\t' << r.score << '\t' << r.votes << '\n';
            }
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (!best.empty() || best_by_name) {
            // a record's name: its comment line without the marker, up to the first blank
            std::vector<std::string> names;
            for (const std::string& c : comments) {
                const std::string s = c.empty() ? c : c.substr(1);
                names.push_back(s.substr(0, s.find_first_of(" \t")));
            }
            std::vector<size_t> offs{0};
            std::vector<std::string> labels;
            if (best_by_name) {
                auto prefix = [&](const std::string& s) { const size_t p = s.rfind(best_sep[0]); return p == std::string::npos ? s : s.substr(0, p); };
                for (size_t q = 0; q < queries.size(); ++q) {
                    const bool open = names[q].find(best_sep[0]) != std::string::npos;
                    if (q > 0 && open && names[q - 1].find(best_sep[0]) != std::string::npos && prefix(names[q]) == labels.back()) continue;
                    if (q > 0) offs.push_back(q);
                    labels.push_back(prefix(names[q]));
                }
                if (!queries.empty()) offs.push_back(queries.size());
                for (std::string& l : labels) l = "*" + l;
            } else {
                const size_t step = best_size ? best_size : std::max<size_t>(queries.size(), 1);
                for (size_t q = 0; q < queries.size(); q += step) {
                    labels.push_back(comments[q]);
                    offs.push_back(std::min(q + step, queries.size()));
                }
            }
            std::vector<std::vector<cobs_gpu::ClassicSearch::BestResult>> results;
            dynamic_cast<cobs_gpu::ClassicSearch&>(s).search_best(queries, offs, results, threshold, num_results);
            for (size_t g = 0; g + 1 < offs.size(); ++g) {
                std::cout << labels[g] << '\t' << results[g].size() << '\n';
                for (const auto& r : results[g])
                    std::cout << r.doc_name << '\t' << names[r.query] << '\t' << r.score << '\t' << r.positions << '\t' << r.ties << '\n';
            }
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        if (positions) {
            print_with_positions(dynamic_cast<cobs_gpu::ClassicSearch&>(s), queries, &comments, threshold, num_results, fpr_adjust);
            std::cout.flush();
            print_timer(s);
            return 0;
        }
        std::vector<std::vector<cobs_gpu::SearchResult>> results;
        s.search_batch(queries, results, threshold, num_results);
        for (size_t q = 0; q < queries.size(); ++q) {
            std::cout << comments[q] << '\t' << results[q].size() << '\n';
            std::vector<cobs_gpu::ClassicSearch::Adjusted> adj;
            if (fpr_adjust) adj = adjusted_of(dynamic_cast<cobs_gpu::ClassicSearch&>(s), queries[q], results[q]);
            for (size_t i = 0; i < results[q].size(); ++i)
                std::cout << results[q][i].doc_name << '\t' << results[q][i].score
                          << (fpr_adjust ? adjusted_columns(adj[i]) : std::string()) << '\n';
        }
        std::cout.flush();
        print_timer(s);
    } catch (const cobs_gpu::Error& e) {
        // the reference prints "EXCEPTION: ..." and returns -1 (src/cobs.cpp:1070-1076) or exits
        std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
        return 1;
    }
    return 0;
}
