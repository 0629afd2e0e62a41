// include/cobs_gpu_search.hpp -- C++17 host-side mirror of the reference's operator
// API for the query path, implemented over the C ABI of cobs_gpu.h (header only).
//
// Reference interface being mirrored:
//   struct cobs::SearchResult { const char* doc_name; uint32_t score; }   (cobs/query/search.hpp:17-27)
//   class  cobs::Search { virtual void search(const std::string& query,
//                std::vector<SearchResult>& result, double threshold = 0.0,
//                size_t num_results = 0) = 0; }                            (cobs/query/search.hpp:29-47)
//   class  cobs::ClassicSearch : Search { ClassicSearch(std::string path); ... } (classic_search.hpp:19-37)
//   class  cobs::IndexSearchFile, ClassicIndexMMapSearchFile(path), CompactIndexMMapSearchFile(path) and
//          ClassicSearch(std::shared_ptr<IndexSearchFile>), ClassicSearch(std::vector<std::shared_ptr<...>>)
//          (cobs/query/index_file.hpp:19-49, */mmap_search_file.hpp, classic_search.cpp:41-49)
//
// Same names, argument meaning and defaults.  Differences, all at the error
// boundary: where the reference terminates the process (exit/abort on a short
// query, a non-ACGT base, an unreadable index: classic_search.cpp:431-433, :93-96,
// :61-63) this class throws cobs_gpu::Error carrying the C-ABI status.
// `result` is caller-owned, resized and overwritten (classic_search.cpp:147,190);
// SearchResult::doc_name points into strings owned by the Search object.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "cobs_gpu.h"
#include "cobs_gpu_batch.h"      // cobs_gpu_search_batch_view

namespace cobs_gpu {

struct SearchResult {
    //! string reference to document name (owned by the index handle)
    const char* doc_name = nullptr;
    //! score (number of matched k-mers)
    uint32_t score = 0;
    SearchResult() = default;
    SearchResult(const char* name, uint32_t s) : doc_name(name), score(s) {}
};

class Error : public std::runtime_error {
public:
    Error(cobs_gpu_status st, const std::string& msg) : std::runtime_error(msg), status(st) {}
    cobs_gpu_status status;
};

//! The query bases covered by the set positions of one cobs_gpu_hit_positions bitmap of n positions (a set position
//! covers span = term size + findere bases): what ClassicSearch::search_coverage scores the document with.  Host
//! arithmetic (cobs_gpu_covered_bases); Error(COBS_GPU_ERR_ARG) when words is too short for n.
inline uint64_t covered_bases(const std::vector<uint64_t>& words, size_t n, uint32_t span) {
    if (n > words.size() * 64) throw Error(COBS_GPU_ERR_ARG, "covered_bases: words holds fewer than n positions");
    return cobs_gpu_covered_bases(words.data(), n, span);
}

//! The largest number of set positions in any min(window, n) consecutive positions of one cobs_gpu_hit_positions bitmap
//! of n positions, and (start, optional) the smallest start that reaches it: what ClassicSearch::search_window scores
//! the document with.  Host arithmetic (cobs_gpu_best_window); Error(COBS_GPU_ERR_ARG) when words is too short for n.
inline uint32_t best_window(const std::vector<uint64_t>& words, size_t n, uint32_t window, size_t* start = nullptr) {
    if (n > words.size() * 64) throw Error(COBS_GPU_ERR_ARG, "best_window: words holds fewer than n positions");
    return cobs_gpu_best_window(words.data(), n, window, start);
}

//! The reference's Search carries a public `Timer timer_` with an accessor `timer()` (cobs/query/search.hpp:35-46,
//! cobs/util/timer.hpp:19-55) that its callers read and reset: `s.timer().print("search")` (src/cobs.cpp:468),
//! `s.timer().reset()` and `cobs::Timer t = s.timer(); t.get("hashes") ...` in benchmark_fpr_run (:623, :644-661).
//! Same shape here, over the handle's phase timers (cobs_gpu_timers): get(name), reset(), print(info[, os]); a COPY is a
//! snapshot (the reference copies the object to read it).  Names: the engine's own -- "hashes" (K1), "h2d" (query text),
//! "scan" (K2: row gather + AND + count, ONE kernel), "d2h", "rank" -- and the reference's, so that its callers compile
//! and print unchanged: "io" = the scan kernel (it is bound by the row gather the reference times as io), "and rows" and
//! "add rows" = 0 (inside that kernel), "sort results" = d2h + rank.  An unknown name reads 0, as a fresh entry of the
//! reference's timer does (timer.cpp:61-63).
class Timer {
public:
    Timer() = default;
    Timer(const Timer& o) { o.read(snap_); frozen_ = true; }
    Timer& operator=(const Timer& o) {
        if (this != &o) { o.read(snap_); frozen_ = true; ix_ = nullptr; }
        return *this;
    }
    //! (the Search object that owns this timer names its index handle once it is open)
    void bind(cobs_gpu_index* ix) { ix_ = ix; frozen_ = false; }
    void reset() {
        if (ix_ && !frozen_) (void)cobs_gpu_timers(ix_, nullptr, 1);
        for (double& v : snap_) v = 0;
    }
    double get(const char* name) const {
        double t[5];
        read(t);
        const std::string n(name ? name : "");
        if (n == "hashes") return t[0];
        if (n == "h2d") return t[1];
        if (n == "scan" || n == "io") return t[2];
        if (n == "d2h") return t[3];
        if (n == "rank") return t[4];
        if (n == "sort results") return t[3] + t[4];
        if (n == "total") return t[0] + t[1] + t[2] + t[3] + t[4];
        return 0.0;
    }
    //! "TIMER info=<info> name=seconds ... total=seconds" (timer.cpp:77-85)
    void print(const char* info, std::ostream& os) const {
        double t[5];
        read(t);
        os << "TIMER info=" << info << " hashes=" << t[0] << " h2d=" << t[1] << " scan=" << t[2] << " d2h=" << t[3]
           << " rank=" << t[4] << " total=" << t[0] + t[1] + t[2] + t[3] + t[4] << std::endl;
    }
    void print(const char* info) const { print(info, std::cerr); }

private:
    void read(double out[5]) const {
        for (int i = 0; i < 5; ++i) out[i] = snap_[i];
        if (ix_ && !frozen_) (void)cobs_gpu_timers(ix_, out, 0);
    }
    cobs_gpu_index* ix_ = nullptr;
    bool frozen_ = false;
    double snap_[5] = {0, 0, 0, 0, 0};
};

class Search {
public:
    virtual ~Search() = default;
    //! Returns timer_ (cobs/query/search.hpp:35-38)
    Timer& timer() { return timer_; }
    const Timer& timer() const { return timer_; }
    virtual void search(const std::string& query, std::vector<SearchResult>& result,
                        double threshold = 0.0, size_t num_results = 0) = 0;

public:
    //! timer of different query phases
    Timer timer_;
};

//! Search plus the batch call (the performance path; the reference loops queries serially)
class BatchSearch : public Search {
public:
    virtual void search_batch(const std::vector<std::string>& queries,
                              std::vector<std::vector<SearchResult>>& results,
                              double threshold = 0.0, size_t num_results = 0) = 0;
    //! the index handle timers / geometry are read from (rank 0 of a sharded search)
    virtual cobs_gpu_index* handle() const = 0;
};

//! The reference hands ClassicSearch its index files as objects (cobs/query/index_file.hpp:19-49) made from a path
//! by the class of their kind, which refuses a file of the other kind when it reads the header
//! (classic_index/mmap_search_file.cpp:21-25, compact_index/mmap_search_file.cpp:20-27).  Here such an object is
//! the checked NAME of a file: the engine maps and stages it when a ClassicSearch is made from it.
class IndexSearchFile {
public:
    virtual ~IndexSearchFile() = default;
    const std::string& path() const { return path_; }

protected:
    IndexSearchFile(const std::string& path, const char* kind_word) : path_(path) {
        // every index file starts with "COBS:" and the word of its kind (cobs/file/header.cpp)
        const std::string want = std::string("COBS:") + kind_word;
        char head[32] = {0};
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw Error(COBS_GPU_ERR_OPEN, "cannot open index file " + path);
        const size_t got = std::fread(head, 1, want.size(), f);
        std::fclose(f);
        if (got != want.size() || std::memcmp(head, want.data(), want.size()) != 0)
            throw Error(COBS_GPU_ERR_FORMAT, path + " is not a " + kind_word + " file");
    }

private:
    std::string path_;
};

class ClassicIndexMMapSearchFile : public IndexSearchFile {
public:
    explicit ClassicIndexMMapSearchFile(const std::string& path) : IndexSearchFile(path, "CLASSIC_INDEX") {}
};

class CompactIndexMMapSearchFile : public IndexSearchFile {
public:
    explicit CompactIndexMMapSearchFile(const std::string& path) : IndexSearchFile(path, "COMPACT_INDEX") {}
};

class ClassicSearch : public BatchSearch {
public:
    //! one index file object / several, searched together (classic_search.cpp:41-49)
    explicit ClassicSearch(const std::shared_ptr<IndexSearchFile>& index, int device = -1, uint64_t hbm_budget_bytes = 0)
        : ClassicSearch(std::vector<std::string>{index->path()}, device, hbm_budget_bytes) {}
    explicit ClassicSearch(const std::vector<std::shared_ptr<IndexSearchFile>>& indices, int device = -1,
                           uint64_t hbm_budget_bytes = 0)
        : ClassicSearch(paths_of(indices), device, hbm_budget_bytes) {}

    //! auto-detect classic / compact and stage the index into HBM
    //! hbm_budget_bytes > 0: an index larger than the budget is streamed chunk-wise at every
    //! search (the role of the reference's mmap / AIO back-ends for indexes beyond memory)
    explicit ClassicSearch(const std::string& path, int device = -1, uint64_t hbm_budget_bytes = 0)
        : ClassicSearch(std::vector<std::string>{path}, device, hbm_budget_bytes) {}

    //! several index files searched together (reference: vector<shared_ptr<IndexSearchFile>>)
    explicit ClassicSearch(const std::vector<std::string>& paths, int device = -1,
                           uint64_t hbm_budget_bytes = 0) {
        std::vector<const char*> cp;
        for (const auto& p : paths) cp.push_back(p.c_str());
        cobs_gpu_options o{};
        o.struct_size = sizeof o;
        o.device = device;
        o.hbm_budget_bytes = hbm_budget_bytes;
        check(cobs_gpu_open(cp.data(), cp.size(), &o, &ix_));
        timer_.bind(ix_);
    }

    //! adopt an index handle that is already open (e.g. built by cobs_gpu_build_index_list)
    explicit ClassicSearch(cobs_gpu_index* adopted) : ix_(adopted) { timer_.bind(ix_); }

    ~ClassicSearch() override { cobs_gpu_close(ix_); }
    ClassicSearch(const ClassicSearch&) = delete;
    ClassicSearch& operator=(const ClassicSearch&) = delete;
    ClassicSearch(ClassicSearch&& o) noexcept : ix_(o.ix_), hits_(std::move(o.hits_)) {
        o.ix_ = nullptr;
        o.timer_.bind(nullptr);
        timer_.bind(ix_);
    }

    void search(const std::string& query, std::vector<SearchResult>& result,
                double threshold = 0.0, size_t num_results = 0) final {
        size_t n = 0;
        const size_t total = (size_t)cobs_gpu_total_counts(ix_);
        hits_.resize(num_results == 0 || num_results > total ? total : num_results);
        check(cobs_gpu_search(ix_, query.data(), query.size(), threshold, num_results,
                              hits_.data(), hits_.size(), &n));
        result.resize(n);
        for (size_t i = 0; i < n; ++i)
            result[i] = SearchResult(cobs_gpu_doc_name(ix_, hits_[i].file_no, hits_[i].doc), hits_[i].score);
    }

    //! many queries in one device pass (the performance path; the reference loops serially)
    void search_batch(const std::vector<std::string>& queries,
                      std::vector<std::vector<SearchResult>>& results,
                      double threshold = 0.0, size_t num_results = 0) override {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        std::vector<size_t> offs(queries.size() + 1, 0);
        const size_t total = (size_t)cobs_gpu_total_counts(ix_);
        // hit buffer: exact when the result count is known (a limit, or threshold 0 = every
        // document); with a threshold start small and grow to the size the library reports
        size_t cap;
        if (num_results > 0) cap = (num_results > total ? total : num_results) * queries.size();
        else if (threshold <= 0.0) cap = total * queries.size();
        else cap = 1;                                    // (thresholded without a limit: the view call below)
        size_t bad = 0;
        cobs_gpu_status st;
        if (threshold > 0.0 && num_results == 0) {
            // the number of hits is not known beforehand: collected in the arena the library grows as the passes come
            // home (cobs_gpu_batch.h) -- into a vector of a guessed size the whole search could have to run twice
            const cobs_gpu_hit* vh = nullptr;
            const size_t* vo = nullptr;
            check(cobs_gpu_search_batch_view(ix_, qp.data(), ql.data(), queries.size(), threshold, 0, &vh, &vo, &bad));
            results.resize(queries.size());
            for (size_t q = 0; q < queries.size(); ++q) {
                results[q].resize(vo[q + 1] - vo[q]);
                for (size_t i = vo[q]; i < vo[q + 1]; ++i)
                    results[q][i - vo[q]] = SearchResult(cobs_gpu_doc_name(ix_, vh[i].file_no, vh[i].doc), vh[i].score);
            }
            return;
        }
        for (;;) {
            hits_.resize(cap + 1);
            st = cobs_gpu_search_batch(ix_, qp.data(), ql.data(), queries.size(), threshold,
                                       num_results, hits_.data(), hits_.size(), offs.data(), &bad);
            if (st == COBS_GPU_ERR_CAPACITY && offs[queries.size()] > cap) {
                cap = offs[queries.size()];        // needed size, as documented in cobs_gpu.h
                continue;
            }
            break;
        }
        check(st);
        results.resize(queries.size());
        for (size_t q = 0; q < queries.size(); ++q) {
            results[q].resize(offs[q + 1] - offs[q]);
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q][i - offs[q]] =
                    SearchResult(cobs_gpu_doc_name(ix_, hits_[i].file_no, hits_[i].doc), hits_[i].score);
        }
    }

    cobs_gpu_index* handle() const override { return ix_; }

    //! search() plus WHERE in the query each result matched (beyond the reference; cobs_gpu_hit_positions):
    //! positions[i] holds the words of result[i] -- position p of the query's n = T - z positions is bit p % 64 of word
    //! p / 64, set when the terms p .. p + z are all present in the document; their popcount is result[i].score
    void search_positions(const std::string& query, std::vector<SearchResult>& result,
                          std::vector<std::vector<uint64_t>>& positions, double threshold = 0.0, size_t num_results = 0) {
        std::vector<std::vector<SearchResult>> rs;
        std::vector<std::vector<std::vector<uint64_t>>> ps;
        search_batch_positions({query}, rs, ps, threshold, num_results);
        result = std::move(rs[0]);
        positions = std::move(ps[0]);
    }

    //! ... for many queries: positions[q] is parallel to results[q]; num_positions (optional) receives every result's
    //! n = T - z, which depends on the term size of the index file that holds the document
    void search_batch_positions(const std::vector<std::string>& queries, std::vector<std::vector<SearchResult>>& results,
                                std::vector<std::vector<std::vector<uint64_t>>>& positions, double threshold = 0.0,
                                size_t num_results = 0, std::vector<std::vector<size_t>>* num_positions = nullptr) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        const cobs_gpu_hit* vh = nullptr;
        const size_t* vo = nullptr;
        size_t bad = 0, need = 0;
        // (the hits stay in the library's arena, which the positions call reads them from: it is not a search call)
        check(cobs_gpu_search_batch_view(ix_, qp.data(), ql.data(), nq, threshold, num_results, &vh, &vo, &bad));
        std::vector<size_t> bo(vo[nq] + 1, 0);
        std::vector<uint64_t> bits;
        cobs_gpu_status st = cobs_gpu_hit_positions(ix_, qp.data(), ql.data(), nq, vh, vo, nullptr, 0, bo.data(), &need, &bad);
        if (st == COBS_GPU_ERR_CAPACITY && need > 0) {       // the size is host arithmetic: nothing has run yet
            bits.resize(need);
            st = cobs_gpu_hit_positions(ix_, qp.data(), ql.data(), nq, vh, vo, bits.data(), bits.size(), bo.data(), &need, &bad);
        }
        check(st);
        std::vector<size_t> term_size(cobs_gpu_num_files(ix_));
        for (size_t f = 0; f < term_size.size(); ++f) {
            cobs_gpu_index_info info;
            check(cobs_gpu_info(ix_, f, &info));
            term_size[f] = info.term_size;
        }
        const size_t z = findere();
        results.resize(nq);
        positions.resize(nq);
        if (num_positions) num_positions->assign(nq, {});
        for (size_t q = 0; q < nq; ++q) {
            results[q].resize(vo[q + 1] - vo[q]);
            positions[q].resize(vo[q + 1] - vo[q]);
            for (size_t i = vo[q]; i < vo[q + 1]; ++i) {
                if (num_positions) (*num_positions)[q].push_back(ql[q] - term_size[vh[i].file_no] + 1 - z);
                results[q][i - vo[q]] = SearchResult(cobs_gpu_doc_name(ix_, vh[i].file_no, vh[i].doc), vh[i].score);
                positions[q][i - vo[q]].assign(bits.begin() + bo[i], bits.begin() + bo[i + 1]);
            }
        }
    }

    //! for every position of every query, how many documents hold it (beyond the reference; cobs_gpu_prevalence): segment
    //! (q, f) of file f is counts[offsets[q * n_files + f] .. offsets[q * n_files + f + 1]), one count per position of the
    //! query's n = T_f - z; on one shard of several the documents of the shard's own slots (the parts add up)
    void prevalence(const std::vector<std::string>& queries, std::vector<uint32_t>& counts, std::vector<size_t>& offsets) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        offsets.assign(nq * cobs_gpu_num_files(ix_) + 1, 0);
        counts.clear();
        size_t bad = 0, need = 0;
        cobs_gpu_status st = cobs_gpu_prevalence(ix_, qp.data(), ql.data(), nq, nullptr, 0, offsets.data(), &need, &bad);
        if (st == COBS_GPU_ERR_CAPACITY && need > 0) {       // the size is host arithmetic: nothing has run yet
            counts.resize(need);
            st = cobs_gpu_prevalence(ix_, qp.data(), ql.data(), nq, counts.data(), counts.size(), offsets.data(), &need, &bad);
        }
        check(st);
    }

    //! IDF-weighted search (beyond the reference; cobs_gpu_search_weighted): a position held by c of a file's D documents
    //! weighs 1 + min(14, floor(log2(D / c))) (0 for c = 0), a document scores the sum of the weights of the positions it
    //! holds and is a hit when that reaches max(1, ceil(threshold * W)); results[q] is ordered by score descending, then
    //! (file, document).  total_weight (optional) receives W, [query][file].
    void search_weighted(const std::vector<std::string>& queries, std::vector<std::vector<SearchResult>>& results,
                         double threshold = 0.0, size_t num_results = 0,
                         std::vector<std::vector<uint64_t>>* total_weight = nullptr) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size(), nf = cobs_gpu_num_files(ix_);
        std::vector<size_t> offs(nq + 1, 0);
        std::vector<uint64_t> tw(nq * nf + 1, 0);
        std::vector<cobs_gpu_hit> hits(16 * nq + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_weighted(ix_, qp.data(), ql.data(), nq, threshold, num_results, hits.data(), hits.size(),
                                          offs.data(), tw.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[nq] <= hits.size()) break;
            hits.resize(offs[nq]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(nq, {});
        if (total_weight) total_weight->assign(nq, {});
        for (size_t q = 0; q < nq; ++q) {
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q].push_back(SearchResult(cobs_gpu_doc_name(ix_, hits[i].file_no, hits[i].doc), hits[i].score));
            if (total_weight) (*total_weight)[q].assign(tw.begin() + q * nf, tw.begin() + (q + 1) * nf);
        }
    }

    //! one set of documents of a set result: the positions at least one member holds, and the positions every member holds
    struct SetResult {
        uint32_t file_no, set, any, all;
    };

    //! label the documents of a file with sets (beyond the reference; cobs_gpu_set_doc_sets): labels[d] is a set number
    //! below n_sets or COBS_GPU_NO_SET, one entry per document of the file; the labels replace earlier ones
    void set_doc_sets(const std::vector<uint32_t>& labels, uint32_t n_sets, size_t file_no = 0) {
        if (labels.empty()) throw Error(COBS_GPU_ERR_ARG, "set_doc_sets needs one label per document (clear_doc_sets takes labels away)");
        check(cobs_gpu_set_doc_sets(ix_, file_no, labels.data(), labels.size(), n_sets));
    }
    //! ... and take them away again
    void clear_doc_sets(size_t file_no = 0) { check(cobs_gpu_set_doc_sets(ix_, file_no, nullptr, 0, 0)); }

    //! score every query against every non-empty set of every labelled file (cobs_gpu_search_sets): results[q] holds the
    //! sets whose key -- any, or all with rank_by = COBS_GPU_SETS_BY_ALL -- reaches max(1, ceil(threshold * P)), by key
    //! descending, then the other count descending, then (file, set)
    void search_sets(const std::vector<std::string>& queries, std::vector<std::vector<SetResult>>& results,
                     double threshold = 0.0, uint32_t rank_by = COBS_GPU_SETS_BY_ANY, size_t num_results = 0) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        std::vector<size_t> offs(nq + 1, 0);
        std::vector<cobs_gpu_set_hit> hits(16 * nq + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_sets(ix_, qp.data(), ql.data(), nq, threshold, rank_by, num_results, hits.data(), hits.size(),
                                      offs.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[nq] <= hits.size()) break;
            hits.resize(offs[nq]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(nq, {});
        for (size_t q = 0; q < nq; ++q)
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q].push_back(SetResult{hits[i].file_no, hits[i].set, hits[i].any, hits[i].all});
    }

    //! one set of documents of a quorum result: the positions at least need(set) members hold, and the positions at least
    //! one member holds
    struct SetQuorumResult {
        uint32_t file_no, set, core, any;
    };

    //! the soft core of every non-empty set of every labelled file (cobs_gpu_search_sets_quorum): results[q] holds the sets
    //! whose core -- the positions at least max(1, ceil(quorum * members)) members hold, 0 < quorum <= 1 -- reaches
    //! max(1, ceil(threshold * P)), by core descending, then any descending, then (file, set)
    void search_sets_quorum(const std::vector<std::string>& queries, std::vector<std::vector<SetQuorumResult>>& results,
                            double quorum, double threshold = 0.0, size_t num_results = 0) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        std::vector<size_t> offs(nq + 1, 0);
        std::vector<cobs_gpu_set_quorum_hit> hits(16 * nq + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_sets_quorum(ix_, qp.data(), ql.data(), nq, threshold, quorum, num_results, hits.data(),
                                             hits.size(), offs.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[nq] <= hits.size()) break;
            hits.resize(offs[nq]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(nq, {});
        for (size_t q = 0; q < nq; ++q)
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q].push_back(SetQuorumResult{hits[i].file_no, hits[i].set, hits[i].core, hits[i].any});
    }

    //! how many members of every set hold each position of every query (cobs_gpu_set_prevalence): segment (q, f) is
    //! counts[offsets[q * n_files + f] .. offsets[q * n_files + f + 1]), the file's non-empty sets (ascending set number) x
    //! the query's n = T_f - z positions, set-major; empty for a file without labels
    void set_prevalence(const std::vector<std::string>& queries, std::vector<uint32_t>& counts, std::vector<size_t>& offsets) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        offsets.assign(nq * cobs_gpu_num_files(ix_) + 1, 0);
        counts.clear();
        size_t bad = 0, need = 0;
        cobs_gpu_status st = cobs_gpu_set_prevalence(ix_, qp.data(), ql.data(), nq, nullptr, 0, offsets.data(), &need, &bad);
        if (st == COBS_GPU_ERR_CAPACITY && need > 0) {       // the size is host arithmetic: nothing has run yet
            counts.resize(need);
            st = cobs_gpu_set_prevalence(ix_, qp.data(), ql.data(), nq, counts.data(), counts.size(), offsets.data(), &need, &bad);
        }
        check(st);
    }

    //! Coverage search (beyond the reference; cobs_gpu_search_coverage): a document scores the query bases that lie inside
    //! a set position (term size + findere bases from the position on) and is a hit when that reaches
    //! max(1, ceil(threshold * query length)); results[q] is ordered by coverage descending, then (file, document), and
    //! SearchResult::score carries the covered bases.
    void search_coverage(const std::vector<std::string>& queries, std::vector<std::vector<SearchResult>>& results,
                         double threshold = 0.0, size_t num_results = 0) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        std::vector<size_t> offs(nq + 1, 0);
        std::vector<cobs_gpu_hit> hits(16 * nq + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_coverage(ix_, qp.data(), ql.data(), nq, threshold, num_results, hits.data(), hits.size(),
                                          offs.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[nq] <= hits.size()) break;
            hits.resize(offs[nq]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(nq, {});
        for (size_t q = 0; q < nq; ++q)
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q].push_back(SearchResult(cobs_gpu_doc_name(ix_, hits[i].file_no, hits[i].doc), hits[i].score));
    }

    //! Window search (beyond the reference; cobs_gpu_search_window): a document scores the largest number of set positions
    //! in any w = min(window, the query's positions) consecutive positions of the query and is a hit when that reaches
    //! max(1, ceil(threshold * w)); results[q] is ordered by that number descending, then (file, document), and
    //! SearchResult::score carries it.  window: 1 .. 4095.  positions (optional) receives the cobs_gpu_hit_positions words
    //! of every result and num_positions its n, parallel to results[q]: best_window over them gives the window's start.
    void search_window(const std::vector<std::string>& queries, uint32_t window, std::vector<std::vector<SearchResult>>& results,
                       double threshold = 0.0, size_t num_results = 0,
                       std::vector<std::vector<std::vector<uint64_t>>>* positions = nullptr,
                       std::vector<std::vector<size_t>>* num_positions = nullptr) {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t nq = queries.size();
        std::vector<size_t> offs(nq + 1, 0);
        std::vector<cobs_gpu_hit> hits(16 * nq + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_window(ix_, qp.data(), ql.data(), nq, window, threshold, num_results, hits.data(), hits.size(),
                                        offs.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[nq] <= hits.size()) break;
            hits.resize(offs[nq]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(nq, {});
        for (size_t q = 0; q < nq; ++q)
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q].push_back(SearchResult(cobs_gpu_doc_name(ix_, hits[i].file_no, hits[i].doc), hits[i].score));
        if (!positions) return;
        std::vector<size_t> bo(offs[nq] + 1, 0);
        std::vector<uint64_t> bits;
        size_t need = 0;
        st = cobs_gpu_hit_positions(ix_, qp.data(), ql.data(), nq, hits.data(), offs.data(), nullptr, 0, bo.data(), &need, &bad);
        if (st == COBS_GPU_ERR_CAPACITY && need > 0) {       // the size is host arithmetic: nothing has run yet
            bits.resize(need);
            st = cobs_gpu_hit_positions(ix_, qp.data(), ql.data(), nq, hits.data(), offs.data(), bits.data(), bits.size(), bo.data(),
                                        &need, &bad);
        }
        check(st);
        const size_t z = findere();
        positions->assign(nq, {});
        if (num_positions) num_positions->assign(nq, {});
        for (size_t q = 0; q < nq; ++q)
            for (size_t i = offs[q]; i < offs[q + 1]; ++i) {
                (*positions)[q].emplace_back(bits.begin() + bo[i], bits.begin() + bo[i + 1]);
                if (num_positions) {
                    cobs_gpu_index_info info;
                    check(cobs_gpu_info(ix_, hits[i].file_no, &info));
                    (*num_positions)[q].push_back(ql[q] - info.term_size + 1 - z);
                }
            }
    }

    //! one document of a group's result: the sum of the scores of the group's queries and how many of them it was a hit of
    struct GroupResult {
        const char* doc_name;
        uint32_t score, votes;
    };

    //! which documents a SET of queries comes from (beyond the reference; cobs_gpu_search_groups): group g is the queries
    //! [group_offsets[g], group_offsets[g + 1]); results[g] holds the documents whose summed score reaches
    //! max(1, ceil(threshold * P)), by score descending, then (file, document); votes counts the group's queries that
    //! reach read_threshold in the document.  positions (optional) receives P, [group][file].
    void search_groups(const std::vector<std::string>& queries, const std::vector<size_t>& group_offsets,
                       std::vector<std::vector<GroupResult>>& results, double threshold = 0.0, double read_threshold = 0.0,
                       size_t num_results = 0, std::vector<std::vector<uint64_t>>* positions = nullptr) {
        if (group_offsets.empty()) throw Error(COBS_GPU_ERR_ARG, "group_offsets needs n_groups + 1 entries");
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t ng = group_offsets.size() - 1, nf = cobs_gpu_num_files(ix_);
        std::vector<size_t> offs(ng + 1, 0);
        std::vector<uint64_t> pos(ng * nf + 1, 0);
        std::vector<cobs_gpu_group_hit> hits(16 * ng + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_groups(ix_, qp.data(), ql.data(), queries.size(), group_offsets.data(), ng, threshold,
                                        read_threshold, num_results, hits.data(), hits.size(), offs.data(), pos.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[ng] <= hits.size()) break;
            hits.resize(offs[ng]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(ng, {});
        if (positions) positions->assign(ng, {});
        for (size_t g = 0; g < ng; ++g) {
            for (size_t i = offs[g]; i < offs[g + 1]; ++i)
                results[g].push_back(GroupResult{cobs_gpu_doc_name(ix_, hits[i].file_no, hits[i].doc), hits[i].score, hits[i].votes});
            if (positions) (*positions)[g].assign(pos.begin() + g * nf, pos.begin() + (g + 1) * nf);
        }
    }

    //! one document of a group's result: the group's best query in it (its index in the call), that query's score and the
    //! positions the score is out of, and how many of the group's queries fit equally well (the best one included)
    struct BestResult {
        const char* doc_name;
        uint32_t file_no, doc, query, score, positions, ties;
    };

    //! every document's best query of a group (beyond the reference; cobs_gpu_search_best): group g is the queries
    //! [group_offsets[g], group_offsets[g + 1]); results[g] holds the documents whose best query reaches
    //! max(1, ceil(threshold * its positions)), by score / positions descending, then score, then (file, document)
    void search_best(const std::vector<std::string>& queries, const std::vector<size_t>& group_offsets,
                     std::vector<std::vector<BestResult>>& results, double threshold = 0.0, size_t num_results = 0) {
        if (group_offsets.empty()) throw Error(COBS_GPU_ERR_ARG, "group_offsets needs n_groups + 1 entries");
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        const size_t ng = group_offsets.size() - 1;
        std::vector<size_t> offs(ng + 1, 0);
        std::vector<cobs_gpu_best_hit> hits(16 * ng + 1024);
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            st = cobs_gpu_search_best(ix_, qp.data(), ql.data(), queries.size(), group_offsets.data(), ng, threshold, num_results,
                                      hits.data(), hits.size(), offs.data(), &bad);
            if (st != COBS_GPU_ERR_CAPACITY || offs[ng] <= hits.size()) break;
            hits.resize(offs[ng]);          // (the call reported the needed size)
        }
        check(st);
        results.assign(ng, {});
        for (size_t g = 0; g < ng; ++g)
            for (size_t i = offs[g]; i < offs[g + 1]; ++i)
                results[g].push_back(BestResult{cobs_gpu_doc_name(ix_, hits[i].file_no, hits[i].doc), hits[i].file_no, hits[i].doc,
                                                hits[i].query, hits[i].score, hits[i].positions, hits[i].ties});
    }

    //! the bits set in every document's Bloom filter (beyond the reference; cobs_gpu_doc_bits): one entry per score slot
    //! this handle holds of the file, counted on the device on the first request and cached by the library
    std::vector<uint64_t> doc_bits(size_t file_no = 0) {
        size_t need = 0;
        const cobs_gpu_status st = cobs_gpu_doc_bits(ix_, file_no, nullptr, 0, &need);
        if (st != COBS_GPU_ERR_CAPACITY) check(st);
        std::vector<uint64_t> bits(need);
        check(cobs_gpu_doc_bits(ix_, file_no, bits.data(), bits.size(), &need));
        return bits;
    }

    //! fill ratio bits / S_p of every REAL document of a file (an unsharded handle: document d is score slot d)
    std::vector<double> doc_fill(size_t file_no = 0) {
        const std::vector<uint64_t> bits = doc_bits(file_no);
        const cobs_gpu_index_info info = whole_file_info(file_no);
        std::vector<double> fill(info.num_docs);
        for (uint64_t d = 0; d < info.num_docs; ++d)
            fill[d] = (double)bits[d] / (double)cobs_gpu_signature_size(ix_, file_no, page_of(info, d));
        return fill;
    }

    //! document similarity (beyond the reference; cobs_gpu_doc_shared_bits): for every reference document refs[i] of the
    //! file, in how many rows it and every document of ITS sub-index both have their bit set -- one vector per reference,
    //! one entry per score slot of that sub-index in slot order (classic: counts_size entries; compact: 8 * page_size;
    //! the reference's own entry = its doc_bits).  Documents of different sub-indexes are not comparable and never paired.
    std::vector<std::vector<uint64_t>> doc_shared_bits(const std::vector<uint32_t>& refs, size_t file_no = 0) {
        std::vector<uint64_t> offs(refs.size() + 1, 0);
        size_t need = 0;
        check(cobs_gpu_doc_shared_bits(ix_, file_no, refs.data(), refs.size(), offs.data(), nullptr, 0, &need));
        std::vector<uint64_t> cells(need);
        check(cobs_gpu_doc_shared_bits(ix_, file_no, refs.data(), refs.size(), offs.data(), cells.data(), cells.size(), &need));
        std::vector<std::vector<uint64_t>> out(refs.size());
        for (size_t i = 0; i < refs.size(); ++i) out[i].assign(cells.begin() + offs[i], cells.begin() + offs[i + 1]);
        return out;
    }

    //! the Bloom-filter estimate of two documents' k-mer set similarity (cobs_gpu_jaccard_estimate, host arithmetic); the
    //! three estimates and n_inter are NaN when the union of the two filters is saturated, bit_jaccard still answers
    struct JaccardEstimate {
        double bit_jaccard = 0, jaccard = 0, containment_a_in_b = 0, containment_b_in_a = 0, n_inter = 0;
    };
    static JaccardEstimate jaccard_estimate(uint64_t sig, uint32_t num_hashes, uint64_t bits_a, uint64_t bits_b, uint64_t shared_ab) {
        double v[5];
        check(cobs_gpu_jaccard_estimate(sig, num_hashes, bits_a, bits_b, shared_ab, v));
        JaccardEstimate e;
        e.bit_jaccard = v[0], e.jaccard = v[1], e.containment_a_in_b = v[2], e.containment_b_in_a = v[3], e.n_inter = v[4];
        return e;
    }
    //! the one rule of a Jaccard threshold: min_jaccard <= 0 is no threshold and keeps every pair; a positive one keeps
    //! the pairs whose ESTIMATE reaches it, so a NaN estimate (a saturated filter) passes no threshold
    static bool reaches(double jaccard, double min_jaccard) { return !(min_jaccard > 0.0) || jaccard >= min_jaccard; }

    struct SimilarDocument {
        const char* doc_name;
        uint64_t doc;           // document index in the file
        uint32_t sub_index;
        uint64_t shared;
        double bit_jaccard, jaccard, containment_ref_in_doc, containment_doc_in_ref;
    };
    //! per reference the real documents of its sub-index other than itself, estimated Jaccard descending, then document
    //! index; documents whose estimate is NaN follow every finite one, ordered by bit_jaccard descending.  min_jaccard:
    //! see reaches(); num_results > 0 cuts each list.  All references go through ONE doc_shared_bits call.
    std::vector<std::vector<SimilarDocument>> similar_documents(const std::vector<uint32_t>& refs, size_t file_no = 0,
                                                                double min_jaccard = 0.0, size_t num_results = 0) {
        const cobs_gpu_index_info info = whole_file_info(file_no);
        for (uint32_t r : refs)
            if (r >= info.num_docs) throw Error(COBS_GPU_ERR_ARG, "similar_documents: a reference that is not a document of the file");
        const std::vector<std::vector<uint64_t>> shared = doc_shared_bits(refs, file_no);
        const std::vector<uint64_t> bits = doc_bits(file_no);
        const uint64_t per = info.kind == 0 ? info.counts_size : 8 * info.page_size;
        std::vector<std::vector<SimilarDocument>> out(refs.size());
        for (size_t i = 0; i < refs.size(); ++i) {
            const uint64_t ref = refs[i];
            const uint32_t pg = page_of(info, ref);
            const uint64_t d0 = info.kind == 0 ? 0 : pg * per, sig = cobs_gpu_signature_size(ix_, file_no, pg);
            std::vector<SimilarDocument>& rows = out[i];
            for (uint64_t s = 0; s < shared[i].size() && d0 + s < info.num_docs; ++s) {
                const uint64_t d = d0 + s;
                if (d == ref) continue;
                const JaccardEstimate e = jaccard_estimate(sig, (uint32_t)info.num_hashes, bits[ref], bits[d], shared[i][s]);
                if (!reaches(e.jaccard, min_jaccard)) continue;
                rows.push_back(SimilarDocument{cobs_gpu_doc_name(ix_, file_no, d), d, pg, shared[i][s], e.bit_jaccard, e.jaccard,
                                               e.containment_a_in_b, e.containment_b_in_a});
            }
            std::stable_sort(rows.begin(), rows.end(), [](const SimilarDocument& a, const SimilarDocument& b) {
                const bool na = std::isnan(a.jaccard), nb = std::isnan(b.jaccard);
                if (na != nb) return nb;
                return na ? a.bit_jaccard > b.bit_jaccard : a.jaccard > b.jaccard;
            });
            if (num_results > 0 && rows.size() > num_results) rows.resize(num_results);
        }
        return out;
    }
    std::vector<SimilarDocument> similar_documents(uint32_t ref, size_t file_no = 0, double min_jaccard = 0.0, size_t num_results = 0) {
        return similar_documents(std::vector<uint32_t>{ref}, file_no, min_jaccard, num_results)[0];
    }

    //! what a score is worth: expected_fp = the positions the document's filter fill alone is expected to hit, adjusted =
    //! the method-of-moments estimate of the positions that are truly shared (cobs_gpu_batch.h, "filter fill")
    struct Adjusted {
        double expected_fp = 0, adjusted = 0;
    };
    static Adjusted fpr_adjust(double score, double positions, uint64_t bits, uint64_t sig, uint64_t num_hashes, unsigned z = 0) {
        const double fill = (double)bits / (double)sig;
        const double q = std::pow(std::pow(fill, (double)num_hashes), (double)(z + 1));
        Adjusted a;
        a.expected_fp = positions * q;
        a.adjusted = q >= 1.0 ? 0.0 : std::max(0.0, (score - a.expected_fp) / (1.0 - q));
        return a;
    }

    //! ... for the results of a search of a query of query_length characters on this object (result[i].doc_name as the
    //! search returned it: the name's address identifies the document).  The positions are T - z; under
    //! COBS_GPU_INVALID_SKIP they are the query's valid positions, which this call does not have at hand: pass them per
    //! file (cobs_gpu_batch_scored_positions) or it throws.
    std::vector<Adjusted> adjust(const std::vector<SearchResult>& result, size_t query_length,
                                 const std::vector<uint64_t>* positions_per_file = nullptr) {
        const size_t nf = cobs_gpu_num_files(ix_);
        if (invalid_bases() == COBS_GPU_INVALID_SKIP && !(positions_per_file && positions_per_file->size() == nf))
            throw Error(COBS_GPU_ERR_UNSUPPORTED, "adjust: under invalid_bases = skip the valid positions per file are needed");
        const unsigned z = findere();
        std::vector<cobs_gpu_index_info> info(nf);
        std::vector<std::vector<uint64_t>> bits(nf);
        for (size_t f = 0; f < nf; ++f) info[f] = whole_file_info(f);
        if (doc_of_name_.empty())
            for (size_t f = 0; f < nf; ++f)
                for (uint64_t d = 0; d < info[f].num_docs; ++d) doc_of_name_[cobs_gpu_doc_name(ix_, f, d)] = {f, d};
        std::vector<Adjusted> out(result.size());
        for (size_t i = 0; i < result.size(); ++i) {
            const auto it = doc_of_name_.find(result[i].doc_name);
            if (it == doc_of_name_.end()) throw Error(COBS_GPU_ERR_ARG, "adjust: a result that is not from this object");
            const size_t f = it->second.first;
            const uint64_t d = it->second.second;
            if (bits[f].empty()) bits[f] = doc_bits(f);
            const double P = positions_per_file ? (double)(*positions_per_file)[f]
                                                : (double)query_length - (double)info[f].term_size + 1.0 - (double)z;
            out[i] = fpr_adjust(result[i].score, P, bits[f][d], cobs_gpu_signature_size(ix_, f, page_of(info[f], d)),
                                info[f].num_hashes, z);
        }
        return out;
    }

    //! findere z (0..7, beyond the reference): a position scores only when its z + 1 consecutive terms are all present
    //! (cobs_gpu_set_findere); 0 = the reference's count
    void set_findere(unsigned z) { check(cobs_gpu_set_findere(ix_, z)); }
    unsigned findere() const {
        uint32_t z = 0;
        check(cobs_gpu_get_findere(ix_, &z));
        return z;
    }

    //! what a character outside ACGT in a query does (beyond the reference, which dies): COBS_GPU_INVALID_ERROR (the
    //! default), _MISS (its k-mers are absent from every document) or _SKIP (... and leave the threshold's denominator);
    //! cobs_gpu_set_invalid_bases
    void set_invalid_bases(unsigned mode) { check(cobs_gpu_set_invalid_bases(ix_, mode)); }
    unsigned invalid_bases() const {
        uint32_t m = 0;
        check(cobs_gpu_get_invalid_bases(ix_, &m));
        return m;
    }

private:
    static void check(cobs_gpu_status st) {
        if (st != COBS_GPU_OK) throw Error(st, cobs_gpu_last_error());
    }
    static std::vector<std::string> paths_of(const std::vector<std::shared_ptr<IndexSearchFile>>& indices) {
        std::vector<std::string> out;
        for (const auto& i : indices) out.push_back(i->path());
        return out;
    }
    static uint32_t page_of(const cobs_gpu_index_info& info, uint64_t doc) {
        return info.kind == 0 ? 0u : (uint32_t)(doc / (8 * info.page_size));
    }
    cobs_gpu_index_info whole_file_info(size_t file_no) const {
        cobs_gpu_index_info info;
        check(cobs_gpu_info(ix_, file_no, &info));
        if (info.slot_begin != 0 || info.slot_count < info.num_docs)
            throw Error(COBS_GPU_ERR_UNSUPPORTED, "this handle holds a shard of the file's documents: use doc_bits");
        return info;
    }
    cobs_gpu_index* ix_ = nullptr;
    std::vector<cobs_gpu_hit> hits_;
    std::unordered_map<const char*, std::pair<size_t, uint64_t>> doc_of_name_;      // adjust(): built on first use
};

//! The same operator over SEVERAL GPUs of one node, one process: the index is sharded by
//! sub-index block over the devices, every search is one scan per GPU plus one exchange over RCCL
//! inside libcobs_gpu.so (cobs_gpu_multi_*: worker thread per device, communicator, collective
//! cobs_gpu_sharded_search_batch).  Results are identical to ClassicSearch on one GPU.
class ShardedClassicSearch : public BatchSearch {
public:
    ShardedClassicSearch(const std::vector<std::string>& paths, const std::vector<int>& devices,
                         uint64_t hbm_budget_bytes = 0) {
        std::vector<const char*> cp;
        for (const auto& p : paths) cp.push_back(p.c_str());
        cobs_gpu_options o{};
        o.struct_size = sizeof o;
        o.hbm_budget_bytes = hbm_budget_bytes;
        check(cobs_gpu_multi_open(cp.data(), cp.size(), devices.data(), devices.size(), &o, &m_));
        timer_.bind(handle());
    }
    ~ShardedClassicSearch() override { cobs_gpu_multi_close(m_); }
    ShardedClassicSearch(const ShardedClassicSearch&) = delete;
    ShardedClassicSearch& operator=(const ShardedClassicSearch&) = delete;

    void search(const std::string& query, std::vector<SearchResult>& result,
                double threshold = 0.0, size_t num_results = 0) final {
        std::vector<std::vector<SearchResult>> rs;
        search_batch({query}, rs, threshold, num_results);
        result = std::move(rs[0]);
    }

    void search_batch(const std::vector<std::string>& queries, std::vector<std::vector<SearchResult>>& results,
                      double threshold = 0.0, size_t num_results = 0) override {
        std::vector<const char*> qp;
        std::vector<size_t> ql;
        for (const auto& q : queries) { qp.push_back(q.data()); ql.push_back(q.size()); }
        std::vector<size_t> offs(queries.size() + 1, 0);
        cobs_gpu_index* ix = handle();
        const size_t total = (size_t)cobs_gpu_total_counts(ix);
        size_t cap;
        if (num_results > 0) cap = (num_results > total ? total : num_results) * queries.size();
        else if (threshold <= 0.0) cap = total * queries.size();
        else cap = std::max<size_t>(16 * queries.size(), (size_t)(hits_per_query_ * 1.25 * (double)queries.size())) + 1024;
        size_t bad = 0;
        cobs_gpu_status st;
        for (;;) {
            hits_.resize(cap + 1);
            st = cobs_gpu_multi_search_batch(m_, qp.data(), ql.data(), queries.size(), threshold, num_results,
                                             hits_.data(), hits_.size(), offs.data(), &bad);
            // the call is collective: if the buffer was too small every GPU repeats it
            if (st == COBS_GPU_ERR_CAPACITY && offs[queries.size()] > cap) {
                cap = offs[queries.size()];
                continue;
            }
            break;
        }
        check(st);
        if (threshold > 0.0 && num_results == 0 && !queries.empty())       // sizes the next thresholded calls: no second run
            hits_per_query_ = std::max((double)offs[queries.size()] / (double)queries.size(), 0.95 * hits_per_query_);
        results.resize(queries.size());
        for (size_t q = 0; q < queries.size(); ++q) {
            results[q].resize(offs[q + 1] - offs[q]);
            for (size_t i = offs[q]; i < offs[q + 1]; ++i)
                results[q][i - offs[q]] = SearchResult(cobs_gpu_doc_name(ix, hits_[i].file_no, hits_[i].doc), hits_[i].score);
        }
    }

    cobs_gpu_index* handle() const override { return cobs_gpu_multi_index(m_, 0); }
    //! every rank's shard handle (each holds the score slots of its own documents)
    std::vector<cobs_gpu_index*> shard_handles() const {
        std::vector<cobs_gpu_index*> v;
        for (size_t r = 0; r < cobs_gpu_multi_size(m_); ++r) v.push_back(cobs_gpu_multi_index(m_, r));
        return v;
    }
    //! ncclCommCount of the communicator the GPUs joined
    int comm_size() const { return (int)cobs_gpu_multi_size(m_); }
    //! findere z on every shard (see ClassicSearch::set_findere)
    void set_findere(unsigned z) { check(cobs_gpu_multi_set_findere(m_, z)); }
    unsigned findere() const {
        uint32_t z = 0;
        check(cobs_gpu_multi_get_findere(m_, &z));
        return z;
    }
    //! the invalid-bases policy on every shard (see ClassicSearch::set_invalid_bases)
    void set_invalid_bases(unsigned mode) { check(cobs_gpu_multi_set_invalid_bases(m_, mode)); }
    unsigned invalid_bases() const {
        uint32_t m = 0;
        check(cobs_gpu_multi_get_invalid_bases(m_, &m));
        return m;
    }

private:
    static void check(cobs_gpu_status st) {
        if (st != COBS_GPU_OK) throw Error(st, cobs_gpu_last_error());
    }
    cobs_gpu_multi* m_ = nullptr;
    std::vector<cobs_gpu_hit> hits_;
    double hits_per_query_ = 0.0;
};

}  // namespace cobs_gpu
