// cobs_amd/csrc/pooled_call.hpp -- the host skeleton of a pooled search call, the parts that are plain arithmetic: the seven
// families whose kernels append records to a pool (weighted.cpp, coverage.cpp, window.cpp, groups.cpp, best.cpp, sets.cpp,
// set_quorum.cpp) count the real documents, guess the pool, turn a threshold into the smallest key of a hit, cut the
// call's queries into device passes and hand the ordered lists out with what stands here.  No HIP header: a host program
// compiles this file alone (tests/host/pooled_call.cpp).  The device half -- the pool and its one retry, the pass of the
// pooled scans -- is pooled_pass.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cobs_gpu.h"

namespace cobs_amd {

cobs_gpu_status fail(cobs_gpu_status st, const std::string& msg);     // engine.cpp

// the real documents among the score slots a file computes on this device (the slots behind them are padding)
template <typename PartT>
uint64_t real_documents_of(const PartT& p) {
    const uint64_t docs = p.meta.doc_names.size();
    return docs > p.slot_begin ? std::min<uint64_t>(docs - p.slot_begin, p.slot_count) : 0;
}

// ... of all files
template <typename IndexT>
uint64_t real_documents(const IndexT& ix) {
    uint64_t total = 0;
    for (const auto& p : ix.parts) total += real_documents_of(p);
    return total;
}

// ... as the select kernels walk them: per file with real documents Range{first local slot, the slot behind the last,
// first document, file}
template <typename Range, typename IndexT>
std::vector<Range> real_ranges(const IndexT& ix) {
    std::vector<Range> ranges;
    for (size_t f = 0; f < ix.parts.size(); ++f) {
        const auto& p = ix.parts[f];
        if (const uint64_t real = real_documents_of(p))
            ranges.push_back(Range{(uint32_t)p.local_offset, (uint32_t)(p.local_offset + real), (uint32_t)p.slot_begin, (uint32_t)f});
    }
    return ranges;
}

// The first guess of a pool for n_lists lists (queries of a pass, groups of a call) over real_total documents: every
// record when every document comes back, else a share the retry corrects.  hit_cap (tuning key, 0: none) lowers it, so
// that tests reach the overflow path; never below one record.
inline uint64_t first_pool_cap(uint64_t hit_cap, double threshold, uint64_t real_total, uint64_t n_lists) {
    const uint64_t all = real_total * n_lists;
    uint64_t cap = threshold > 0.0 ? std::min<uint64_t>(all, std::max<uint64_t>(1u << 20, n_lists * 1024ull)) : all;
    if (hit_cap) cap = std::min<uint64_t>(cap, hit_cap);
    return std::max<uint64_t>(cap, 1);
}

// The threshold rule of the pooled families, on the host: a hit needs key >= max(1, ceil(threshold * P)), the product
// formed in double; a threshold that is not > 0 (0, negative, NaN) gives 0 -- every document.  Key = uint32_t saturates at
// 2^32 - 1; Key = uint64_t (the group sums) at 2^64 - 1, from the largest double below 2^64 on.
//
// threshold_for (pass.cpp) is the plain search's rule and differs in exactly one way: it has no "at least 1".  It returns
// ceil(threshold * T) as the reference computes it, so a product that is 0, negative or NaN (T = 0; inf * 0) gives 0 and
// the query matches EVERY document, where min_key gives 1 and a document needs one position.  For a threshold that is
// not > 0 both give 0; for every threshold > 0, min_key<uint32_t> == max(1, threshold_for).
template <typename Key>
Key min_key(double threshold, uint64_t P) {
    static_assert(sizeof(Key) == 4 || sizeof(Key) == 8, "a 32-bit or a 64-bit key");
    if (!(threshold > 0.0)) return 0;
    const double v = std::ceil(threshold * (double)P);
    constexpr double from = sizeof(Key) == 8 ? 18446744073709549568.0 : 4294967295.0;
    return !(v >= 1.0) ? (Key)1 : v >= from ? (Key)~(Key)0 : (Key)v;
}

// The passes of a call: run(first, last) for consecutive ranges of the queries [0, nq) whose bytes_of(q) add up to at most
// `limit`; a query that alone exceeds the limit gets a pass of its own (the families that cannot run it refuse it before
// they come here).  The last range is run even when it is empty: nq = 0 gives run(0, 0) -- no family comes here with it.
// The first status that is not OK ends the call.
template <typename BytesOf, typename Run>
cobs_gpu_status cut_passes(size_t nq, uint64_t limit, BytesOf&& bytes_of, Run&& run) {
    size_t first = 0;
    uint64_t bytes = 0;
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t qb = bytes_of(q);
        if (q > first && bytes + qb > limit) {
            if (cobs_gpu_status s = run(first, q); s != COBS_GPU_OK) return s;
            first = q;
            bytes = 0;
        }
        bytes += qb;
    }
    return run(first, nq);
}

// The hand-over of a call's records as n_lists lists (list_of(rec): its query or group): ordered by list and inside a
// list by before(a, b), every list cut to num_results (0: whole), hit_offsets[0 .. n_lists] written, and -- when the
// `cap` records of `hits` hold them -- hits[i] = emit(rec).  They do not: ERR_CAPACITY, hit_offsets[n_lists] is the size
// needed and nothing is written to hits.  offsets_end names that entry in the message ("nq", "n_groups").
template <typename Rec, typename ListOf, typename Before, typename Hit, typename Emit>
cobs_gpu_status hand_out_lists(std::vector<Rec>& recs, size_t n_lists, ListOf&& list_of, Before&& before, size_t num_results,
                               Hit* hits, size_t cap, size_t* hit_offsets, const char* offsets_end, Emit&& emit) {
    std::sort(recs.begin(), recs.end(), [&](const Rec& a, const Rec& b) {
        if (list_of(a) != list_of(b)) return list_of(a) < list_of(b);
        return before(a, b);
    });
    std::vector<size_t> begin(n_lists + 1, 0);
    for (const Rec& r : recs) begin[list_of(r) + 1]++;
    for (size_t l = 0; l < n_lists; ++l) begin[l + 1] += begin[l];
    size_t used = 0;
    hit_offsets[0] = 0;
    for (size_t l = 0; l < n_lists; ++l) {
        const size_t have = begin[l + 1] - begin[l];
        used += num_results ? std::min(have, num_results) : have;
        hit_offsets[l + 1] = used;
    }
    if (used > cap)
        return fail(COBS_GPU_ERR_CAPACITY, std::string("result buffer too small; hit_offsets[") + offsets_end + "] holds the needed size");
    for (size_t l = 0; l < n_lists; ++l) {
        const Rec* r = recs.data() + begin[l];
        Hit* out = hits + hit_offsets[l];
        for (size_t i = 0, n = hit_offsets[l + 1] - hit_offsets[l]; i < n; ++i) out[i] = emit(r[i]);
    }
    return COBS_GPU_OK;
}

}  // namespace cobs_amd
