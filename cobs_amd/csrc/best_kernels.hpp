// cobs_amd/csrc/best_kernels.hpp -- device side of cobs_gpu_search_best (best.cpp): for every (group, slot) the best
// member of the group -- the query with the largest score / positions -- kept where the score rows of a pass lie
// (group_best_kernel), the partial states of a group whose queries were split over several work-groups folded in
// (group_best_merge_kernel), and the documents whose best member reaches the threshold appended to a pool
// (group_best_select_kernel).
//
// The state of a cell is (score, positions, query, ties) of the best member so far; the empty state is
// (0, 0, kBestNone, 0).  Two states merge by best_merge (best_kernels.hip), which is the order of cobs_gpu_batch.h:
// the larger fraction score / positions as 64-bit cross products (positions = 0 compares as the fraction 0 / 1), then the
// larger score, then the lower query; ties add up where the fractions are equal.  The merge is associative and the empty
// state is its identity, so a group may be cut by passes and pieces anywhere.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "group_kernels.hpp"

namespace cobs_amd {

constexpr uint32_t kBestNone = 0xFFFFFFFFu;     // `query` of the empty state; `piece` of a span that owns its cells

// The slots [begin, end) of a local score row that belong to one file, and P of the pass's queries in that file: the
// nominal T - z the host uploads, or K1's valid positions (`skip`).  begin and end are multiples of 8.
struct BestFile {
    uint32_t begin, end;
    const uint32_t* pos;
};

// A run of queries [q0, q1) of the pass that belong to one group.  piece == kBestNone: the only span of its group in the
// launch, its work-groups own their cells of the stored state (plain read-modify-write); otherwise the group's queries
// are split over several spans, and this one writes the partial state `piece`.
struct BestSpan {
    uint32_t group, q0, q1, piece;
};

// four arrays of [rows][nslots] words
struct BestState {
    uint32_t* score;
    uint32_t* positions;
    uint32_t* query;
    uint32_t* ties;
};

struct BestArgs {
    const void* rows;           // score rows of the pass: u8, u16 or u32 [nq][nslots]
    const BestSpan* spans;
    const BestFile* files;
    BestState state;            // [n_groups][nslots]
    BestState part;             // [pieces][nslots]
    uint64_t nslots;            // local score slots (a multiple of 8)
    uint32_t nspans, nfiles;
    uint32_t tiles;             // work-groups per span: ceil(nslots / (256 lanes x 16 bytes of scores))
    uint32_t score_bytes;
    uint32_t query0;            // index in the call of the pass's first query
};

// the partial states [piece0, piece1) belong to one group
struct BestFold {
    uint32_t group, piece0, piece1;
};

struct BestMergeArgs {
    const BestFold* folds;
    BestState state, part;
    uint64_t nslots;
    uint32_t nfolds;
};

struct BestRec {
    uint32_t group, file, doc, query, score, positions, ties;
};

struct BestSelArgs {
    BestState state;
    const GroupRange* ranges;
    BestRec* pool;
    unsigned long long* fill;   // records appended (may exceed cap: overflow, the caller grows the pool and selects again)
    uint64_t nslots;
    uint64_t cap;
    double threshold;           // a document is kept when score >= max(1, ceil(threshold * positions)); <= 0: every one
    uint32_t n_groups, nranges;
};

hipError_t launch_best_init(const BestState& s, uint64_t ncells, hipStream_t stream);
hipError_t launch_group_best(const BestArgs& a, hipStream_t stream);
hipError_t launch_group_best_merge(const BestMergeArgs& a, hipStream_t stream);
hipError_t launch_group_best_select(const BestSelArgs& a, hipStream_t stream);

}  // namespace cobs_amd
