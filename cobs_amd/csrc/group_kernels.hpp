// cobs_amd/csrc/group_kernels.hpp -- device side of cobs_gpu_search_groups (groups.cpp): the score rows of a pass summed
// by group of queries where they lie (group_accumulate_kernel), and the documents of every group that reach the group's
// threshold appended to a pool (group_select_kernel).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace cobs_amd {

// The slots [begin, end) of a local score row that belong to one file, and the thresholds of the pass's queries in that
// file (PartWork::thr; nullptr: no read threshold, every document gets every query's vote).  begin and end are multiples
// of 8 (a file's slots are whole row bytes).
struct GroupFile {
    uint32_t begin, end;
    const uint32_t* thr;
};

// A run of queries [q0, q1) of the pass that belong to one group.  atomic == 0: this is the only span of its group in the
// launch, its work-groups own their cells (plain read-modify-write); != 0: the group's queries are split over several
// spans, which combine with one atomicAdd per cell and span.
struct GroupSpan {
    uint32_t group, q0, q1, atomic;
};

struct GroupAccArgs {
    const void* rows;           // score rows of the pass: u8, u16 or u32 [nq][nslots]
    const GroupSpan* spans;
    const GroupFile* files;
    uint32_t* acc_sum;          // [n_groups][nslots]
    uint32_t* acc_votes;        // [n_groups][nslots]
    uint64_t nslots;            // local score slots (a multiple of 8)
    uint32_t nspans, nfiles;
    uint32_t tiles;             // work-groups per span: ceil(nslots / (256 lanes x 16 bytes of scores))
    uint32_t score_bytes;
};

// The real documents of one file in a local score row: slot begin + i is document doc0 + i (padding slots excluded).
struct GroupRange {
    uint32_t begin, end, doc0, file;
};

struct GroupRec {
    uint32_t group, file, doc, sum, votes;
};

struct GroupSelArgs {
    const uint32_t* acc_sum;
    const uint32_t* acc_votes;
    const GroupRange* ranges;
    const uint64_t* gthr;       // [file][group]: a document is kept when its sum >= gthr
    GroupRec* pool;
    unsigned long long* fill;   // records appended (may exceed cap: overflow, the caller grows the pool and selects again)
    uint64_t nslots;
    uint64_t cap;
    uint32_t n_groups, nranges;
};

// slots one work-group of the accumulate kernel covers (256 lanes x 16 bytes)
inline uint32_t group_tile_slots(uint32_t score_bytes) { return 256u * 16u / score_bytes; }

hipError_t launch_group_zero(uint32_t* p, uint64_t nwords, hipStream_t stream);
hipError_t launch_group_accumulate(const GroupAccArgs& a, hipStream_t stream);
hipError_t launch_group_select(const GroupSelArgs& a, hipStream_t stream);

}  // namespace cobs_amd
