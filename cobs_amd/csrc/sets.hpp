// cobs_amd/csrc/sets.hpp -- what the handle keeps for the document sets: the labels of every file and what is derived from
// them (sets.cpp: the segment records of cobs_gpu_search_sets, built when the labels are set; set_quorum.cpp: the inverse
// records of cobs_gpu_search_sets_quorum / cobs_gpu_set_prevalence, built on their first call), and the buffers of the two
// searches.  A FileSets that is replaced or cleared takes everything derived from its labels with it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"
#include "pooled_pass.hpp"
#include "set_count_kernels.hpp"
#include "set_kernels.hpp"

namespace cobs_amd {

struct ChunkSegs {                          // the segment records of one resident chunk (set_kernels.hpp)
    DevBuf<uint32_t> first;
    DevBuf<uint4> mask;
    DevBuf<uint32_t> set;
    bool built = false;
};

struct ChunkRuns {                          // the inverse records of one resident chunk (set_count_kernels.hpp)
    DevBuf<SetRun> runs;
    DevBuf<uint32_t> col;
    DevBuf<uint4> mask;
    size_t n_runs = 0;
    uint32_t max_recs = 0;                  // records of the longest run
};

struct FileSets {
    std::vector<uint32_t> labels;           // [documents of the file]; empty: the file has no labels
    uint32_t n_sets = 0;
    std::vector<uint32_t> members;          // [n_sets]
    std::vector<uint32_t> sets;             // the non-empty sets, ascending: the bitmaps' set index -> set number
    std::vector<ChunkSegs> chunks;          // [Part::chunks]
    std::vector<ChunkRuns> runs;            // [Part::chunks] once a quorum call has asked for them, else empty
};

struct SetQuorumWork {                      // set_quorum.cpp
    DevBuf<uint32_t> cells;                 // the counts of a pass
    DevBuf<uint64_t> cell_off;
    DevBuf<SetQuorumItem> items;
    DevBuf<SetQuorumRec> pool;
    DevBuf<unsigned long long> fill;
    PinnedBuf<uint64_t> h_cell_off;
    PassLanding land;
    PhaseEvents<4> ev;                      // before K1 | count | select | after it
    double ms[4] = {0, 0, 0, 0};            // hash | count | select | host ordering
    uint64_t passes = 0;
};

struct SetsWork {
    std::vector<FileSets> files;            // [parts]
    DevBuf<uint32_t> bits;                  // any | miss of a pass
    DevBuf<uint64_t> bm_off;
    DevBuf<SetItem> items;
    DevBuf<SetRec> pool;
    DevBuf<unsigned long long> fill;
    PinnedBuf<uint64_t> h_bm_off;
    PassLanding land;
    PhaseEvents<4> ev;                      // before K1 | presence | select | after it
    double ms[4] = {0, 0, 0, 0};            // hash | presence | select | host ordering
    uint64_t passes = 0;
    SetQuorumWork quorum;
};

}  // namespace cobs_amd
