// cobs_amd/csrc/presence_kernels.hpp -- the per-position presence kernel of cobs_gpu_hit_positions (presence_kernels.hip):
// which terms of a query are present in ONE document, as a bit vector along the query.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "row_table.hpp"

namespace cobs_amd {

// One (query, document) pair as the host resolved it: the document's column in the resident chunk that holds it.
struct PresencePair {
    const uint8_t* col;     // address of (row 0 of the document's sub-index, the byte that holds the document's bit)
    uint64_t out;           // first output word of the pair (PresenceArgs::bits)
    uint32_t query;         // query of the pass (index into blk_off / q_len)
    uint32_t tpage;         // the sub-index in K1's row-index table
    uint32_t pitch;         // bytes between the rows of that sub-index
    uint32_t bit;           // document % 8
};

// Arguments of the presence kernel for one index file: the pairs whose document lives in that file.
struct PresenceArgs {
    TableRef t;                 // K1's row indices of the file (row_table.hpp); findere z: position p is set when terms
                                // p .. p + z are all present
    const PresencePair* pairs;
    uint64_t* bits;             // output words: pair i writes ceil((T - z) / 64) words from pairs[i].out
    uint32_t npairs;
};

// One work-group of four waves per pair (grid.x), a wave per 64 consecutive terms; max_words = the longest pair's output.
hipError_t launch_presence(const PresenceArgs& a, uint32_t max_words, hipStream_t stream);

}  // namespace cobs_amd
