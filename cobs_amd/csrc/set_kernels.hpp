// cobs_amd/csrc/set_kernels.hpp -- device side of cobs_gpu_search_sets (sets.cpp): the positions of a query that at least
// one / every member of a labelled SET of documents holds.  The prevalence kernel's gather, reduced over labelled subsets
// of the columns into two bit matrices, and the selection of the sets that reach their threshold.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// segment records a lane keeps in registers at a time (fixed indexing: no scratch); a column chunk with more distinct
// sets among its 128 slots walks its rows once per batch of this many, the repeats from cache
constexpr uint32_t kSetBatch = 4;

// Arguments of the set presence kernel for one chunk of one labelled index file, as the engine holds it.
struct SetPresenceArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages: base, doc0, valid_bytes, tpage
    TableRef t;                 // K1's row indices of the file (row_table.hpp); findere z as in the prevalence kernel
    // the segments of the chunk, CSR over (page, 16-byte column chunk): records [seg_first[page * cpp + c],
    // seg_first[page * cpp + c + 1]) are the distinct sets among the 128 slots of column chunk c of that page.  A mask holds
    // the slots of the set's members only -- no padding slot, no slot at or beyond the file's last document, no
    // unlabelled document: the kernel masks nothing else
    const uint32_t* seg_first;
    const uint4* seg_mask;
    const uint32_t* seg_set;    // the set's number among the file's NON-EMPTY sets (ascending set number)
    const uint64_t* bm_off;     // first word of query q's bitmaps of this file: bm_off[q * bm_stride]
    uint32_t* any;              // [set][W] words from there, W = ceil(n / 32): bit p % 32 of word p / 32 = position p is set
                                // in at least one member
    uint32_t* miss;             // same shape: ... is NOT set in some member (all = n - popcount).  Both zeroed by a kernel
    uint32_t bm_stride;         // files of the handle
    uint32_t page0;             // blockIdx.z + page0 = the page
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t cpp;               // column chunks per page in seg_first (pitch / 16)
    uint32_t num_docs;          // real documents of the file
    uint32_t lx;                // lanes side by side along a row (16-byte chunks): a power of two, 1..64
    uint32_t ly;                // blocks of 32 positions a wave takes side by side: 64 / lx
};

// one non-empty set of a labelled file: a work item of the select kernel per query
struct SetItem {
    uint32_t file_no, set;      // the file and the caller's set number
    uint32_t local;             // its number among the file's non-empty sets (the bitmaps' set index)
    uint32_t term_size;
    uint32_t use_valid;         // P = K1's valid positions of (query, file) (invalid_bases = skip), else n
};

// one selected (query, set): 16 bytes
struct SetRec {
    uint32_t query;
    uint32_t item;              // index into the items
    uint32_t any, all;
};

struct SetSelectArgs {
    const uint32_t* any;
    const uint32_t* miss;
    const uint64_t* bm_off;     // [nq * nfiles]
    const SetItem* items;
    const uint32_t* q_len;
    const uint32_t* valid;      // K1's valid positions [file][nq] (read where use_valid)
    SetRec* pool;
    unsigned long long* fill;   // 64-bit fill of the pool (zeroed)
    uint64_t cap;
    double threshold;           // <= 0: every item is a hit
    uint32_t nq, nitems, nfiles, findere;
    uint32_t rank_by;           // 0: the key is `any`, 1: `all`
};

// one launch per chunk (65535 pages at a time): grid (queries, slabs of position blocks, pages); max_positions = the
// longest query's n = T - z in this file
hipError_t launch_set_presence(SetPresenceArgs a, const std::vector<PageDev>& pages, uint32_t nq, uint32_t max_positions,
                               hipStream_t stream);
hipError_t launch_set_select(const SetSelectArgs& a, hipStream_t stream);

}  // namespace cobs_amd
