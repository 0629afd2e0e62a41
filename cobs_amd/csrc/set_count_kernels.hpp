// cobs_amd/csrc/set_count_kernels.hpp -- device side of cobs_gpu_search_sets_quorum and cobs_gpu_set_prevalence
// (set_quorum.cpp): for every position of a query HOW MANY members of every labelled set hold it -- the prevalence kernel's
// gather reduced over the columns of one set at a time -- and the selection of the sets whose soft core (the positions held
// by at least need(set) members) reaches the threshold.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// The segment records of set_kernels.hpp inverted: one RUN per (page of the chunk, set with a member in that page), its
// records the 16-byte column chunks of the page that hold members, ascending, with the members' 128-bit mask.  A mask holds
// the slots of the set's members only -- no padding slot, no slot at or beyond the file's last document, no unlabelled
// document: the kernel masks nothing else.  The runs of a chunk are ordered by (page, set).
struct SetRun {
    uint32_t page;              // index into the chunk's pages
    uint32_t set;               // the set's number among the file's NON-EMPTY sets (ascending set number)
    uint32_t rec0, nrec;        // its records: rec_col / rec_mask [rec0, rec0 + nrec), nrec >= 1
};

// Arguments of the set count kernel for one chunk of one labelled index file, as the engine holds it.
struct SetCountArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages: base, tpage
    TableRef t;                 // K1's row indices of the file (row_table.hpp); findere z as in the prevalence kernel
    const SetRun* runs;
    const uint32_t* rec_col;    // the record's 16-byte column chunk of its page (< pitch / 16)
    const uint4* rec_mask;
    const uint64_t* cell_off;   // first cell of query q in this file: cell_off[q * cell_stride]
    uint32_t* cells;            // [set][n] from there, n = T - z: cells[set * n + p] += the members of the run that hold position p
                                // (zeroed by a kernel)
    uint32_t cell_stride;       // files of the handle
    uint32_t run0;              // blockIdx.z + run0 = the run
    uint32_t pitch;             // bytes between rows (a multiple of 16)
};

// one non-empty set of a labelled file: a work item of the select kernel per query
struct SetQuorumItem {
    uint32_t file_no, set;      // the file and the caller's set number
    uint32_t local;             // its number among the file's non-empty sets (the cells' set index)
    uint32_t term_size;
    uint32_t use_valid;         // P = K1's valid positions of (query, file) (invalid_bases = skip), else n
    uint32_t need;              // max(1, ceil(quorum * members)), computed on the host in double
};

// one selected (query, set): 16 bytes
struct SetQuorumRec {
    uint32_t query;
    uint32_t item;              // index into the items
    uint32_t core, any;
};

struct SetQuorumSelectArgs {
    const uint32_t* cells;
    const uint64_t* cell_off;   // [nq * nfiles]
    const SetQuorumItem* items;
    const uint32_t* q_len;
    const uint32_t* valid;      // K1's valid positions [file][nq] (read where use_valid)
    SetQuorumRec* pool;
    unsigned long long* fill;   // 64-bit fill of the pool (zeroed)
    uint64_t cap;
    double threshold;           // <= 0: every item is a hit
    uint32_t nq, nitems, nfiles, findere;
};

// one launch per chunk (65535 runs at a time): grid (queries, slabs of positions, runs); max_positions = the longest
// query's n = T - z in this file, max_recs = the records of the chunk's longest run
hipError_t launch_set_count(SetCountArgs a, size_t n_runs, uint32_t max_recs, uint32_t nq, uint32_t max_positions,
                            hipStream_t stream);
hipError_t launch_set_quorum_select(const SetQuorumSelectArgs& a, hipStream_t stream);

}  // namespace cobs_amd
