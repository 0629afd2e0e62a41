// cobs_amd/csrc/querygen_kernels.hpp -- launchers of the generate-queries kernels
// (querygen_kernels.hip), called from querygen.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace cobs_amd {

// negative terms are looked up by their exact 2-bit packing: at most this many 64-bit words (k <= 256)
constexpr uint32_t kQgMaxWords = 8;

// The open-addressing table of the negative candidates' terms: one entry per term occurrence
// (candidate c, offset t) with id c * cand_terms + t; vals[slot] = id + 1, 0 = empty.  A term held
// by several candidates has one entry per occurrence on its probe chain.
struct QgTable {
    uint64_t* keys;             // capacity * words
    uint32_t* vals;             // capacity
    uint64_t mask;              // capacity - 1 (capacity a power of two >= 2 * entries)
    uint32_t words;             // ceil(k / 32)
    uint32_t cand_terms;        // size - k + 1
};

// One staged batch of documents (staging.hpp): the stretch tables of build_kernel plus where the
// positives of the batch's documents go.
struct QgBatchArgs {
    const uint8_t* text;        // term text, padded by kTextPad readable bytes
    const uint64_t* seg_off;    // nsegs + 1
    const uint32_t* seg_col;    // nsegs: visit index of the document | kBuildRawStretch, or kBuildGapStretch
    uint64_t total;             // bytes of text
    uint32_t nsegs, term_size;
    uint32_t col_base, ndocs;   // visit indices [col_base, col_base + ndocs) are in this batch
    uint64_t* blk_cnt;          // ceil(total / 256): terms per 256 positions, then their exclusive prefix
    unsigned long long* doc_base;   // ndocs: batch rank of the document's first term (set to ~0 first)
    // positives
    const uint64_t* vis_pos_off;    // visited documents + 1: positives of visit index j are [off[j], off[j + 1])
    const uint64_t* pos_local;      // document-local term index of every positive (ascending per document)
    uint8_t* pos_text;              // num_positive * term_size
    uint8_t* pos_hit;               // num_positive: 1 once the positive's term was written
    // the -N probe (probe != 0)
    uint32_t probe, canonical;
    QgTable table;
    uint8_t* found;                 // per candidate: 1 if one of its terms occurs in a document
    unsigned long long* probed;     // ACGT document terms looked up
};

struct QgInsertArgs {
    const uint8_t* cand_text;   // num_cand * size bytes, all ACGT
    uint64_t num_cand, size;
    uint32_t term_size, canonical;
    QgTable table;
};

hipError_t launch_qg_insert(const QgInsertArgs& a, hipStream_t stream);
// count -> scan -> document bases -> positives + probe, on one stream
hipError_t launch_qg_batch(const QgBatchArgs& a, hipStream_t stream);

}  // namespace cobs_amd
