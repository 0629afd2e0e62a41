// cobs_amd/csrc/prevalence_kernels.hpp -- device side of cobs_gpu_prevalence (prevalence.cpp): for every position of a
// query, HOW MANY real documents hold it -- K2's gather reduced across the documents instead of across the terms.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// Arguments of the prevalence kernel for one chunk of one index file, as the engine holds it.
struct PrevalenceArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages: base, doc0, valid_bytes, tpage (row `sig` is the zero row K1 names for absent terms)
    TableRef t;                 // K1's row indices of the file (row_table.hpp); findere z: position p is set when terms
                                // p .. p + z are all present
    const uint64_t* seg_off;    // first cell of query q in this file: seg_off[q * seg_stride]
    uint32_t* out;              // cells of the pass: out[seg_off[q * seg_stride] + p] += documents of the slice that hold position p
    uint32_t seg_stride;        // files of the handle
    uint32_t page0;             // blockIdx.z + page0 = the page
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t num_docs;          // real documents of the file: slots at or beyond it never count
    uint32_t lx;                // lanes side by side along a row (16-byte chunks): a power of two, 1..64
    uint32_t ly;                // positions a wave takes side by side: 64 / lx
};

// lanes of a wave along a row of `valid_bytes` bytes: the next power of two of its 16-byte chunks, at most 64 (wider
// rows loop with stride 64); the other 64 / lx lanes take further positions
uint32_t prevalence_lx(uint32_t valid_bytes);

hipError_t launch_prevalence_zero(uint32_t* out, uint64_t n, hipStream_t stream);
// one launch per chunk (65535 pages at a time): grid (queries, position slabs, pages); max_positions = the longest
// query's n = T - z in this file
hipError_t launch_prevalence(PrevalenceArgs a, const std::vector<PageDev>& pages, uint32_t nq, uint32_t max_positions,
                             hipStream_t stream);

}  // namespace cobs_amd
