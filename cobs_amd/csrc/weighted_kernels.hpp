// cobs_amd/csrc/weighted_kernels.hpp -- device side of cobs_gpu_search_weighted (weighted.cpp): the per-position counts of
// the prevalence kernel become 4-bit IDF weights (weight_kernel), and a scan shaped like K2 adds every position's weight,
// where K2 adds 1, into bit-sliced per-document counters (weighted_scan_kernel).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// the largest weight: 1 + min(14, floor(log2(D / c)))
constexpr uint32_t kMaxWeight = 15;
// 15 * n stays below 2^20 (the counter planes the scan is instantiated for): n <= 69 905
constexpr uint64_t kWeightedMaxPositions = ((1ull << 20) - 1) / kMaxWeight;

// The IDF weight of a position that `count` of `num_docs` documents hold: 0 for count = 0, else
// 1 + max{ j in 0..14 : count * 2^j <= num_docs } -- integer arithmetic; the ONE definition, called by
// cobs_gpu_idf_weight on the host and by weight_kernel on the device.
__host__ __device__ inline uint32_t idf_weight(uint64_t num_docs, uint64_t count) {
    if (count == 0) return 0;
    const uint64_t r = num_docs / count;    // count * 2^j <= num_docs  <=>  2^j <= floor(num_docs / count)
    uint32_t j = 0;
    while (j < 14 && (r >> (j + 1)) != 0) ++j;
    return 1 + j;
}

// Arguments of the weight kernel for one index file: block q turns the cells of segment (q, file) into weights.
struct WeightArgs {
    const uint32_t* cells;      // the prevalence kernel's counts of the pass
    uint8_t* weights;           // same layout: weights[seg + p] = idf_weight(num_docs, cells[seg + p])
    const uint64_t* seg_off;    // first cell of query q in this file: seg_off[q * seg_stride] (a multiple of 8)
    const uint32_t* q_len;      // characters per query
    uint64_t* total;            // W(q, f) at total[q * seg_stride]
    uint32_t* thr;              // [nq] of this file: threshold > 0: max(1, ceil(threshold * W)) in double; else 0
    double threshold;
    uint32_t seg_stride;        // files of the handle
    uint32_t term_size;
    uint32_t findere;
    uint32_t num_docs;          // D_f
};

// Arguments of the weighted scan for one chunk of one index file.
struct WeightedScanArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages
    TableRef t;                 // K1's row indices of the file (row_table.hpp)
    const uint64_t* seg_off;    // first weight of query q in this file: seg_off[q * seg_stride] (a multiple of 8; the
                                // segment is padded to a multiple of 8 with weights of 0)
    const uint8_t* weights;
    const uint32_t* thr;        // [nq] thresholds of this file (0: every real document)
    HitDev* pool;               // (query of the pass, file, document, weighted score)
    unsigned long long* fill;   // pool fill (may exceed cap: overflow)
    uint64_t cap;
    uint32_t seg_stride;
    uint32_t nq;
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t cpp;               // 16-byte chunks per row (pitch / 16)
    uint32_t total_chunks;      // pages * cpp
    uint32_t tile_w;            // 16-byte chunks per tile: a power of two, 1..64
    uint32_t tile0;             // blockIdx.x / nq + tile0 = the tile
    uint32_t num_docs;          // real documents of the file
    uint32_t file_no;
};

// counter planes of the scan for a longest query of `max_positions` positions: 8, 12, 14, 16 or 20 (0: too long)
int weighted_planes_for(uint64_t max_positions);
// tile width for a chunk of `total_chunks` 16-byte column chunks
uint32_t weighted_tile_w(uint32_t total_chunks);

// one launch per file: grid (queries)
hipError_t launch_weights(const WeightArgs& a, uint32_t nq, hipStream_t stream);
// one launch per chunk (in pieces of at most 2^31 - 1 work-groups): grid (tiles x queries), tile-major
hipError_t launch_weighted_scan(WeightedScanArgs a, int planes, hipStream_t stream);

}  // namespace cobs_amd
