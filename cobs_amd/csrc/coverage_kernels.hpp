// cobs_amd/csrc/coverage_kernels.hpp -- device side of cobs_gpu_search_coverage (coverage.cpp): a scan shaped like the
// weighted scan whose per-document state RUNS ALONG the query -- a bit-sliced saturating countdown per document says
// whether the base under the walk is covered by a set position, and the covered bases are counted into bit-sliced
// counters (coverage_scan_kernel).  Also the ONE definition of "covered bases of a positions bitmap" (covered_bases).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// a set position covers span = k + z bases; the countdown has 8 planes
constexpr uint32_t kCoverageMaxSpan = 255;
// the count planes reach 2^20 - 1 covered bases: a query is shorter than this
constexpr uint64_t kCoverageMaxLen = 1ull << 20;
// shortest segment of positions a lane group takes when nothing is forced (a segment costs span - 1 positions of pre-roll)
constexpr uint32_t kCoverageMinSeg = 64;

// Covered bases of one bitmap of n positions (bit p of words[p / 64], as cobs_gpu_hit_positions packs it): the bases
// b in [0, n + span - 1) with a set position p in [b - span + 1, b].  Bits at or beyond n are ignored.  Host arithmetic;
// the ONE definition behind cobs_gpu_covered_bases.
inline uint64_t covered_bases(const uint64_t* words, size_t n, uint32_t span) {
    if (span == 0) return 0;
    uint64_t covered = 0, end = 0;          // end: one past the last base covered so far
    for (size_t w = 0; w * 64 < n; ++w) {
        uint64_t x = words[w];
        if (n - w * 64 < 64) x &= (1ull << (n - w * 64)) - 1;
        while (x) {
            const uint64_t p = w * 64 + (uint64_t)__builtin_ctzll(x);
            x &= x - 1;
            const uint64_t from = p > end ? p : end;
            covered += p + span - from;
            end = p + span;
        }
    }
    return covered;
}

// Arguments of the coverage scan for one chunk of one index file.
struct CoverageScanArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages
    TableRef t;                 // K1's row indices of the file (row_table.hpp)
    const uint32_t* thr;        // [nq] thresholds in covered bases, the same for every file (0: every real document)
    HitDev* pool;               // (query of the pass, file, document, covered bases)
    unsigned long long* fill;   // pool fill (may exceed cap: overflow)
    uint64_t cap;
    uint32_t nq;
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t cpp;               // 16-byte chunks per row (pitch / 16)
    uint32_t total_chunks;      // pages * cpp
    uint32_t tile_w;            // 16-byte chunks per tile: a power of two, 1..64
    uint32_t tile0;             // blockIdx.x / nq + tile0 = the tile
    uint32_t num_docs;          // real documents of the file
    uint32_t file_no;
    uint32_t span;              // term_size + findere: 1..255
    uint32_t seg;               // positions per segment (0: max(kCoverageMinSeg, the query's positions / lane groups))
};

// count planes of the scan for a longest query of `max_len` characters: 8, 12, 16 or 20 (0: too long)
int coverage_planes_for(uint64_t max_len);
// tile width for a chunk of `total_chunks` 16-byte column chunks
uint32_t coverage_tile_w(uint32_t total_chunks);

// one launch per chunk (in pieces of at most 2^31 - 1 work-groups): grid (tiles x queries), tile-major
hipError_t launch_coverage_scan(CoverageScanArgs a, int planes, hipStream_t stream);

}  // namespace cobs_amd
