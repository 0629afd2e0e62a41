// cobs_amd/csrc/window_kernels.hpp -- device side of cobs_gpu_search_window (window.cpp): a scan shaped like the coverage
// scan whose per-document state is the count of set positions in the window of w positions that ends under the walk,
// kept bit-sliced as its distance to the best count so far (window_scan_kernel).  Also the ONE definition of "best window
// of a positions bitmap" (best_window).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "device_types.hpp"
#include "row_table.hpp"

namespace cobs_amd {

// the record planes hold counts below 2^12
constexpr uint32_t kWindowMax = 4095;
// the walk's positions, segment ends and block numbers are 32-bit: s + seg and 8 b0 + w stay below 2^31 for queries
// below this many characters.  The bound is by arithmetic only: the tests walk queries of up to 8 193 positions and
// reach the refusal; nothing between has been run
constexpr uint64_t kWindowMaxLen = 1ull << 30;
// shortest segment of positions a lane group takes when nothing is forced ...
constexpr uint32_t kWindowMinSeg = 64;
// ... and its length in windows.  A segment costs w - 1 positions of pre-roll, both row streams included, so segments of
// m w positions walk 1 + 1 / m times the query.  m = 1: the pre-roll at most doubles the walk, and a query of a few
// windows still spreads over the lane groups.  Lane groups without a segment are not free: their waves hold their
// registers until the merge.  A query with w = n is one segment whatever m is (DESIGN.md sections 4 and 7).
constexpr uint32_t kWindowSegWindows = 1;

// Best window of one bitmap of n positions (bit p of words[p / 64], as cobs_gpu_hit_positions packs it): with
// w = min(window, n), the largest number of set positions in [s, s + w) over s in [0, n - w], and the smallest s that
// reaches it.  Bits at or beyond n are ignored.  Host arithmetic; the ONE definition behind cobs_gpu_best_window.
inline uint32_t best_window(const uint64_t* words, size_t n, uint32_t window, size_t* start) {
    if (start) *start = 0;
    if (!words || n == 0 || window == 0) return 0;
    const size_t w = window < n ? (size_t)window : n;
    auto bit = [&](size_t p) -> uint32_t { return (uint32_t)(words[p >> 6] >> (p & 63)) & 1u; };
    uint32_t c = 0;
    for (size_t p = 0; p < w; ++p) c += bit(p);
    uint32_t best = c;
    size_t at = 0;
    for (size_t p = w; p < n; ++p) {            // the window [p - w + 1, p]
        c += bit(p);
        c -= bit(p - w);
        if (c > best) {
            best = c;
            at = p - w + 1;
        }
    }
    if (start) *start = at;
    return best;
}

// Arguments of the window scan for one chunk of one index file.
struct WindowScanArgs {
    const uint8_t* data;        // the chunk's buffer
    const PageDev* pages;       // its pages
    TableRef t;                 // K1's row indices of the file (row_table.hpp)
    const uint32_t* thr;        // [nq] thresholds in set positions of THIS file (0: every real document)
    const uint32_t* win;        // [nq] w = min(window, the query's positions in this file): 1..kWindowMax
    HitDev* pool;               // (query of the pass, file, document, best)
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
    uint32_t window;            // W of the call: picks the plane count (every win[q] <= window)
    uint32_t seg;               // positions per segment (0: max(kWindowMinSeg, kWindowSegWindows w, positions / lane groups))
};

// planes of the scan for a call's window: 6, 8, 10 or 12 (0: beyond kWindowMax)
int window_planes_for(uint32_t window);

// one launch per chunk (in pieces of at most 2^31 - 1 work-groups): grid (tiles x queries), tile-major
hipError_t launch_window_scan(WindowScanArgs a, hipStream_t stream);

}  // namespace cobs_amd
