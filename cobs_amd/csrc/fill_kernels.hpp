// cobs_amd/csrc/fill_kernels.hpp -- device side of cobs_gpu_doc_bits (fill.cpp): how many rows of a sub-index have the
// bit of each document set -- a vertical popcount of the bit-sliced matrix, one launch per chunk as the engine holds it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "device_types.hpp"

namespace cobs_amd {

// Bit planes of a lane's vertical counters: a lane counts at most 2^kFillPlanes - 1 rows (one row slab) and then adds
// its counters to the output.  12 planes: a flush writes 128 cells of 8 bytes for 16 x 4088 bytes read, 1.6 % of the input.
constexpr int kFillPlanes = 12;
constexpr uint32_t kFillBlockRows = 8;                                                  // rows of one carry-save block
constexpr uint32_t kFillFlushBlocks = ((1u << kFillPlanes) - 1u) / kFillBlockRows;      // 511 blocks = 4088 rows

struct FillArgs {
    const uint8_t* data;        // the chunk's buffer (resident blob or stream buffer)
    const PageDev* pages;       // its pages: base, sig (rows IN the buffer; row `sig` is the zero row and is never read), slot0, valid_bytes
    unsigned long long* out;    // [local slots of the file] sums; every lane adds its own (atomicAdd)
    uint64_t slab_rows;         // rows of one row slab (at most kFillFlushBlocks blocks per lane)
    uint64_t slab0;             // first slab of this launch
    uint32_t page0;             // blockIdx.y + page0 = the page
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t tiles;             // column tiles per row; blockIdx.x = slab * tiles + tile
    uint32_t lx;                // lanes (16-byte chunks) of a tile along a row
    uint32_t ly;                // rows a work-group of 256 lanes takes side by side: 256 / lx
};

// the launch geometry of a chunk (host arithmetic; fill.cpp and the probe share it)
struct FillGeom {
    uint64_t slab_rows;
    uint64_t max_slabs;
    uint32_t tiles, lx, ly;
};
// tests shrink the geometry so that small fixtures reach full-length slabs and slab boundaries (0 = automatic)
struct FillTune {
    uint32_t groups = 0;        // work-groups a launch aims for (1024)
    uint32_t max_side = 0;      // upper bound of ly
};
FillGeom fill_geometry(const std::vector<PageDev>& pages, const FillTune& tune);

hipError_t launch_fill_zero(unsigned long long* out, uint64_t n, hipStream_t stream);
// counts the rows [0, sig) of every page of the chunk; *bytes_read (optional) += rows x valid row bytes
hipError_t launch_fill_count(const uint8_t* data, const PageDev* d_pages, const std::vector<PageDev>& pages, uint32_t pitch,
                             unsigned long long* out, hipStream_t stream, uint64_t* bytes_read, const FillTune& tune);
// the arithmetic-free yardstick (scripts/probes/fill_probe.py): the same loads over the same buffers, one XOR per load,
// one store per lane into sink[global lane]; sink holds fill_probe_lanes() words
uint64_t fill_probe_lanes(const std::vector<PageDev>& pages, const FillTune& tune);
hipError_t launch_fill_probe(const uint8_t* data, const PageDev* d_pages, const std::vector<PageDev>& pages, uint32_t pitch,
                             uint32_t* sink, hipStream_t stream, const FillTune& tune);

}  // namespace cobs_amd
