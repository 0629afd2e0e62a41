// cobs_amd/csrc/similarity_kernels.hpp -- device side of cobs_gpu_doc_shared_bits (similarity.cpp): for a panel of up to
// kSimRefs reference documents of one sub-index, in how many rows every document of that sub-index has its bit set
// TOGETHER with each reference -- the vertical popcount of fill_kernels.hip conditioned on the references' own bits.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"

namespace cobs_amd {

// References of one panel = counter sets a lane keeps.  A lane owns ONE 32-bit column word (32 documents) and keeps
// kSimPlanes bit planes of it per reference: kSimRefs x kSimPlanes = 96 plane registers ("shared_count_kernel").
constexpr int kSimRefs = 8;
constexpr int kSimPlanes = 12;
constexpr uint32_t kSimBlockRows = 8;                                               // rows of one carry-save block
constexpr uint32_t kSimFlushBlocks = ((1u << kSimPlanes) - 1u) / kSimBlockRows;     // 511 blocks = 4088 rows per lane and slab
static_assert(kSimRefs <= 8, "a row's reference word is one byte");

// where a reference's bit lies in a row of its sub-index
struct SimRef { uint32_t byte, bit; };

struct RefRowsArgs {
    const uint8_t* data;        // the resident chunk of the sub-index
    uint64_t base;              // byte offset of its row 0
    uint64_t sig;               // rows (row `sig` is the zero row and is never read)
    uint8_t* refw;              // [sig] out: bit j of refw[r] = reference j has its bit set in row r
    SimRef ref[kSimRefs];
    uint32_t nrefs;
    uint32_t pitch;
};

struct SimArgs {
    const uint8_t* data;
    const uint8_t* refw;        // [sig] from ref_rows_kernel
    unsigned long long* out;    // [nrefs][nslots] cells, zeroed; every lane adds its own sums (atomicAdd)
    uint64_t base, sig;
    uint64_t slab_rows;         // rows of one row slab (at most kSimFlushBlocks blocks per lane)
    uint32_t nslots;            // valid_bytes x 8: cells per reference
    uint32_t valid_bytes;       // row bytes that map to cells (bytes beyond them map to none)
    uint32_t nrefs;
    uint32_t pitch;             // bytes between rows (a multiple of 16)
    uint32_t tiles;             // column tiles per row; blockIdx.x = slab * tiles + tile
    uint32_t lx;                // lanes (4-byte words) of a tile along a row; 64 = a wave lies in one row
    uint32_t ly;                // rows a work-group of 256 lanes takes side by side
};

struct SimGeom {
    uint64_t slab_rows, slabs;
    uint32_t tiles, lx, ly;
};
// tests shrink the geometry so that small fixtures reach full-length slabs and slab boundaries (0 = automatic)
struct SimTune {
    uint32_t groups = 0;        // COBS_GPU_SIM_GROUPS: work-groups a launch aims for (1024)
    uint32_t max_side = 0;      // COBS_GPU_SIM_SIDE: upper bound of ly
};
SimGeom sim_geometry(uint64_t sig, uint32_t valid_bytes, const SimTune& tune);

hipError_t launch_ref_rows(const RefRowsArgs& a, hipStream_t stream);
hipError_t launch_sim_zero(unsigned long long* out, uint64_t n, hipStream_t stream);
// one sweep over the rows [0, sig) of the sub-index; a.slab_rows, tiles, lx, ly are filled in here from sim_geometry
hipError_t launch_shared_count(SimArgs a, hipStream_t stream, const SimTune& tune);

}  // namespace cobs_amd
