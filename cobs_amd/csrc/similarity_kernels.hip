// cobs_amd/csrc/similarity_kernels.hip -- shared filter bits of documents on the device (cobs_gpu_doc_shared_bits,
// similarity.cpp).
//
// shared(a, d) of a sub-index = the rows in which documents a and d both have their bit set.  For a panel of up to M
// reference documents one sweep over the sub-index counts it for every document d: the vertical popcount of
// fill_kernels.hip, once per reference, each conditioned on the reference's own bit of the row (DESIGN 3,
// "shared_count_kernel").  gfx950, wave64.
//
// ref_rows_kernel writes one byte per row: bit j = reference j of the panel has its bit set in that row.
//
// shared_count_kernel<M>.  A lane owns one 32-bit column word (32 documents) and keeps, per reference, kSimPlanes bit
// planes of it.  The lx lanes of a column tile sit side by side along a row, so a wave's load is a contiguous piece of
// one row; the rest of the 256 lanes take further rows (ly rows side by side).  The grid is column tiles x row slabs.
// A lane walks its slab in blocks of 8 rows, all 8 loads in flight at once, and reads the 8 rows' reference bytes
// beside them.  Where a wave lies in one row (lx = 64: every sub-index of 2017 documents or more) the reference bytes
// are wave-uniform: they are moved to scalar registers, a reference without a set bit in the block costs a scalar branch
// and no vector work, and the masks of the others are made by the scalar unit.  For every other reference the block's 8
// words, each ANDed with (the reference's bit of its row, spread over the word), go into the reference's planes through
// the Harley-Seal carry-save tree of the fill kernel: 8 + 14 + 2 x 9 = 40 ops per 8 words and reference.  A slab ends
// before the planes can overflow (4088 rows per lane); the planes are expanded and added to the 64-bit cells.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "similarity_kernels.hpp"
#include "wave_ops.hpp"      // csa

namespace cobs_amd {

namespace {

constexpr int NP = kSimPlanes;

// eight row words into the planes of one column word (fill_kernels.hip: absorb8)
__device__ __forceinline__ void absorb8(uint32_t (&pl)[NP], uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4,
                                        uint32_t x5, uint32_t x6, uint32_t x7) {
    uint32_t t2a, t2b, f4a, f4b, carry;
    csa(t2a, pl[0], pl[0], x0, x1);
    csa(t2b, pl[0], pl[0], x2, x3);
    csa(f4a, pl[1], pl[1], t2a, t2b);
    csa(t2a, pl[0], pl[0], x4, x5);
    csa(t2b, pl[0], pl[0], x6, x7);
    csa(f4b, pl[1], pl[1], t2a, t2b);
    csa(carry, pl[2], pl[2], f4a, f4b);
#pragma unroll
    for (int k = 3; k < NP; ++k) {
        const uint32_t t = pl[k] & carry;
        pl[k] ^= carry;
        carry = t;
    }
}

// bit j of w spread over a word: 0 or ~0 (one bit-field extract, on the scalar unit where w is wave-uniform)
__device__ __forceinline__ uint32_t spread(uint32_t w, int j) { return 0u - ((w >> j) & 1u); }

// planes of one column word -> 32 per-document sums, added to the cells (bytes beyond the row's valid bytes map to no cell)
__device__ __forceinline__ void flush_word(const uint32_t (&pl)[NP], unsigned long long* out, uint32_t byte0, uint32_t valid_bytes) {
    for (uint32_t b = 0; b < 32u; ++b) {
        if (byte0 + (b >> 3) >= valid_bytes) break;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) v |= ((pl[k] >> b) & 1u) << k;
        if (v) atomicAdd(out + b, (unsigned long long)v);
    }
}

// UNI: lx == 64, every wave lies in one row (its reference bytes are wave-uniform)
template <int M, bool UNI>
__global__ __launch_bounds__(256) void shared_count_kernel(SimArgs a) {
    const uint32_t tile = blockIdx.x % a.tiles;
    const uint64_t slab = blockIdx.x / a.tiles;
    const uint64_t r_begin = slab * a.slab_rows;
    const uint32_t cx = threadIdx.x % a.lx, ry = threadIdx.x / a.lx;
    const uint32_t word = tile * a.lx + cx;
    if (r_begin >= a.sig || ry >= a.ly || (uint64_t)word * 4u >= a.valid_bytes) return;
    const uint64_t r_end = min(a.sig, r_begin + a.slab_rows);
    const uint8_t* col = a.data + a.base + (uint64_t)word * 4u;
    const uint64_t step = (uint64_t)kSimBlockRows * a.ly;
    uint32_t pl[M][NP];
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[j][k] = 0u;
    for (uint64_t r = r_begin + ry; r < r_end; r += step) {
        uint32_t X[kSimBlockRows], W[kSimBlockRows];
#pragma unroll
        for (uint32_t i = 0; i < kSimBlockRows; ++i) {
            const uint64_t row = r + (uint64_t)i * a.ly;
            X[i] = 0u;
            W[i] = 0u;
            if (row < r_end) {
                X[i] = *reinterpret_cast<const uint32_t*>(col + row * a.pitch);
                W[i] = a.refw[row];
            }
        }
        if (UNI) {
#pragma unroll
            for (uint32_t i = 0; i < kSimBlockRows; ++i) W[i] = __builtin_amdgcn_readfirstlane(W[i]);
        }
        const uint32_t any = W[0] | W[1] | W[2] | W[3] | W[4] | W[5] | W[6] | W[7];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (!((any >> j) & 1u)) continue;
            absorb8(pl[j], X[0] & spread(W[0], j), X[1] & spread(W[1], j), X[2] & spread(W[2], j), X[3] & spread(W[3], j),
                    X[4] & spread(W[4], j), X[5] & spread(W[5], j), X[6] & spread(W[6], j), X[7] & spread(W[7], j));
        }
    }
    unsigned long long* out = a.out + (uint64_t)word * 32u;
#pragma unroll
    for (int j = 0; j < M; ++j)
        if ((uint32_t)j < a.nrefs) flush_word(pl[j], out + (uint64_t)j * a.nslots, word * 4u, a.valid_bytes);
}

__global__ __launch_bounds__(256) void ref_rows_kernel(RefRowsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.sig) return;
    const uint8_t* row = a.data + a.base + r * a.pitch;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < kSimRefs; ++j)
        if ((uint32_t)j < a.nrefs) w |= ((row[a.ref[j].byte] >> a.ref[j].bit) & 1u) << j;
    a.refw[r] = (uint8_t)w;
}

__global__ void sim_zero_kernel(unsigned long long* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0ull;
}

}  // namespace

// Column tiles of 64 lanes (a wave = 256 bytes of one row) where a row has 64 words or more -- the last tile's spare
// lanes idle, the price of wave-uniform reference bytes --, else one tile of the row's words with the rest of the 256
// lanes on further rows.  Row slabs as the fill kernel cuts them: the longest a lane's planes can count where that still
// gives the device 1024 work-groups, else the rows spread over 1024 work-groups.
SimGeom sim_geometry(uint64_t sig, uint32_t valid_bytes, const SimTune& tune) {
    SimGeom g{};
    const uint32_t words = (valid_bytes + 3u) / 4u;
    if (words == 0) return g;
    g.tiles = (words + 63u) / 64u;
    g.lx = std::min(words, 64u);
    g.ly = 256u / g.lx;
    if (tune.max_side) g.ly = std::min(g.ly, tune.max_side);
    const uint64_t groups = tune.groups ? tune.groups : 1024u;
    const uint64_t block_rows = (uint64_t)kSimBlockRows * g.ly;
    const uint64_t total = g.tiles * ((sig + block_rows - 1) / block_rows);      // blocks of all work-groups
    const uint64_t per = std::min<uint64_t>(kSimFlushBlocks, std::max<uint64_t>(1, (total + groups - 1) / groups));
    g.slab_rows = per * block_rows;
    g.slabs = std::max<uint64_t>(1, (sig + g.slab_rows - 1) / g.slab_rows);
    return g;
}

hipError_t launch_ref_rows(const RefRowsArgs& a, hipStream_t stream) {
    if (a.sig == 0) return hipSuccess;
    if (a.nrefs > (uint32_t)kSimRefs) return hipErrorInvalidValue;
    const uint64_t blocks = (a.sig + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ref_rows_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sim_zero(unsigned long long* out, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sim_zero_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, out, n);
    return hipGetLastError();
}

hipError_t launch_shared_count(SimArgs a, hipStream_t stream, const SimTune& tune) {
    if (a.sig == 0 || a.valid_bytes == 0 || a.nrefs == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || a.valid_bytes > a.pitch || a.nrefs > (uint32_t)kSimRefs) return hipErrorInvalidValue;
    if (a.nslots != a.valid_bytes * 8u) return hipErrorInvalidValue;
    const SimGeom g = sim_geometry(a.sig, a.valid_bytes, tune);
    if (g.lx == 0 || g.ly == 0 || g.tiles * g.slabs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.slab_rows = g.slab_rows;
    a.tiles = g.tiles;
    a.lx = g.lx;
    a.ly = g.ly;
    const dim3 grid((uint32_t)(g.tiles * g.slabs));
    if (g.lx == 64u) hipLaunchKernelGGL((shared_count_kernel<kSimRefs, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((shared_count_kernel<kSimRefs, false>), grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
