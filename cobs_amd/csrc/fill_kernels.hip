// cobs_amd/csrc/fill_kernels.hip -- per-document filter fill on the device (cobs_gpu_doc_bits, fill.cpp).
//
// bits(d) of a sub-index = the rows whose bit d is set: a vertical popcount of the bit-sliced matrix, a pure sweep of the
// index ("filter fill").  gfx950, wave64.
//
// Mapping.  A lane owns one 16-byte column chunk (128 documents) and loads it with one 16-byte load per row.  The lx
// lanes of a column tile sit side by side along a row, so a wave's load is contiguous; where a row has fewer than 64
// chunks the remaining lanes of the work-group take further rows (ly = 256 / lx rows side by side), so a wave covers
// whole neighbouring rows.  The grid is (column tiles x row slabs, pages).  A lane walks its slab in blocks of 8 rows,
// all 8 loads of a block in flight at once.
//
// Arithmetic.  Per 32-bit column word a lane keeps kFillPlanes bit planes (plane k = bit k of the 32 documents' counts).
// The 8 row words of a block are folded into planes 0..2 by a Harley-Seal carry-save tree (7 adders of 2 three-input
// boolean ops each); only the block's carry into plane 3 ripples through the upper planes (2 ops per plane).  That is
// 14 + 2 x 9 = 32 ops per 8 words = 1 VALU op per byte, against 2 x 12 x 8 / 32 = 6 per byte when every row ripples.
// A row slab is at most kFillFlushBlocks blocks long (4088 rows < 2^12: the planes cannot overflow); at its end the lane
// expands its planes to per-document integers and adds them to the 64-bit output cells.  Lanes never combine with each
// other, each adds its own sums.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fill_kernels.hpp"
#include "wave_ops.hpp"      // csa

namespace cobs_amd {

namespace {

constexpr int NP = kFillPlanes;

// eight row words into the planes of one column word
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

// planes of one column word -> 32 per-document sums, added to the output (bytes beyond the slice's valid bytes -- the
// padding of the row pitch, which a stream buffer does not clear -- map to no slot and are dropped)
__device__ __forceinline__ void flush_word(const uint32_t (&pl)[NP], unsigned long long* out, uint32_t byte0, uint32_t valid_bytes) {
    for (uint32_t b = 0; b < 32u; ++b) {
        if (byte0 + (b >> 3) >= valid_bytes) break;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) v |= ((pl[k] >> b) & 1u) << k;
        if (v) atomicAdd(out + b, (unsigned long long)v);
    }
}

template <bool PROBE>
__global__ __launch_bounds__(256) void fill_count_kernel(FillArgs a, uint32_t* sink) {
    const PageDev pd = a.pages[a.page0 + blockIdx.y];
    const uint32_t tile = blockIdx.x % a.tiles;
    const uint64_t slab = a.slab0 + blockIdx.x / a.tiles;
    const uint64_t r_begin = slab * a.slab_rows;
    const uint32_t cx = threadIdx.x % a.lx, ry = threadIdx.x / a.lx;
    const uint32_t chunk = tile * a.lx + cx;
    if (r_begin >= pd.sig || ry >= a.ly || chunk * 16u >= pd.valid_bytes) return;
    const uint64_t r_end = min(pd.sig, r_begin + a.slab_rows);
    const uint8_t* col = a.data + pd.base + (uint64_t)chunk * 16u;
    unsigned long long* out = a.out + pd.slot0 + (uint64_t)chunk * 128u;
    const uint64_t step = (uint64_t)kFillBlockRows * a.ly;
    uint32_t pl[4][NP];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[w][k] = 0u;
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    for (uint64_t r = r_begin + ry; r < r_end; r += step) {
        uint4 X[kFillBlockRows];
#pragma unroll
        for (uint32_t i = 0; i < kFillBlockRows; ++i) {
            const uint64_t row = r + (uint64_t)i * a.ly;
            X[i] = make_uint4(0u, 0u, 0u, 0u);
            if (row < r_end) X[i] = *reinterpret_cast<const uint4*>(col + row * a.pitch);
        }
        if (PROBE) {
#pragma unroll
            for (uint32_t i = 0; i < kFillBlockRows; ++i) {
                acc.x ^= X[i].x; acc.y ^= X[i].y; acc.z ^= X[i].z; acc.w ^= X[i].w;
            }
            continue;
        }
        absorb8(pl[0], X[0].x, X[1].x, X[2].x, X[3].x, X[4].x, X[5].x, X[6].x, X[7].x);
        absorb8(pl[1], X[0].y, X[1].y, X[2].y, X[3].y, X[4].y, X[5].y, X[6].y, X[7].y);
        absorb8(pl[2], X[0].z, X[1].z, X[2].z, X[3].z, X[4].z, X[5].z, X[6].z, X[7].z);
        absorb8(pl[3], X[0].w, X[1].w, X[2].w, X[3].w, X[4].w, X[5].w, X[6].w, X[7].w);
    }
    if (PROBE) {
        const uint64_t lane = ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
        sink[lane] = acc.x ^ acc.y ^ acc.z ^ acc.w;
        return;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) flush_word(pl[w], out + 32 * w, chunk * 16u + 4u * w, pd.valid_bytes);
}

__global__ void fill_zero_kernel(unsigned long long* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0ull;
}

constexpr uint32_t kMaxGridY = 65535u;

template <bool PROBE>
hipError_t launch(const uint8_t* data, const PageDev* d_pages, const std::vector<PageDev>& pages, uint32_t pitch,
                  unsigned long long* out, uint32_t* sink, hipStream_t stream, uint64_t* bytes_read, const FillTune& tune) {
    if (pages.empty()) return hipSuccess;
    if (pitch == 0 || pitch % 16u != 0) return hipErrorInvalidValue;
    const FillGeom g = fill_geometry(pages, tune);
    if (g.lx == 0) return hipErrorInvalidValue;
    const uint64_t slabs_per_launch = 0x7FFFFFFFull / g.tiles;       // (one launch unless a sub-index has ~2^44 rows)
    if (PROBE && g.max_slabs > slabs_per_launch) return hipErrorInvalidValue;
    FillArgs a;
    a.data = data;
    a.pages = d_pages;
    a.out = out;
    a.slab_rows = g.slab_rows;
    a.pitch = pitch;
    a.tiles = g.tiles;
    a.lx = g.lx;
    a.ly = g.ly;
    for (size_t p0 = 0; p0 < pages.size(); p0 += kMaxGridY) {
        const uint32_t np = (uint32_t)std::min<size_t>(kMaxGridY, pages.size() - p0);
        a.page0 = (uint32_t)p0;
        uint32_t* s = PROBE ? sink + p0 * g.tiles * g.max_slabs * 256u : nullptr;
        for (uint64_t s0 = 0; s0 < g.max_slabs; s0 += slabs_per_launch) {
            a.slab0 = s0;
            const uint64_t ns = std::min(slabs_per_launch, g.max_slabs - s0);
            hipLaunchKernelGGL(fill_count_kernel<PROBE>, dim3((uint32_t)(g.tiles * ns), np), dim3(256), 0, stream, a, s);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    if (bytes_read)
        for (const PageDev& pd : pages) *bytes_read += pd.sig * (uint64_t)pd.valid_bytes;
    return hipSuccess;
}

}  // namespace

// Column tiles of at most 64 lanes, equal in width (a row of 98 chunks: two tiles of 49, not 64 + 34), the rest of the
// 256 lanes on further rows.  Row slabs: the longest a lane's planes can count (511 blocks) where that still gives the
// device 1024 work-groups (256 CUs x 16 waves), else the rows spread over 1024 work-groups -- so one large sub-index and
// 245 small ones both fill the device.  Every page of a launch uses the same slab length; a work-group whose slab lies
// beyond its page's rows returns at once.
FillGeom fill_geometry(const std::vector<PageDev>& pages, const FillTune& tune) {
    FillGeom g{};
    uint32_t valid = 0;
    uint64_t max_sig = 0;
    for (const PageDev& pd : pages) {
        valid = std::max(valid, pd.valid_bytes);
        max_sig = std::max(max_sig, pd.sig);
    }
    const uint32_t chunks = (valid + 15u) / 16u;
    if (chunks == 0) return g;
    g.tiles = (chunks + 63u) / 64u;
    g.lx = (chunks + g.tiles - 1u) / g.tiles;
    g.ly = 256u / g.lx;
    if (tune.max_side) g.ly = std::min(g.ly, tune.max_side);
    const uint64_t groups = tune.groups ? tune.groups : 1024u;
    const uint64_t block_rows = (uint64_t)kFillBlockRows * g.ly;
    uint64_t total = 0;                                     // blocks of all work-groups
    for (const PageDev& pd : pages) total += g.tiles * ((pd.sig + block_rows - 1) / block_rows);
    const uint64_t per = std::min<uint64_t>(kFillFlushBlocks, std::max<uint64_t>(1, (total + groups - 1) / groups));
    g.slab_rows = per * block_rows;
    g.max_slabs = std::max<uint64_t>(1, (max_sig + g.slab_rows - 1) / g.slab_rows);
    return g;
}

hipError_t launch_fill_zero(unsigned long long* out, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_zero_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, out, n);
    return hipGetLastError();
}

hipError_t launch_fill_count(const uint8_t* data, const PageDev* d_pages, const std::vector<PageDev>& pages, uint32_t pitch,
                             unsigned long long* out, hipStream_t stream, uint64_t* bytes_read, const FillTune& tune) {
    return launch<false>(data, d_pages, pages, pitch, out, nullptr, stream, bytes_read, tune);
}

uint64_t fill_probe_lanes(const std::vector<PageDev>& pages, const FillTune& tune) {
    const FillGeom g = fill_geometry(pages, tune);
    return (uint64_t)pages.size() * g.tiles * g.max_slabs * 256u;
}

hipError_t launch_fill_probe(const uint8_t* data, const PageDev* d_pages, const std::vector<PageDev>& pages, uint32_t pitch,
                             uint32_t* sink, hipStream_t stream, const FillTune& tune) {
    return launch<true>(data, d_pages, pages, pitch, nullptr, sink, stream, nullptr, tune);
}

}  // namespace cobs_amd
