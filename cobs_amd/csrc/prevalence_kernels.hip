// cobs_amd/csrc/prevalence_kernels.hip -- gfx950 kernel of cobs_gpu_prevalence: for every position of a query the number
// of real documents that hold it.  K2's gather reduced along the other axis: the rows looked up are the same, the
// reduction runs across the documents of a row instead of across the terms of a query.  wave64.
//
// Mapping.  A lane owns one 16-byte column chunk (128 documents) of one position and loads it with one 16-byte load per
// looked-up row.  The lx lanes of a position sit side by side along the row, so a wave's load is contiguous; where a row
// has fewer than 64 chunks the remaining lanes of the wave take further positions (ly = 64 / lx positions side by side:
// a sub-index of 2 row bytes keeps all 64 lanes busy on 64 positions).  Rows wider than 64 chunks loop with stride 64.
// The grid is (queries, position slabs, pages of the chunk); a wave walks its positions two groups at a time, the loads
// of both in flight at once.
//
// Per (position, slice): AND of the H x (z + 1) addressed rows (findere: terms p .. p + z), everything that is no real
// document masked away -- the bytes at or beyond the slice's valid width, the bits at or beyond the file's last document
// -- popcount, a sum over the lx lanes in DPP steps of the VALU, and ONE atomicAdd into the position's cell.  A slice
// without a real document (a trailing sub-index of padding) returns before any load.  Positions at or beyond n = T - z
// are never written, and since p + z < T for every p < n no term at or beyond T is ever looked up.
//
// Bound: the read-only gather rate.  At z = 0 the bytes are K2's for the same batch (positions x H x row bytes per held
// sub-index) and 4 bytes per (position, slice) of atomics; at z > 0 every row is read z + 1 times, z of them from cache.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "prevalence_kernels.hpp"
#include "wave_ops.hpp"      // group_sum_last, low_bits, dispatch_idx_flag

namespace cobs_amd {

// H1: one hash function (the COBS default), no loop over the hashes
template <typename IdxT, bool H1>
__global__ __launch_bounds__(256) void prevalence_kernel(PrevalenceArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x;
    const PageDev pd = a.pages[a.page0 + blockIdx.z];
    // real documents of the slice: its slots [doc0, doc0 + 8 * valid_bytes) below the file's document count
    // (an early return, not `num_docs > doc0 ? min(num_docs - doc0, ...) : 0`: for that form, with uniform operands, the
    // compiler emitted s_sub_i32 + s_min_u32 and no comparison -- a trailing sub-index of padding then counted as
    // 8 * valid_bytes live documents; test_gpu_prevalence.py's unmasked fixture found it)
    if (a.num_docs <= pd.doc0 || pd.valid_bytes == 0u) return;      // (uniform: a slice of padding documents only)
    const uint32_t live = min(a.num_docs - pd.doc0, pd.valid_bytes * 8u);
    const uint32_t z = a.t.findere;
    const uint32_t n = a.t.q_len[q] - a.t.term_size + 1u - z;   // the host made sure T > z
    const uint32_t H = H1 ? 1u : a.t.num_hashes;
    const RowTable<IdxT> tab(a.t, q, pd.tpage, H);
    const uint8_t* __restrict__ rows = a.data + pd.base;
    uint32_t* __restrict__ out = a.out + a.seg_off[(uint64_t)q * a.seg_stride];
    const uint32_t lx = a.lx, ly = a.ly;
    const uint32_t cx = lane & (lx - 1u), py = lane / lx;
    const uint32_t groups = (n + ly - 1u) / ly;
    const uint32_t nw = gridDim.y * 4u;

    // documents of column chunk `chunk` (128 slots from 128 * chunk) that hold position p
    auto count = [&](uint32_t p, uint32_t chunk) -> uint32_t {
        uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u);
        const uint8_t* col = rows + (uint64_t)chunk * 16u;
        for (uint32_t s = 0; s <= z; ++s) {
            const IdxT* e = tab.term(p + s);
            if (H1) {
                const uint4 x = *reinterpret_cast<const uint4*>(col + (uint64_t)e[0] * a.pitch);
                acc.x &= x.x; acc.y &= x.y; acc.z &= x.z; acc.w &= x.w;
            } else {
                for (uint32_t j = 0; j < H; ++j) {
                    const uint4 x = *reinterpret_cast<const uint4*>(col + (uint64_t)e[j * kRowTableLanes] * a.pitch);
                    acc.x &= x.x; acc.y &= x.y; acc.z &= x.z; acc.w &= x.w;
                }
            }
        }
        const uint32_t rem = live - chunk * 128u;            // > 0: the caller's loop stops at the last live chunk
        return __popc(acc.x & low_bits(rem)) + (rem > 32u ? __popc(acc.y & low_bits(rem - 32u)) : 0u) +
               (rem > 64u ? __popc(acc.z & low_bits(rem - 64u)) : 0u) + (rem > 96u ? __popc(acc.w & low_bits(rem - 96u)) : 0u);
    };

    for (uint32_t g = blockIdx.y * 4u + wave; g < groups; g += 2u * nw) {      // (uniform per wave)
        const uint32_t p0 = g * ly + py, p1 = p0 + nw * ly;
        const bool in0 = p0 < n, in1 = (uint64_t)g + nw < groups && p1 < n;    // (the last group may be partly filled)
        uint32_t c0 = 0u, c1 = 0u;
        for (uint32_t chunk = cx; chunk * 128u < live; chunk += lx) {
            if (in0) c0 += count(p0, chunk);
            if (in1) c1 += count(p1, chunk);
        }
        c0 = group_sum_last(c0, lx);
        c1 = group_sum_last(c1, lx);
        if (cx == lx - 1u) {
            if (in0 && c0 != 0u) atomicAdd(out + p0, c0);
            if (in1 && c1 != 0u) atomicAdd(out + p1, c1);
        }
    }
}

__global__ void prevalence_zero_kernel(uint32_t* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0u;
}

uint32_t prevalence_lx(uint32_t valid_bytes) {
    const uint32_t chunks = (valid_bytes + 15u) / 16u;
    uint32_t lx = 1;
    while (lx < chunks && lx < 64u) lx *= 2u;
    return lx;
}

// The cells back to zero by a kernel, not a memset node (fetch_kernels.hip: clear_flags_kernel says why).
hipError_t launch_prevalence_zero(uint32_t* out, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prevalence_zero_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, out, n);
    return hipGetLastError();
}

hipError_t launch_prevalence(PrevalenceArgs a, const std::vector<PageDev>& pages, uint32_t nq, uint32_t max_positions,
                             hipStream_t stream) {
    if (pages.empty() || nq == 0 || max_positions == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || nq > 0x7FFFFFFFu) return hipErrorInvalidValue;
    uint32_t valid = 0;
    for (const PageDev& pd : pages) {
        if (pd.valid_bytes > a.pitch) return hipErrorInvalidValue;
        valid = std::max(valid, pd.valid_bytes);
    }
    a.lx = prevalence_lx(valid);
    a.ly = 64u / a.lx;
    // four waves per work-group, two position groups per wave and trip: up to four trips per wave, then more slabs
    const uint32_t groups = (max_positions + a.ly - 1u) / a.ly;
    const uint32_t gy = std::min(1024u, (groups + 31u) / 32u);
    constexpr size_t kMaxGridZ = 65535;
    for (size_t p0 = 0; p0 < pages.size(); p0 += kMaxGridZ) {
        a.page0 = (uint32_t)p0;
        const dim3 grid(nq, gy, (uint32_t)std::min(kMaxGridZ, pages.size() - p0)), block(256);
        dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
            hipLaunchKernelGGL((prevalence_kernel<decltype(idx), decltype(h1)::value>), grid, block, 0, stream, a);
        });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cobs_amd
