// cobs_amd/csrc/group_kernels.hip -- grouped search on the device (cobs_gpu_search_groups, groups.cpp).
//
// group_accumulate_kernel runs behind the scan of every pass: it reads the pass's score rows ONCE, 16 bytes per lane
// along the slot dimension, and adds every row to the sums and votes of its query's group.  A work-group owns 256 x 16
// bytes of slots of one span of queries of one group; every lane keeps its 4 / 8 / 16 sums and votes in registers
// (widened to 32 bit) while it walks the span's queries, and writes them once.  Its bound is the score matrix:
// nq x nslots x score bytes read, plus 8 bytes per (span, slot) written.
//
// group_select_kernel runs once, after the last pass: documents whose sum reaches the group's threshold are appended
// to a pool with one atomic per wave (ballot + popcount), the pattern of the scan's threshold epilogue.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "group_kernels.hpp"
#include "score_rows.hpp"

namespace cobs_amd {
namespace {

// Accumulators are zeroed by a kernel, not a memset node (fetch_kernels.hip, clear_flags_kernel: a captured memset node
// replayed stale host data; a kernel carries its arguments by value).
__global__ __launch_bounds__(256) void group_zero_kernel(uint32_t* p, uint64_t nwords) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const uint64_t nvec = nwords / 4u;
    u32x4* v = reinterpret_cast<u32x4*>(p);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += stride) v[i] = u32x4{0u, 0u, 0u, 0u};
    for (uint64_t i = nvec * 4u + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += stride) p[i] = 0u;
}

template <typename ST>
__global__ __launch_bounds__(256) void group_accumulate_kernel(GroupAccArgs a) {
    constexpr uint32_t E = 16u / sizeof(ST);            // slots per lane
    constexpr uint32_t U = E > 8u ? E / 8u : 1u;        // threshold units per lane: 8 slots never straddle two files
    constexpr uint32_t UE = E / U;
    const uint32_t span_no = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - span_no * a.tiles;
    const GroupSpan sp = a.spans[span_no];
    const uint64_t s0 = ((uint64_t)tile * 256u + threadIdx.x) * E;
    if (s0 >= a.nslots) return;
    const bool half = s0 + E > a.nslots;                // (u8 only: nslots is a multiple of 8)
    // the thresholds of the lane's slots: found once, read once per query
    const uint32_t* thr[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        thr[u] = nullptr;
        const uint64_t s = s0 + (uint64_t)u * UE;
        for (uint32_t f = 0; f < a.nfiles; ++f)
            if (s >= a.files[f].begin && s < a.files[f].end) thr[u] = a.files[f].thr;
    }
    uint32_t sum[E], votes[E];
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) sum[j] = votes[j] = 0u;
    const uint64_t row_bytes = a.nslots * sizeof(ST);
    const uint8_t* p = static_cast<const uint8_t*>(a.rows) + s0 * sizeof(ST);
    auto add = [&](const u32x4& v, const uint32_t (&t)[U]) {
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            const uint32_t s = score_of<ST>(v, j);
            sum[j] += s;
            votes[j] += s >= t[j / UE] ? 1u : 0u;
        }
    };
    uint32_t q = sp.q0;
    // four rows in flight per lane
    for (; q + 4u <= sp.q1; q += 4u) {
        u32x4 v[4];
        uint32_t t[4][U];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            v[i] = load_scores(p + (uint64_t)(q + i) * row_bytes, half);
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) t[i][u] = thr[u] ? thr[u][q + i] : 0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) add(v[i], t[i]);
    }
    for (; q < sp.q1; ++q) {
        const u32x4 v = load_scores(p + (uint64_t)q * row_bytes, half);
        uint32_t t[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) t[u] = thr[u] ? thr[u][q] : 0u;
        add(v, t);
    }
    uint32_t* ps = a.acc_sum + (uint64_t)sp.group * a.nslots + s0;
    uint32_t* pv = a.acc_votes + (uint64_t)sp.group * a.nslots + s0;
    const uint32_t n = half ? 8u : E;
    if (sp.atomic) {
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            if (j < n && sum[j]) atomicAdd(ps + j, sum[j]);
            if (j < n && votes[j]) atomicAdd(pv + j, votes[j]);
        }
    } else {
        // the only writer of these cells in this launch (accumulator rows are 32-byte aligned, s0 a multiple of 4)
#pragma unroll
        for (uint32_t j = 0; j < E; j += 4u) {
            if (j >= n) break;
            u32x4 s = *reinterpret_cast<u32x4*>(ps + j), v = *reinterpret_cast<u32x4*>(pv + j);
            s += u32x4{sum[j], sum[j + 1u], sum[j + 2u], sum[j + 3u]};
            v += u32x4{votes[j], votes[j + 1u], votes[j + 2u], votes[j + 3u]};
            *reinterpret_cast<u32x4*>(ps + j) = s;
            *reinterpret_cast<u32x4*>(pv + j) = v;
        }
    }
}

// one lane per slot, blockIdx.y strides over the groups; every lane of a wave takes part in the ballot
__global__ __launch_bounds__(256) void group_select_kernel(GroupSelArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool real = false;
    GroupRange rg{0u, 0u, 0u, 0u};
    if (s < a.nslots)
        for (uint32_t r = 0; r < a.nranges; ++r)
            if (s >= a.ranges[r].begin && s < a.ranges[r].end) { rg = a.ranges[r]; real = true; }
    for (uint32_t g = blockIdx.y; g < a.n_groups; g += gridDim.y) {
        uint32_t sum = 0u;
        bool in = false;
        if (real) {
            sum = a.acc_sum[(uint64_t)g * a.nslots + s];
            in = (uint64_t)sum >= a.gthr[(uint64_t)rg.file * a.n_groups + g];
        }
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        unsigned long long base = 0ull;
        if (lane == 0u) base = atomicAdd(a.fill, (unsigned long long)__popcll(mask));
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, 0), hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0);
        const uint64_t at = ((uint64_t)hi << 32 | lo) + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (in && at < a.cap)
            a.pool[at] = GroupRec{g, rg.file, rg.doc0 + (uint32_t)(s - rg.begin), sum, a.acc_votes[(uint64_t)g * a.nslots + s]};
    }
}

}  // namespace

hipError_t launch_group_zero(uint32_t* p, uint64_t nwords, hipStream_t stream) {
    if (nwords == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((nwords / 4u + 255u) / 256u + 1u, 4096u);
    hipLaunchKernelGGL(group_zero_kernel, dim3(blocks), dim3(256), 0, stream, p, nwords);
    return hipGetLastError();
}

hipError_t launch_group_accumulate(const GroupAccArgs& a, hipStream_t stream) {
    if (a.nspans == 0 || a.nslots == 0) return hipSuccess;
    if ((a.nslots % 8u) != 0 || a.tiles == 0 || (uint64_t)a.tiles * group_tile_slots(a.score_bytes) < a.nslots ||
        (uint64_t)a.nspans * a.tiles > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const dim3 grid(a.nspans * a.tiles);
    if (a.score_bytes == 1) hipLaunchKernelGGL(group_accumulate_kernel<uint8_t>, grid, dim3(256), 0, stream, a);
    else if (a.score_bytes == 2) hipLaunchKernelGGL(group_accumulate_kernel<uint16_t>, grid, dim3(256), 0, stream, a);
    else if (a.score_bytes == 4) hipLaunchKernelGGL(group_accumulate_kernel<uint32_t>, grid, dim3(256), 0, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_group_select(const GroupSelArgs& a, hipStream_t stream) {
    if (a.n_groups == 0 || a.nslots == 0 || a.nranges == 0) return hipSuccess;
    const uint64_t bx = (a.nslots + 255u) / 256u;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel, dim3((uint32_t)bx, std::min<uint32_t>(a.n_groups, 65535u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
