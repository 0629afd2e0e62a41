// cobs_amd/csrc/best_kernels.hip -- best-of-group search on the device (cobs_gpu_search_best, best.cpp).
//
// group_best_kernel runs behind the scan of every pass, in the tile shape of group_accumulate_kernel: it reads the pass's
// score rows ONCE, 16 bytes per lane along the slot dimension, four rows in flight.  A work-group owns 256 x 16 bytes of
// slots of one span of queries of one group; every lane keeps (score, positions, query, ties) of the best member so far
// for its 4 / 8 / 16 slots in registers while it walks the span, and merges them into the stored state once.  Its bound
// is the score matrix: nq x nslots x score bytes read, plus 16 bytes per (span, slot) read and written.
//
// No atomics: a cell's state is four words ordered by a comparison of products.  Every cell has ONE writer per launch --
// the work-group of the only span of its group, which merges into the stored state read-modify-write (passes are ordered
// on the stream) --, or the group's queries are split over several spans that write partial states [piece][slot], and
// group_best_merge_kernel folds those into the stored state with the same merge.
//
// group_best_select_kernel runs once, after the last pass: documents whose best member reaches its own threshold are
// appended to a pool with one atomic per wave (ballot + popcount), the pattern of group_select_kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "best_kernels.hpp"
#include "score_rows.hpp"

namespace cobs_amd {
namespace {

// The empty state is written by a kernel, not by memset nodes (group_kernels.hip, group_zero_kernel).
__global__ __launch_bounds__(256) void best_init_kernel(BestState s, uint64_t ncells) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const uint64_t nvec = ncells / 4u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += stride) {
        reinterpret_cast<u32x4*>(s.score)[i] = u32x4{0u, 0u, 0u, 0u};
        reinterpret_cast<u32x4*>(s.positions)[i] = u32x4{0u, 0u, 0u, 0u};
        reinterpret_cast<u32x4*>(s.query)[i] = u32x4{kBestNone, kBestNone, kBestNone, kBestNone};
        reinterpret_cast<u32x4*>(s.ties)[i] = u32x4{0u, 0u, 0u, 0u};
    }
    for (uint64_t i = nvec * 4u + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < ncells; i += stride) {
        s.score[i] = 0u;
        s.positions[i] = 0u;
        s.query[i] = kBestNone;
        s.ties[i] = 0u;
    }
}

// (s, p, q, t) <- the merge of (s, p, q, t) and (s2, p2, q2, t2): the definition of cobs_gpu_batch.h on two states.  The
// fractions s / p are compared as 64-bit cross products, p = 0 (which implies s = 0) as 0 / 1; at equal fraction the ties
// add up and the larger score, then the lower query wins.  A total preorder on the fractions: associative, commutative,
// (0, 0, kBestNone, 0) the identity.
__device__ __forceinline__ void best_merge(uint32_t& s, uint32_t& p, uint32_t& q, uint32_t& t, uint32_t s2, uint32_t p2,
                                           uint32_t q2, uint32_t t2) {
    const uint64_t x = (uint64_t)s2 * max(p, 1u), y = (uint64_t)s * max(p2, 1u);
    const bool gt = x > y, eq = x == y;
    const bool win = gt || (eq && (s2 > s || (s2 == s && q2 < q)));
    t = gt ? t2 : eq ? t + t2 : t;
    s = win ? s2 : s;
    p = win ? p2 : p;
    q = win ? q2 : q;
}

__device__ __forceinline__ void best_merge4(u32x4& s, u32x4& p, u32x4& q, u32x4& t, const u32x4& s2, const u32x4& p2,
                                            const u32x4& q2, const u32x4& t2) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        uint32_t a = s[k], b = p[k], c = q[k], d = t[k];
        best_merge(a, b, c, d, s2[k], p2[k], q2[k], t2[k]);
        s[k] = a;
        p[k] = b;
        q[k] = c;
        t[k] = d;
    }
}

template <typename ST>
__global__ __launch_bounds__(256) void group_best_kernel(BestArgs a) {
    constexpr uint32_t E = 16u / sizeof(ST);            // slots per lane
    constexpr uint32_t U = E > 8u ? E / 8u : 1u;        // file units per lane: 8 slots never straddle two files
    constexpr uint32_t UE = E / U;
    const uint32_t span_no = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - span_no * a.tiles;
    const BestSpan sp = a.spans[span_no];
    const uint64_t s0 = ((uint64_t)tile * 256u + threadIdx.x) * E;
    if (s0 >= a.nslots) return;
    const bool half = s0 + E > a.nslots;                // (u8 only: nslots is a multiple of 8)
    // P of the lane's slots: the file is found once, P read once per query
    const uint32_t* pos[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        pos[u] = nullptr;
        const uint64_t s = s0 + (uint64_t)u * UE;
        for (uint32_t f = 0; f < a.nfiles; ++f)
            if (s >= a.files[f].begin && s < a.files[f].end) pos[u] = a.files[f].pos;
    }
    const uint64_t row_bytes = a.nslots * sizeof(ST);
    const uint8_t* p = static_cast<const uint8_t*>(a.rows) + s0 * sizeof(ST);
    // the span's first member is the best so far
    uint32_t bs[E], bp[E], bq[E], bt[E];
    {
        const u32x4 v = load_scores(p + (uint64_t)sp.q0 * row_bytes, half);
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            bs[j] = score_of<ST>(v, j);
            bp[j] = pos[j / UE] ? pos[j / UE][sp.q0] : 0u;
            bq[j] = sp.q0;
            bt[j] = 1u;
        }
    }
    // Member q against the best so far, which has the lower index.  The scores and P of a pass of u8 or u16 rows are
    // below 2^16: their cross products are exact in 32 bits; u32 rows take the 64-bit products.
    auto take = [&](const u32x4& v, const uint32_t (&P)[U], uint32_t q) {
        uint32_t pe[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) pe[u] = max(P[u], 1u);
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            const uint32_t s = score_of<ST>(v, j);
            const uint32_t bpe = max(bp[j], 1u);
            bool gt, eq;
            if (sizeof(ST) == 4) {
                const uint64_t x = (uint64_t)s * bpe, y = (uint64_t)bs[j] * pe[j / UE];
                gt = x > y;
                eq = x == y;
            } else {
                const uint32_t x = __umul24(s, bpe), y = __umul24(bs[j], pe[j / UE]);
                gt = x > y;
                eq = x == y;
            }
            const bool win = gt || (eq && s > bs[j]);
            bt[j] = gt ? 1u : bt[j] + (eq ? 1u : 0u);
            bs[j] = win ? s : bs[j];
            bp[j] = win ? P[j / UE] : bp[j];
            bq[j] = win ? q : bq[j];
        }
    };
    uint32_t q = sp.q0 + 1u;
    // four rows in flight per lane
    for (; q + 4u <= sp.q1; q += 4u) {
        u32x4 v[4];
        uint32_t P[4][U];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            v[i] = load_scores(p + (uint64_t)(q + i) * row_bytes, half);
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) P[i][u] = pos[u] ? pos[u][q + i] : 0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) take(v[i], P[i], q + i);
    }
    for (; q < sp.q1; ++q) {
        const u32x4 v = load_scores(p + (uint64_t)q * row_bytes, half);
        uint32_t P[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) P[u] = pos[u] ? pos[u][q] : 0u;
        take(v, P, q);
    }
    const uint32_t n = half ? 8u : E;
    const bool own = sp.piece == kBestNone;
    // (state rows are 32-byte aligned, s0 a multiple of 4)
    const uint64_t at = (uint64_t)(own ? sp.group : sp.piece) * a.nslots + s0;
    const BestState& dst = own ? a.state : a.part;
#pragma unroll
    for (uint32_t j = 0; j < E; j += 4u) {
        if (j >= n) break;
        u32x4 s{bs[j], bs[j + 1u], bs[j + 2u], bs[j + 3u]}, ps{bp[j], bp[j + 1u], bp[j + 2u], bp[j + 3u]};
        u32x4 qs{bq[j], bq[j + 1u], bq[j + 2u], bq[j + 3u]}, ts{bt[j], bt[j + 1u], bt[j + 2u], bt[j + 3u]};
        qs += u32x4{a.query0, a.query0, a.query0, a.query0};
        if (own) {
            // the only writer of these cells in this launch: what earlier passes stored is merged in
            u32x4 s1 = *reinterpret_cast<const u32x4*>(dst.score + at + j), p1 = *reinterpret_cast<const u32x4*>(dst.positions + at + j);
            u32x4 q1 = *reinterpret_cast<const u32x4*>(dst.query + at + j), t1 = *reinterpret_cast<const u32x4*>(dst.ties + at + j);
            best_merge4(s1, p1, q1, t1, s, ps, qs, ts);
            s = s1;
            ps = p1;
            qs = q1;
            ts = t1;
        }
        *reinterpret_cast<u32x4*>(dst.score + at + j) = s;
        *reinterpret_cast<u32x4*>(dst.positions + at + j) = ps;
        *reinterpret_cast<u32x4*>(dst.query + at + j) = qs;
        *reinterpret_cast<u32x4*>(dst.ties + at + j) = ts;
    }
}

// one lane per 4 slots of one fold: the group's partial states, in piece order, into the stored state
__global__ __launch_bounds__(256) void group_best_merge_kernel(BestMergeArgs a, uint32_t tiles) {
    const uint32_t fold_no = blockIdx.x / tiles;
    const uint32_t tile = blockIdx.x - fold_no * tiles;
    const uint64_t s0 = ((uint64_t)tile * 256u + threadIdx.x) * 4u;
    if (s0 >= a.nslots) return;                          // (nslots is a multiple of 8: the 4 slots exist)
    const BestFold fd = a.folds[fold_no];
    const uint64_t at = (uint64_t)fd.group * a.nslots + s0;
    u32x4 s = *reinterpret_cast<const u32x4*>(a.state.score + at), p = *reinterpret_cast<const u32x4*>(a.state.positions + at);
    u32x4 q = *reinterpret_cast<const u32x4*>(a.state.query + at), t = *reinterpret_cast<const u32x4*>(a.state.ties + at);
    for (uint32_t piece = fd.piece0; piece < fd.piece1; ++piece) {
        const uint64_t pa = (uint64_t)piece * a.nslots + s0;
        best_merge4(s, p, q, t, *reinterpret_cast<const u32x4*>(a.part.score + pa), *reinterpret_cast<const u32x4*>(a.part.positions + pa),
                    *reinterpret_cast<const u32x4*>(a.part.query + pa), *reinterpret_cast<const u32x4*>(a.part.ties + pa));
    }
    *reinterpret_cast<u32x4*>(a.state.score + at) = s;
    *reinterpret_cast<u32x4*>(a.state.positions + at) = p;
    *reinterpret_cast<u32x4*>(a.state.query + at) = q;
    *reinterpret_cast<u32x4*>(a.state.ties + at) = t;
}

// one lane per slot, blockIdx.y strides over the groups; every lane of a wave takes part in the ballot.  The threshold is
// formed from the cell's own positions, in double as the host forms it.
__global__ __launch_bounds__(256) void group_best_select_kernel(BestSelArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool real = false;
    GroupRange rg{0u, 0u, 0u, 0u};
    if (s < a.nslots)
        for (uint32_t r = 0; r < a.nranges; ++r)
            if (s >= a.ranges[r].begin && s < a.ranges[r].end) { rg = a.ranges[r]; real = true; }
    for (uint32_t g = blockIdx.y; g < a.n_groups; g += gridDim.y) {
        uint32_t score = 0u, positions = 0u, query = kBestNone;
        bool in = false;
        if (real) {
            const uint64_t at = (uint64_t)g * a.nslots + s;
            score = a.state.score[at];
            positions = a.state.positions[at];
            query = a.state.query[at];
            in = query != kBestNone;                     // (a group without members reports nothing)
            if (in && a.threshold > 0.0) in = (double)score >= fmax(ceil(a.threshold * (double)positions), 1.0);
        }
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        unsigned long long base = 0ull;
        if (lane == 0u) base = atomicAdd(a.fill, (unsigned long long)__popcll(mask));
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, 0), hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0);
        const uint64_t to = ((uint64_t)hi << 32 | lo) + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (in && to < a.cap)
            a.pool[to] = BestRec{g, rg.file, rg.doc0 + (uint32_t)(s - rg.begin), query, score, positions,
                                 a.state.ties[(uint64_t)g * a.nslots + s]};
    }
}

}  // namespace

hipError_t launch_best_init(const BestState& s, uint64_t ncells, hipStream_t stream) {
    if (ncells == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((ncells / 4u + 255u) / 256u + 1u, 4096u);
    hipLaunchKernelGGL(best_init_kernel, dim3(blocks), dim3(256), 0, stream, s, ncells);
    return hipGetLastError();
}

hipError_t launch_group_best(const BestArgs& a, hipStream_t stream) {
    if (a.nspans == 0 || a.nslots == 0) return hipSuccess;
    if ((a.nslots % 8u) != 0 || a.tiles == 0 || (uint64_t)a.tiles * group_tile_slots(a.score_bytes) < a.nslots ||
        (uint64_t)a.nspans * a.tiles > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const dim3 grid(a.nspans * a.tiles);
    if (a.score_bytes == 1) hipLaunchKernelGGL(group_best_kernel<uint8_t>, grid, dim3(256), 0, stream, a);
    else if (a.score_bytes == 2) hipLaunchKernelGGL(group_best_kernel<uint16_t>, grid, dim3(256), 0, stream, a);
    else if (a.score_bytes == 4) hipLaunchKernelGGL(group_best_kernel<uint32_t>, grid, dim3(256), 0, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_group_best_merge(const BestMergeArgs& a, hipStream_t stream) {
    if (a.nfolds == 0 || a.nslots == 0) return hipSuccess;
    const uint64_t tiles = (a.nslots + 1023u) / 1024u;
    if ((a.nslots % 8u) != 0 || tiles * a.nfolds > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_best_merge_kernel, dim3((uint32_t)(tiles * a.nfolds)), dim3(256), 0, stream, a, (uint32_t)tiles);
    return hipGetLastError();
}

hipError_t launch_group_best_select(const BestSelArgs& a, hipStream_t stream) {
    if (a.n_groups == 0 || a.nslots == 0 || a.nranges == 0) return hipSuccess;
    const uint64_t bx = (a.nslots + 255u) / 256u;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_best_select_kernel, dim3((uint32_t)bx, std::min<uint32_t>(a.n_groups, 65535u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
