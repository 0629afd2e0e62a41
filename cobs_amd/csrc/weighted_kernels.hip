// cobs_amd/csrc/weighted_kernels.hip -- gfx950 kernels of cobs_gpu_search_weighted: a document's score is the SUM OF THE
// WEIGHTS of the query positions it holds, where K2 (kernels.hip) counts every position as 1.  wave64.
//
// weight_kernel.  One work-group per (query, file): cells of the prevalence kernel -> one byte per position,
// w = 0 for c = 0, else 1 + min(14, floor(log2(D / c))); 4 bytes read and 1 byte written per position.  The weights of a
// segment are summed in registers, across a wave with shuffles and across the four waves through LDS -- W(q, f) and the
// threshold max(1, ceil(threshold * W)) (double, as skip_thresholds_kernel makes its own) are written by one thread.
// Segments start at multiples of 8 and are padded to a multiple of 8 with weights of 0, so the scan reads the eight
// weights of a block with one 8-byte load.  5 bytes per position; 0.05 ms for ten million positions.
//
// weighted_scan_kernel.  K2's mapping: a work-group owns one query and one tile of W (a power of two, <= 64) sixteen-byte
// column chunks; a lane owns one chunk, 128 documents, as 4 column words x NP bit planes in registers.  The 8-position
// blocks of the query go round-robin over the 4 x 64 / W lane groups ("virtual waves"), whose partial counters are
// merged at the end (shuffles inside a wave, LDS across waves).  Per block a lane loads the eight looked-up rows
// (H = 1, z = 0: one 16-byte load per row, every row byte once per (query, chunk); otherwise the AND of the H x (z + 1)
// rows of every position, the window's extra rows coming from cache as in the prevalence kernel) and the block's eight
// weights.  Weights are uniform over a lane group, not over a wave (narrow tiles: the lane groups of a wave walk
// different positions), so a weight never steers control flow: for every weight bit b = 0..3 the eight row words are
// masked with -((w >> b) & 1) and go through a seven-CSA tree (v_bitop3_b32: two instructions per CSA) into planes
// b .. b + 2; the four carries, pending at planes 3 .. 6, enter the upper planes in ONE chain (a half adder, three CSAs,
// a ripple from plane 7) instead of four ripples.  No score leaves the registers: the epilogue compares the bit-sliced
// sums with the (query, file) threshold, masks everything that is no real document and appends the survivors to a pool
// as (query, file, document, score) with one atomic per wave.
// Algorithmic bytes: K2's row bytes + 1 byte per position.  Measured on the C3 headline batch (DESIGN 4 "Weighted search",
// profiles/weighted_times.txt): the scan is VALU-bound, not memory-bound -- about 470 VALU instructions per 128 row bytes
// and lane where K2 has about 140.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "weighted_kernels.hpp"
#include "wave_ops.hpp"      // csa, low_bits, pool_append, dispatch_idx_flag

namespace cobs_amd {

namespace {

// eight words into the three planes p[0..2]; returns the carry into the plane above them
__device__ __forceinline__ uint32_t absorb8(uint32_t* p, const uint32_t (&x)[8]) {
    uint32_t t2a, t2b, f4a, f4b, e8;
    csa(t2a, p[0], p[0], x[0], x[1]);
    csa(t2b, p[0], p[0], x[2], x[3]);
    csa(f4a, p[1], p[1], t2a, t2b);
    csa(t2a, p[0], p[0], x[4], x[5]);
    csa(t2b, p[0], p[0], x[6], x[7]);
    csa(f4b, p[1], p[1], t2a, t2b);
    csa(e8, p[2], p[2], f4a, f4b);
    return e8;
}

__device__ __forceinline__ uint32_t word_of(const uint4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// pl += sum over the eight positions t of weight_t * X[t], per document bit; w8 = the eight 4-bit weights, one per byte
template <int NP>
__device__ __forceinline__ void absorb_weighted(uint32_t (&pl)[4][NP], const uint4 (&X)[8], uint2 w8) {
    static_assert(NP >= 7, "the four carries enter planes 3 .. 6");
    uint32_t e[4][4];           // [word][weight bit]: carry pending at plane 3 + bit
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t m[8];          // all ones where bit b of the position's weight is set (v_bfe_i32)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t half = t < 4 ? w8.x : w8.y;
            m[t] = (uint32_t)((int32_t)(half << (31 - ((t & 3) * 8 + b))) >> 31);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = word_of(X[t], c) & m[t];
            e[c][b] = absorb8(&pl[c][b], x);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t k = pl[c][3] & e[c][0];
        pl[c][3] ^= e[c][0];
        csa(k, pl[c][4], pl[c][4], e[c][1], k);
        csa(k, pl[c][5], pl[c][5], e[c][2], k);
        csa(k, pl[c][6], pl[c][6], e[c][3], k);
#pragma unroll
        for (int p = 7; p < NP; ++p) {
            const uint32_t t = pl[c][p] & k;
            pl[c][p] ^= k;
            k = t;
        }
    }
}

__device__ __forceinline__ uint4 load_row(const uint8_t* lane_base, uint64_t row, uint32_t pitch) {
    return *reinterpret_cast<const uint4*>(lane_base + row * pitch);
}

// the eight row indices of one block (H = 1): two 16-byte loads, or four for 64-bit indices
__device__ __forceinline__ void issue_rows(uint4 (&X)[8], const uint8_t* lane_base, uint32_t pitch, const uint32_t* idx) {
    const uint4 a = *reinterpret_cast<const uint4*>(idx), b = *reinterpret_cast<const uint4*>(idx + 4);
    X[0] = load_row(lane_base, a.x, pitch); X[1] = load_row(lane_base, a.y, pitch);
    X[2] = load_row(lane_base, a.z, pitch); X[3] = load_row(lane_base, a.w, pitch);
    X[4] = load_row(lane_base, b.x, pitch); X[5] = load_row(lane_base, b.y, pitch);
    X[6] = load_row(lane_base, b.z, pitch); X[7] = load_row(lane_base, b.w, pitch);
}
__device__ __forceinline__ void issue_rows(uint4 (&X)[8], const uint8_t* lane_base, uint32_t pitch, const uint64_t* idx) {
#pragma unroll
    for (int t = 0; t < 8; t += 2) {
        const uint4 a = *reinterpret_cast<const uint4*>(idx + t);
        X[t] = load_row(lane_base, (uint64_t)a.y << 32 | a.x, pitch);
        X[t + 1] = load_row(lane_base, (uint64_t)a.w << 32 | a.z, pitch);
    }
}

}  // namespace

__global__ __launch_bounds__(256) void weight_kernel(WeightArgs a) {
    __shared__ uint32_t part[4];
    const uint32_t q = blockIdx.x;
    const uint64_t seg = a.seg_off[(uint64_t)q * a.seg_stride];
    const uint32_t n = a.q_len[q] - a.term_size + 1u - a.findere;      // the host made sure T > z
    const uint32_t npad = (n + 7u) & ~7u;
    const uint32_t* __restrict__ cells = a.cells + seg;
    uint8_t* __restrict__ out = a.weights + seg;
    uint32_t sum = 0u;
    for (uint32_t p = threadIdx.x; p < npad; p += 256u) {
        uint32_t w = 0u;
        if (p < n) {
            w = idf_weight(a.num_docs, cells[p]);
        }
        out[p] = (uint8_t)w;
        sum += w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint64_t W = (uint64_t)part[0] + part[1] + part[2] + part[3];
        a.total[(uint64_t)q * a.seg_stride] = W;
        uint32_t thr = 0u;
        if (a.threshold > 0.0) {
            const double v = ceil(a.threshold * (double)W);
            thr = !(v >= 1.0) ? 1u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
        }
        a.thr[q] = thr;
    }
}

// FAST: one hash function and z = 0 -- a position is one row
template <int NP, typename IdxT, bool FAST>
__global__ __launch_bounds__(256) void weighted_scan_kernel(WeightedScanArgs a) {
    __shared__ uint4 mbuf[2 * NP * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t W = a.tile_w, G = 64u / W;
    const uint32_t tile = blockIdx.x / a.nq;
    const uint32_t q = blockIdx.x - tile * a.nq;
    const uint32_t grp = lane / W, col = lane & (W - 1u);
    const uint32_t g = (a.tile0 + tile) * W + col;
    const bool live = g < a.total_chunks;
    const uint32_t gc = live ? g : a.total_chunks - 1u;         // dead lanes duplicate a live one
    const uint32_t pg = gc / a.cpp, ch = gc - pg * a.cpp;
    const PageDev pd = a.pages[pg];
    const uint8_t* lane_base = a.data + pd.base + (uint64_t)ch * 16u;
    const uint32_t pitch = a.pitch;
    const uint32_t H = FAST ? 1u : a.t.num_hashes, z = FAST ? 0u : a.t.findere;
    const RowTable<IdxT> tab(a.t, q, pd.tpage, H);
    const uint32_t n = a.t.q_len[q] - a.t.term_size + 1u - z;
    const uint32_t nb = (n + 7u) >> 3;                                  // blocks of positions (<= tab.nblk)
    const uint8_t* __restrict__ wts = a.weights + a.seg_off[(uint64_t)q * a.seg_stride];
    const uint32_t vw = wave * G + grp, NV = 4u * G;

    uint32_t pl[4][NP];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[c][k] = 0u;

    // trips of this wave (uniform): as many as its first lane group needs; a lane group that has run out walks the
    // padding block (the zero row) with weights of 0
    const uint32_t first = wave * G;
    const uint32_t trips = nb > first ? (nb - first + NV - 1u) / NV : 0u;
    if constexpr (FAST) {
        auto idx_of = [&](uint32_t i) -> const IdxT* {
            const uint32_t b = vw + i * NV;
            return tab.block(b < nb ? b : tab.padding_block());
        };
        auto wts_of = [&](uint32_t i) -> uint2 {
            const uint32_t b = vw + i * NV;
            return b < nb ? *reinterpret_cast<const uint2*>(wts + (uint64_t)b * 8u) : make_uint2(0u, 0u);
        };
        if constexpr (sizeof(IdxT) == 8) {
            // 64-bit row indices: one set of row registers (two sets took the 16-plane instantiation to 262 VGPRs, one
            // wave per SIMD); the waves of the SIMD hide each other's loads
            for (uint32_t i = 0; i < trips; ++i) {
                uint4 X[8];
                const uint2 w8 = wts_of(i);
                issue_rows(X, lane_base, pitch, idx_of(i));
                absorb_weighted<NP>(pl, X, w8);
            }
        } else if (trips > 0u) {
            // rows of trip i + 1 are in flight while trip i goes through the adder tree
            uint4 XA[8], XB[8];
            uint2 wa = wts_of(0), wb;
            issue_rows(XA, lane_base, pitch, idx_of(0));
            uint32_t i = 0;
            for (; i + 2u <= trips; i += 2u) {
                wb = wts_of(i + 1u);
                issue_rows(XB, lane_base, pitch, idx_of(i + 1u));
                absorb_weighted<NP>(pl, XA, wa);
                wa = wts_of(i + 2u);
                issue_rows(XA, lane_base, pitch, idx_of(i + 2u));       // (trip == trips: the padding block)
                absorb_weighted<NP>(pl, XB, wb);
            }
            if (i < trips) absorb_weighted<NP>(pl, XA, wa);
        }
    } else {
        for (uint32_t i = 0; i < trips; ++i) {
            const uint32_t b = vw + i * NV;
            if (b >= nb) continue;              // (no padding walk: a window at the padding block would leave the table)
            const uint2 w8 = *reinterpret_cast<const uint2*>(wts + (uint64_t)b * 8u);
            uint4 X[8];
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) {
                // positions n .. 8 * nb - 1 weigh 0; their terms p + s <= T + 6 lie in the query's blocks or its padding block
                const uint32_t p = b * 8u + t;
                uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u);
                for (uint32_t s = 0; s <= z; ++s) {
                    const uint32_t term = p + s;
                    const IdxT* e = tab.term(term);
                    for (uint32_t j = 0; j < H; ++j) {
                        const uint4 x = load_row(lane_base, (uint64_t)e[j * kRowTableLanes], pitch);
                        acc.x &= x.x; acc.y &= x.y; acc.z &= x.z; acc.w &= x.w;
                    }
                }
                X[t] = acc;
            }
            absorb_weighted<NP>(pl, X, w8);
        }
    }

    // ---- merge the lane groups of a wave (butterfly: every lane group ends with the wave's sum) ...
    for (uint32_t s = W; s < 64u; s <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t carry = 0u;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint32_t o = (uint32_t)__shfl_xor((int)pl[c][k], (int)s);
                uint32_t h;
                csa(h, pl[c][k], pl[c][k], o, carry);
                carry = h;
            }
        }
    }
    // ---- ... and the four waves (tree, bit-sliced adds)
#pragma unroll
    for (int s = 1; s < 4; s <<= 1) {
        uint4* buf = mbuf + (size_t)(wave / (2 * s)) * NP * 64;
        if ((wave & (2 * s - 1)) == (uint32_t)s) {
#pragma unroll
            for (int k = 0; k < NP; ++k) buf[k * 64 + lane] = make_uint4(pl[0][k], pl[1][k], pl[2][k], pl[3][k]);
        }
        __syncthreads();
        if ((wave & (2 * s - 1)) == 0u) {
            uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint4 o = buf[k * 64 + lane];
                uint32_t h;
                csa(h, pl[0][k], pl[0][k], o.x, c0); c0 = h;
                csa(h, pl[1][k], pl[1][k], o.y, c1); c1 = h;
                csa(h, pl[2][k], pl[2][k], o.z, c2); c2 = h;
                csa(h, pl[3][k], pl[3][k], o.w, c3); c3 = h;
            }
        }
        __syncthreads();
    }
    if (wave != 0u) return;

    // ---- epilogue (wave 0, its first lane group: one lane per chunk of the tile): score >= threshold in bit-sliced
    // form, over real documents only -- row bytes inside the slice's valid width, documents below the file's count
    const uint32_t thr = a.thr[q];
    uint32_t ge[4];
    uint32_t cnt = 0u;
    const bool mine = live && grp == 0u;
    const uint32_t vb = (mine && pd.valid_bytes > ch * 16u) ? min(pd.valid_bytes - ch * 16u, 16u) : 0u;
    const uint32_t doc0 = pd.doc0 + ch * 128u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // bit d = (score of document d >= thr), from the lowest plane up: threshold bit 1: &= plane, 0: |= plane
        uint32_t x = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < NP; ++k) x = ((thr >> k) & 1u) ? (x & pl[c][k]) : (x | pl[c][k]);
        if ((thr >> NP) != 0u) x = 0u;                      // no score reaches 2^NP
        const uint32_t vbw = vb > (uint32_t)c * 4u ? vb - (uint32_t)c * 4u : 0u;
        x &= low_bits(vbw * 8u);
        const uint32_t d0 = doc0 + (uint32_t)c * 32u;
        uint32_t nd = 0u;
        if (a.num_docs > d0) nd = a.num_docs - d0;
        x &= low_bits(nd);
        ge[c] = x;
        cnt += (uint32_t)__popc(x);
    }
    if (!__any(cnt != 0u)) return;                          // (uniform)
    uint64_t pos = pool_append(cnt, a.fill, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t x = ge[c];
        while (x != 0u) {
            const uint32_t d = (uint32_t)__ffs((int)x) - 1u;
            x &= x - 1u;
            uint32_t score = 0u;
#pragma unroll
            for (int k = 0; k < NP; ++k) score |= ((pl[c][k] >> d) & 1u) << k;
            if (pos < a.cap) a.pool[pos] = HitDev{q, a.file_no, doc0 + (uint32_t)c * 32u + d, score};
            ++pos;
        }
    }
}

int weighted_planes_for(uint64_t max_positions) {
    const uint64_t top = kMaxWeight * max_positions;        // the largest score
    for (int np : {8, 12, 14, 16, 20})
        if (top < (1ull << np)) return np;
    return 0;
}

uint32_t weighted_tile_w(uint32_t total_chunks) {
    uint32_t w = 1;
    while (w < total_chunks && w < 64u) w *= 2u;
    return w;
}

hipError_t launch_weights(const WeightArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (nq > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(weight_kernel, dim3(nq), dim3(256), 0, stream, a);
    return hipGetLastError();
}

namespace {

template <int NP>
void launch_np(const WeightedScanArgs& a, dim3 grid, hipStream_t stream) {
    dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1 && a.t.findere == 0, [&](auto idx, auto fast) {
        hipLaunchKernelGGL((weighted_scan_kernel<NP, decltype(idx), decltype(fast)::value>), grid, dim3(256), 0, stream, a);
    });
}

}  // namespace

hipError_t launch_weighted_scan(WeightedScanArgs a, int planes, hipStream_t stream) {
    if (a.nq == 0 || a.total_chunks == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || a.cpp != a.pitch / 16u || a.total_chunks % a.cpp != 0 || a.nq > 0x7FFFFFFFu ||
        a.tile_w == 0 || a.tile_w > 64u || (a.tile_w & (a.tile_w - 1u)) != 0 || a.t.num_hashes == 0 || a.t.findere > 7u)
        return hipErrorInvalidValue;
    const uint32_t ntiles = (a.total_chunks + a.tile_w - 1u) / a.tile_w;
    const uint32_t per_launch = std::max(1u, 0x7FFFFFFFu / a.nq);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += per_launch) {
        a.tile0 = t0;
        const dim3 grid(std::min(per_launch, ntiles - t0) * a.nq);
        switch (planes) {
            case 8: launch_np<8>(a, grid, stream); break;
            case 12: launch_np<12>(a, grid, stream); break;
            case 14: launch_np<14>(a, grid, stream); break;
            case 16: launch_np<16>(a, grid, stream); break;
            case 20: launch_np<20>(a, grid, stream); break;
            default: return hipErrorInvalidValue;
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cobs_amd
