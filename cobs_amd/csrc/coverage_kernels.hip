// cobs_amd/csrc/coverage_kernels.hip -- gfx950 kernel of cobs_gpu_search_coverage: a document's score is the number of
// QUERY BASES that lie inside a set position (span = k + z bases from the position on), where K2 (kernels.hip) counts the
// positions themselves.  wave64.
//
// coverage_scan_kernel.  The weighted scan's mapping: a work-group owns one query and one tile of W (a power of two,
// <= 64) sixteen-byte column chunks; a lane owns one chunk, 128 documents, as 4 column words.  Per word the lane keeps
//   * a countdown c: at position p with presence word x, c <- span where x is set, else max(c - 1, 0); y = (c != 0)
//     says "base p is covered".  It is held as the live plane y and NC planes (NC = 5, 6 or 8 >= bit_width(span - 1))
//     of e = c - 1, each stored XORed with the constant bit of span - 1: "set" is then "all planes 0", whatever span is,
//     and a plane's update is ONE three-input boolean, e'_k <- ~x & (e'_k ^ borrow).  The borrow goes on as
//     borrow & ~(e'_k ^ bit_k(span - 1)), a second three-input boolean whose third operand is a scalar mask (span is
//     uniform per launch; nothing steers control flow).  A borrow that leaves the top plane found e = 0, i.e. c = 1:
//     y <- x | (y & ~borrow), so the counter saturates at 0 without a compare.  2 NC + 3 boolean ops per word and
//     position (v_bitop3_b32 / AND), 13 at span 31.
//   * NP count planes (8, 12, 16, 20 by the longest query of the pass): the eight y words of a block of positions go
//     through the seven-CSA tree the weighted scan and K2 use, the carry ripples into the planes above.
// The bases behind the last position, n .. n + span - 2, are covered while the countdown lasts: max(c - 1, 0) = e of
// them where y is set, ONE bit-sliced add of the NC planes into the count planes, not span - 1 further steps.
//
// Splitting a query.  The positions of a document have to be walked in order, but the state at position s depends only
// on the positions s - (span - 1) .. s - 1.  So the query's n positions are cut into segments of `seg` positions, dealt
// round-robin over the 4 x 64 / W lane groups; a lane group starts a segment [s, e) with c = 0 at the 8-aligned block
// at or before s - (span - 1), walks to e and counts only the y of [s, e) (a mask that is uniform per lane group, not a
// branch).  Beyond n the countdown is held (borrow and x masked), so after the walk the lane group of the segment that
// ends at n still has e of position n - 1 and adds the tail.  The partial counts are merged as in the weighted scan
// (shuffle butterfly inside a wave, LDS tree across the waves); the sum is at most the query's length.
//
// Rows: H = 1, z = 0: one 16-byte load per position; otherwise the AND of the H x (z + 1) rows of the position, as the
// prevalence kernel forms it.  No score leaves the registers: the epilogue compares the bit-sliced counts with the
// query's threshold, masks everything that is no real document and appends the survivors to a pool as (query, file,
// document, covered bases) with one atomic per wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coverage_kernels.hpp"
#include "walk_ops.hpp"      // absorb8, word_of, load_row: shared with the window scan
#include "wave_ops.hpp"      // csa, low_bits, pool_append, dispatch_idx_flag

namespace cobs_amd {

// H1: one hash function (the COBS default), no loop over the hashes
template <int NP, int NC, typename IdxT, bool H1>
__global__ __launch_bounds__(256) void coverage_scan_kernel(CoverageScanArgs a) {
    static_assert(NC <= NP, "the tail adds the countdown planes into the count planes");
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
    const uint32_t H = H1 ? 1u : a.t.num_hashes, z = a.t.findere;
    const RowTable<IdxT> tab(a.t, q, pd.tpage, H);
    const uint32_t n = a.t.q_len[q] - a.t.term_size + 1u - z;          // the host made sure n >= 1
    const uint32_t nb = (n + 7u) >> 3;                                  // blocks of positions (<= tab.nblk)
    const uint32_t span = a.span;
    const uint32_t vw = wave * G + grp, NV = 4u * G;
    const uint32_t seg = a.seg ? a.seg : max(kCoverageMinSeg, (n + NV - 1u) / NV);
    const uint32_t nseg = (n + seg - 1u) / seg;
    // the blocks of a segment with its pre-roll: from the 8-aligned block at or before s - (span - 1) to e
    const uint32_t JB = min((seg + span + 13u) >> 3, nb);
    // trips of this wave (uniform): as many as its first lane group needs; a lane group that has run out walks blocks
    // of the query with every mask empty
    const uint32_t first = wave * G;
    const uint32_t trips = nseg > first ? (nseg - first + NV - 1u) / NV : 0u;

    uint32_t sm[NC];            // all ones where bit k of span - 1 is set (uniform)
#pragma unroll
    for (int k = 0; k < NC; ++k) sm[k] = 0u - (((span - 1u) >> k) & 1u);

    uint32_t pl[4][NP];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[c][k] = 0u;

    for (uint32_t i = 0; i < trips; ++i) {
        const uint32_t sg = vw + i * NV;
        const bool has = sg < nseg;
        const uint32_t s = has ? sg * seg : n;
        const uint32_t e = min(s + seg, n);
        const uint32_t b0 = (s >= span ? s - (span - 1u) : 0u) >> 3;
        uint32_t cd[4][NC], y[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            y[c] = 0u;
#pragma unroll
            for (int k = 0; k < NC; ++k) cd[c][k] = 0u;
        }
        for (uint32_t j = 0; j < JB; ++j) {
            const uint32_t bu = b0 + j;                     // the block walked ...
            const uint32_t bl = min(bu, nb - 1u);           // ... and the one loaded: never beyond the query's blocks
            uint4 X[8];
            if (H1 && z == 0u) {                            // (uniform)
                const IdxT* idx = tab.block(bl);
#pragma unroll
                for (int t = 0; t < 8; ++t) X[t] = load_row(lane_base, (uint64_t)idx[t], pitch);
            } else {
#pragma unroll
                for (uint32_t t = 0; t < 8u; ++t) {
                    // terms p + s <= 8 nb - 1 + z <= T + 6 lie in the query's blocks or its padding block
                    const uint32_t p = bl * 8u + t;
                    uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u);
                    for (uint32_t w = 0; w <= z; ++w) {
                        const IdxT* en = tab.term(p + w);
                        for (uint32_t h = 0; h < H; ++h) {
                            const uint4 x = load_row(lane_base, (uint64_t)en[h * kRowTableLanes], pitch);
                            acc.x &= x.x; acc.y &= x.y; acc.z &= x.z; acc.w &= x.w;
                        }
                    }
                    X[t] = acc;
                }
            }
            uint32_t pm[8], cm[8];      // position below n | position inside [s, e): uniform per lane group
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) {
                const uint32_t p = bu * 8u + t;
                pm[t] = p < n ? 0xFFFFFFFFu : 0u;
                cm[t] = (p >= s && p < e) ? 0xFFFFFFFFu : 0u;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t yc[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const uint32_t x = word_of(X[t], c) & pm[t];
                    uint32_t b = pm[t];                     // borrow in: 1; beyond n the countdown is held
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const uint32_t old = cd[c][k];
                        cd[c][k] = ~x & (old ^ b);          // (one v_bitop3_b32 each: the compiler forms them)
                        b = b & ~(old ^ sm[k]);
                    }
                    y[c] = x | (y[c] & ~b);
                    yc[t] = y[c] & cm[t];
                }
                uint32_t k8 = absorb8(&pl[c][0], yc);
#pragma unroll
                for (int k = 3; k < NP; ++k) {
                    const uint32_t t = pl[c][k] & k8;
                    pl[c][k] ^= k8;
                    k8 = t;
                }
            }
        }
        // the bases behind the last position: e = c - 1 where y is set, added by the lane group whose segment ends at n
        const uint32_t tm = (has && s + seg >= n) ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t nz = y[c] & tm;
            uint32_t carry = 0u;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const uint32_t d = (cd[c][k] ^ sm[k]) & nz;
                uint32_t h;
                csa(h, pl[c][k], pl[c][k], d, carry);
                carry = h;
            }
#pragma unroll
            for (int k = NC; k < NP; ++k) {
                const uint32_t t = pl[c][k] & carry;
                pl[c][k] ^= carry;
                carry = t;
            }
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

    // ---- epilogue (wave 0, its first lane group: one lane per chunk of the tile): coverage >= threshold in bit-sliced
    // form, over real documents only -- row bytes inside the slice's valid width, documents below the file's count
    const uint32_t thr = a.thr[q];
    uint32_t ge[4];
    uint32_t cnt = 0u;
    const bool mine = live && grp == 0u;
    const uint32_t vb = (mine && pd.valid_bytes > ch * 16u) ? min(pd.valid_bytes - ch * 16u, 16u) : 0u;
    const uint32_t doc0 = pd.doc0 + ch * 128u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // bit d = (coverage of document d >= thr), from the lowest plane up: threshold bit 1: &= plane, 0: |= plane
        uint32_t x = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < NP; ++k) x = ((thr >> k) & 1u) ? (x & pl[c][k]) : (x | pl[c][k]);
        if ((thr >> NP) != 0u) x = 0u;                      // no coverage reaches 2^NP
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

int coverage_planes_for(uint64_t max_len) {
    for (int np : {8, 12, 16, 20})
        if (max_len < (1ull << np)) return np;
    return 0;
}

uint32_t coverage_tile_w(uint32_t total_chunks) {
    uint32_t w = 1;
    while (w < total_chunks && w < 64u) w *= 2u;
    return w;
}

namespace {

template <int NP, int NC>
void launch_np_nc(const CoverageScanArgs& a, dim3 grid, hipStream_t stream) {
    dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
        hipLaunchKernelGGL((coverage_scan_kernel<NP, NC, decltype(idx), decltype(h1)::value>), grid, dim3(256), 0, stream, a);
    });
}

template <int NP>
void launch_np(const CoverageScanArgs& a, dim3 grid, hipStream_t stream) {
    // countdown planes: bit_width(span) rounded up to an instantiation
    if (a.span < 32u) launch_np_nc<NP, 5>(a, grid, stream);
    else if (a.span < 64u) launch_np_nc<NP, 6>(a, grid, stream);
    else launch_np_nc<NP, 8>(a, grid, stream);
}

}  // namespace

hipError_t launch_coverage_scan(CoverageScanArgs a, int planes, hipStream_t stream) {
    if (a.nq == 0 || a.total_chunks == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || a.cpp != a.pitch / 16u || a.total_chunks % a.cpp != 0 || a.nq > 0x7FFFFFFFu ||
        a.tile_w == 0 || a.tile_w > 64u || (a.tile_w & (a.tile_w - 1u)) != 0 || a.t.num_hashes == 0 || a.t.findere > 7u ||
        a.span == 0 || a.span > kCoverageMaxSpan || a.span != a.t.term_size + a.t.findere || a.seg >= kCoverageMaxLen)
        return hipErrorInvalidValue;
    const uint32_t ntiles = (a.total_chunks + a.tile_w - 1u) / a.tile_w;
    const uint32_t per_launch = std::max(1u, 0x7FFFFFFFu / a.nq);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += per_launch) {
        a.tile0 = t0;
        const dim3 grid(std::min(per_launch, ntiles - t0) * a.nq);
        switch (planes) {
            case 8: launch_np<8>(a, grid, stream); break;
            case 12: launch_np<12>(a, grid, stream); break;
            case 16: launch_np<16>(a, grid, stream); break;
            case 20: launch_np<20>(a, grid, stream); break;
            default: return hipErrorInvalidValue;
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cobs_amd
