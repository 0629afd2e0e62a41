// cobs_amd/csrc/window_kernels.hip -- gfx950 kernel of cobs_gpu_search_window: a document's score is the largest number
// of set positions in any window of w consecutive positions of the query (w = min(W, the query's positions)), where K2
// (kernels.hip) counts the set positions of the whole query.  wave64.
//
// window_scan_kernel.  The coverage scan's mapping (coverage_kernels.hip): a work-group owns one query and one tile of
// tile_w (a power of two, <= 64) sixteen-byte column chunks; a lane owns one chunk, 128 documents, as 4 column words; the
// 4 x 64 / tile_w lane groups share the query's positions by segments.  Per word the lane keeps
//   * NW planes of d = m - c >= 0, where c is the count of the window that ends at the position under the walk and m the
//     largest c so far.  With xi the presence word of position p and xo that of position p - w (0 while p - w lies before
//     the walk's start), c goes up where u = xi & ~xo and down where v = xo & ~xi, by one at the most.  Where c goes up
//     and d is 0 it sets a new record (rec: m grows, d stays 0); elsewhere d goes down (dec) or up (inc = v):
//         t = dec | inc;   per plane:  old = d_k;  d_k = old ^ t;  t &= old ^ dec
//     -- the carry of an increment goes on where old is 1, the borrow of a decrement where old is 0; both lines are
//     three-input booleans.  d <= m <= w < 2^NW: nothing overflows, nothing saturates.
//   * NW planes of m: the maximum is the number of records, so the eight rec words of a block of positions go through
//     the seven-CSA tree the coverage scan counts its covered bases with, the carry ripples into the planes above.
// NW is 6, 8, 10 or 12 by the call's W; it does not depend on the query's length.
// While the first window fills (fewer than w positions walked) the partial counts only grow, so none of them exceeds the
// first full window's count and none needs a mask.  At and beyond the end of the walk xi and xo are masked.
//
// Two row streams.  The rows of position p - w are gathered a second time through the row table (they left the
// registers w positions ago, and a ring of presence words in LDS would take 4 KiB x w); with H > 1 or z > 0 their AND
// is formed again.  An outgoing position that does not count reads the query's padding block (the zero row).
//
// Splitting a query.  A lane group takes the segment [s, e): it sets c = 0 at the 8-aligned block at or before
// s - (w - 1), with xo valid from w positions behind that block's first on, and walks to e.  Every count it forms is the
// count of a true stretch of at most w positions, so every record is <= the document's best, and every full window that
// ends in [s, e) is counted exactly: no count mask is needed.  A lane group that goes on to a further segment keeps m
// and starts it with d = m (c = 0), so m stays the largest count of all its segments.  The lane groups' m are merged
// with a bit-sliced MAX (shuffle butterfly inside a wave, LDS tree across the waves).
//
// No score leaves the registers: the epilogue compares the bit-sliced m with the query's threshold, masks everything
// that is no real document and appends the survivors to a pool as (query, file, document, best) with one atomic per wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "walk_ops.hpp"      // absorb8, word_of, load_row: the coverage scan's
#include "wave_ops.hpp"      // low_bits, pool_append, dispatch_idx_flag
#include "window_kernels.hpp"

namespace cobs_amd {

namespace {

// a <- max(a, b) per bit position, both NW planes: from the top plane down, gt = "a is larger", eq = "equal so far"
template <int NW>
__device__ __forceinline__ void max_planes(uint32_t* a, const uint32_t* b) {
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int k = NW - 1; k >= 0; --k) {
        gt |= eq & a[k] & ~b[k];
        eq &= ~(a[k] ^ b[k]);
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) a[k] = (gt & a[k]) | (~gt & b[k]);
}

}  // namespace

// H1: one hash function (the COBS default), no loop over the hashes
template <int NW, typename IdxT, bool H1>
__global__ __launch_bounds__(256) void window_scan_kernel(WindowScanArgs a) {
    __shared__ uint4 mbuf[2 * NW * 64];
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
    const uint32_t w = a.win[q];                                        // min(window, n) >= 1 (uniform)
    const uint32_t pad = tab.padding_block() * 8u;                      // a term of the zero row
    const uint32_t vw = wave * G + grp, NV = 4u * G;
    const uint32_t seg = a.seg ? a.seg : max(max(kWindowMinSeg, kWindowSegWindows * w), (n + NV - 1u) / NV);
    const uint32_t nseg = (n + seg - 1u) / seg;
    // the blocks of a segment with its pre-roll: from the 8-aligned block at or before s - (w - 1) to e
    const uint32_t JB = min((seg + w + 13u) >> 3, nb);
    // trips of this wave (uniform): as many as its first lane group needs; a lane group that has run out walks blocks
    // of the query with every mask empty
    const uint32_t first = wave * G;
    const uint32_t trips = nseg > first ? (nseg - first + NV - 1u) / NV : 0u;

    uint32_t m[4][NW];          // the record so far
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < NW; ++k) m[c][k] = 0u;

    for (uint32_t i = 0; i < trips; ++i) {
        const uint32_t sg = vw + i * NV;
        const bool has = sg < nseg;
        const uint32_t s = has ? sg * seg : n;
        const uint32_t e = has ? min(s + seg, n) : 0u;      // positions at and beyond e do not count (e <= n)
        const uint32_t b0 = (s >= w ? s - (w - 1u) : 0u) >> 3;
        const uint32_t o0 = b0 * 8u + w;                    // the first position whose outgoing one lies inside the walk
        uint32_t dl[4][NW];     // d = m - c with c = 0
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < NW; ++k) dl[c][k] = m[c][k];
        for (uint32_t j = 0; j < JB; ++j) {
            const uint32_t bu = b0 + j;                     // the block walked ...
            const uint32_t bl = min(bu, nb - 1u);           // ... and the one loaded: never beyond the query's blocks
            uint32_t im[8], om[8], po[8];   // position counts | its outgoing one counts | the term that one is read from
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) {
                const uint32_t p = bu * 8u + t;
                const bool in = p < e, out = in && p >= o0;
                im[t] = in ? 0xFFFFFFFFu : 0u;
                om[t] = out ? 0xFFFFFFFFu : 0u;
                po[t] = out ? p - w : pad;                  // p - w < n; pad + z <= pad + 7 stays inside the padding block
            }
            uint4 X[8], O[8];
            if (H1 && z == 0u) {                            // (uniform)
                const IdxT* idx = tab.block(bl);
#pragma unroll
                for (int t = 0; t < 8; ++t) X[t] = load_row(lane_base, (uint64_t)idx[t], pitch);
#pragma unroll
                for (int t = 0; t < 8; ++t) O[t] = load_row(lane_base, (uint64_t)tab.term(po[t])[0], pitch);
            } else {
#pragma unroll
                for (uint32_t t = 0; t < 8u; ++t) {
                    // terms p + s <= 8 nb - 1 + z <= T + 6 lie in the query's blocks or its padding block
                    const uint32_t p = bl * 8u + t;
                    uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u), aco = acc;
                    for (uint32_t f = 0; f <= z; ++f) {
                        const IdxT* en = tab.term(p + f);
                        const IdxT* eo = tab.term(po[t] + f);
                        for (uint32_t h = 0; h < H; ++h) {
                            const uint4 x = load_row(lane_base, (uint64_t)en[h * kRowTableLanes], pitch);
                            acc.x &= x.x; acc.y &= x.y; acc.z &= x.z; acc.w &= x.w;
                            const uint4 o = load_row(lane_base, (uint64_t)eo[h * kRowTableLanes], pitch);
                            aco.x &= o.x; aco.y &= o.y; aco.z &= o.z; aco.w &= o.w;
                        }
                    }
                    X[t] = acc;
                    O[t] = aco;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t rec[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const uint32_t xi = word_of(X[t], c) & im[t];
                    const uint32_t xo = word_of(O[t], c) & om[t];
                    const uint32_t u = xi & ~xo, v = xo & ~xi;
                    uint32_t nz = 0u;
#pragma unroll
                    for (int k = 0; k < NW; ++k) nz |= dl[c][k];
                    rec[t] = u & ~nz;
                    const uint32_t dec = u & nz;
                    uint32_t tt = dec | v;
#pragma unroll
                    for (int k = 0; k < NW; ++k) {
                        const uint32_t old = dl[c][k];
                        dl[c][k] = old ^ tt;                // (one v_bitop3_b32 each: the compiler forms them)
                        tt &= old ^ dec;
                    }
                }
                uint32_t k8 = absorb8(&m[c][0], rec);
#pragma unroll
                for (int k = 3; k < NW; ++k) {
                    const uint32_t t = m[c][k] & k8;
                    m[c][k] ^= k8;
                    k8 = t;
                }
            }
        }
    }

    // ---- merge the lane groups of a wave (butterfly: every lane group ends with the wave's maximum) ...
    for (uint32_t s = W; s < 64u; s <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t o[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) o[k] = (uint32_t)__shfl_xor((int)m[c][k], (int)s);
            max_planes<NW>(m[c], o);
        }
    }
    // ---- ... and the four waves (tree, bit-sliced maxima)
#pragma unroll
    for (int s = 1; s < 4; s <<= 1) {
        uint4* buf = mbuf + (size_t)(wave / (2 * s)) * NW * 64;
        if ((wave & (2 * s - 1)) == (uint32_t)s) {
#pragma unroll
            for (int k = 0; k < NW; ++k) buf[k * 64 + lane] = make_uint4(m[0][k], m[1][k], m[2][k], m[3][k]);
        }
        __syncthreads();
        if ((wave & (2 * s - 1)) == 0u) {
            uint32_t o[4][NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                const uint4 v = buf[k * 64 + lane];
                o[0][k] = v.x; o[1][k] = v.y; o[2][k] = v.z; o[3][k] = v.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) max_planes<NW>(m[c], o[c]);
        }
        __syncthreads();
    }
    if (wave != 0u) return;

    // ---- epilogue (wave 0, its first lane group: one lane per chunk of the tile): best >= threshold in bit-sliced
    // form, over real documents only -- row bytes inside the slice's valid width, documents below the file's count
    const uint32_t thr = a.thr[q];
    uint32_t ge[4];
    uint32_t cnt = 0u;
    const bool mine = live && grp == 0u;
    const uint32_t vb = (mine && pd.valid_bytes > ch * 16u) ? min(pd.valid_bytes - ch * 16u, 16u) : 0u;
    const uint32_t doc0 = pd.doc0 + ch * 128u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // bit d = (best of document d >= thr), from the lowest plane up: threshold bit 1: &= plane, 0: |= plane
        uint32_t x = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < NW; ++k) x = ((thr >> k) & 1u) ? (x & m[c][k]) : (x | m[c][k]);
        if ((thr >> NW) != 0u) x = 0u;                      // no count reaches 2^NW
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
            for (int k = 0; k < NW; ++k) score |= ((m[c][k] >> d) & 1u) << k;
            if (pos < a.cap) a.pool[pos] = HitDev{q, a.file_no, doc0 + (uint32_t)c * 32u + d, score};
            ++pos;
        }
    }
}

int window_planes_for(uint32_t window) {
    for (int nw : {6, 8, 10, 12})
        if (window < (1u << nw)) return nw;
    return 0;
}

namespace {

template <int NW>
void launch_nw(const WindowScanArgs& a, dim3 grid, hipStream_t stream) {
    dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
        hipLaunchKernelGGL((window_scan_kernel<NW, decltype(idx), decltype(h1)::value>), grid, dim3(256), 0, stream, a);
    });
}

}  // namespace

hipError_t launch_window_scan(WindowScanArgs a, hipStream_t stream) {
    if (a.nq == 0 || a.total_chunks == 0) return hipSuccess;
    const int planes = window_planes_for(a.window);
    if (a.pitch == 0 || a.pitch % 16u != 0 || a.cpp != a.pitch / 16u || a.total_chunks % a.cpp != 0 || a.nq > 0x7FFFFFFFu ||
        a.tile_w == 0 || a.tile_w > 64u || (a.tile_w & (a.tile_w - 1u)) != 0 || a.t.num_hashes == 0 || a.t.findere > 7u ||
        a.window == 0 || planes == 0 || a.seg >= (1u << 20))
        return hipErrorInvalidValue;
    const uint32_t ntiles = (a.total_chunks + a.tile_w - 1u) / a.tile_w;
    const uint32_t per_launch = std::max(1u, 0x7FFFFFFFu / a.nq);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += per_launch) {
        a.tile0 = t0;
        const dim3 grid(std::min(per_launch, ntiles - t0) * a.nq);
        switch (planes) {
            case 6: launch_nw<6>(a, grid, stream); break;
            case 8: launch_nw<8>(a, grid, stream); break;
            case 10: launch_nw<10>(a, grid, stream); break;
            case 12: launch_nw<12>(a, grid, stream); break;
            default: return hipErrorInvalidValue;
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cobs_amd
