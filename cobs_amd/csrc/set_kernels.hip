// cobs_amd/csrc/set_kernels.hip -- gfx950 kernels of cobs_gpu_search_sets: for every labelled SET of documents the
// positions of a query that at least one member holds (`any`) and that some member lacks (`miss`; all = n - miss), as
// bit matrices, and the selection of the sets whose count reaches the threshold.  wave64.
//
// set_presence_kernel.  The prevalence kernel's gather -- the same table access (RowTable, TableRef), the same AND over the
// H x (z + 1) rows of a position -- reduced over labelled subsets of the columns instead of over all of them.  A lane
// owns one 16-byte column chunk (128 documents) and a BLOCK of 32 consecutive positions: one word of a set's bitmap.
// The lx lanes of a block sit side by side along the row, so every load instruction of a wave is contiguous; where a
// row has fewer than 64 chunks the remaining lanes take further blocks (ly = 64 / lx side by side).  Rows wider than 64
// chunks loop with stride 64.  The grid is (queries, slabs of position blocks, pages of the chunk).
//
// The distinct sets among the 128 slots of a column chunk come from the host as segment records (set, 128-bit mask), CSR
// over (page, column chunk) -- sets.cpp builds them once per labelling.  The masks hold members only: no padding slot,
// no slot at or beyond the file's last document, no unlabelled document; nothing else is masked here.  Per record the
// lane assembles two words over its 32 positions, any: (acc & mask) != 0, miss: (acc & mask) != mask, and issues at most
// one atomicOr per non-zero word.  kSetBatch records are held at a time, in registers with fixed indexing; a chunk with
// more records walks its rows again per batch (from cache).  Positions at or beyond n = T - z are never touched: their
// bits stay 0 in both matrices, and since p + z < T for every p < n no term at or beyond T is looked up.
//
// Meant for labellings that follow the document order (a collection sorted by name: 1-2 records per chunk, one batch).
// A labelling that scatters every set over every chunk (up to 128 records) is correct and 128 / kSetBatch times the work.
//
// set_select_kernel.  One work item per (query, non-empty set of a labelled file): popcounts of its words, the threshold
// max(1, ceil(threshold * P)) in double on the key, and a 16-byte record appended through the hit pool's append.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "prevalence_kernels.hpp"      // prevalence_lx: the same lanes-along-the-row rule
#include "set_kernels.hpp"
#include "wave_ops.hpp"                // pool_append, dispatch_idx_flag

namespace cobs_amd {

// H1: one hash function (the COBS default), no loop over the hashes
template <typename IdxT, bool H1>
__global__ __launch_bounds__(256) void set_presence_kernel(SetPresenceArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x;
    const uint32_t page = a.page0 + blockIdx.z;
    const PageDev pd = a.pages[page];
    // (an early return, as in the prevalence kernel: a slice of padding documents only has no records either)
    if (a.num_docs <= pd.doc0 || pd.valid_bytes == 0u) return;
    const uint32_t live = min(a.num_docs - pd.doc0, pd.valid_bytes * 8u);
    const uint32_t z = a.t.findere;
    const uint32_t n = a.t.q_len[q] - a.t.term_size + 1u - z;   // the host made sure T > z
    const uint32_t W = (n + 31u) >> 5;                           // words per set
    const uint32_t H = H1 ? 1u : a.t.num_hashes;
    const RowTable<IdxT> tab(a.t, q, pd.tpage, H);
    const uint8_t* __restrict__ rows = a.data + pd.base;
    const uint64_t bm = a.bm_off[(uint64_t)q * a.bm_stride];
    uint32_t* __restrict__ any = a.any + bm;
    uint32_t* __restrict__ miss = a.miss + bm;
    const uint32_t* __restrict__ first = a.seg_first + (uint64_t)page * a.cpp;
    const uint32_t lx = a.lx, ly = a.ly;
    const uint32_t cx = lane & (lx - 1u), py = lane / lx;
    const uint32_t groups = (W + ly - 1u) / ly;
    const uint32_t nw = gridDim.y * 4u;

    for (uint32_t g = blockIdx.y * 4u + wave; g < groups; g += nw) {      // (uniform per wave)
        const uint32_t pb = g * ly + py;                  // the lane's block of positions = its word of a bitmap
        if (pb >= W) continue;                            // (the last group may be partly filled; no cross-lane step below)
        const uint32_t p0 = pb * 32u, np = min(32u, n - p0);
        for (uint32_t chunk = cx; chunk * 128u < live; chunk += lx) {
            const uint32_t r0 = first[chunk], r1 = first[chunk + 1u];
            const uint8_t* col = rows + (uint64_t)chunk * 16u;
            for (uint32_t r = r0; r < r1; r += kSetBatch) {
                uint4 m[kSetBatch];
                uint32_t av[kSetBatch], mv[kSetBatch];
#pragma unroll
                for (uint32_t k = 0; k < kSetBatch; ++k) {
                    m[k] = r + k < r1 ? a.seg_mask[r + k] : make_uint4(0u, 0u, 0u, 0u);   // (an empty mask raises no bit)
                    av[k] = 0u;
                    mv[k] = 0u;
                }
#pragma unroll 2
                for (uint32_t i = 0; i < np; ++i) {
                    uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u);
                    for (uint32_t s = 0; s <= z; ++s) {
                        const IdxT* e = tab.term(p0 + i + s);
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
#pragma unroll
                    for (uint32_t k = 0; k < kSetBatch; ++k) {
                        const uint32_t tx = acc.x & m[k].x, ty = acc.y & m[k].y, tz = acc.z & m[k].z, tw = acc.w & m[k].w;
                        const uint32_t held = (tx | ty | tz | tw) != 0u ? 1u : 0u;
                        const uint32_t lack = ((tx ^ m[k].x) | (ty ^ m[k].y) | (tz ^ m[k].z) | (tw ^ m[k].w)) != 0u ? 1u : 0u;
                        av[k] |= held << i;
                        mv[k] |= lack << i;
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < kSetBatch; ++k) {
                    if (r + k < r1) {
                        const uint64_t w = (uint64_t)a.seg_set[r + k] * W + pb;
                        if (av[k] != 0u) atomicOr(any + w, av[k]);
                        if (mv[k] != 0u) atomicOr(miss + w, mv[k]);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void set_select_kernel(SetSelectArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    SetRec rec{0u, 0u, 0u, 0u};
    if (t < (uint64_t)a.nq * a.nitems) {
        const uint32_t q = (uint32_t)(t / a.nitems), it = (uint32_t)(t % a.nitems);
        const SetItem item = a.items[it];
        const uint32_t n = a.q_len[q] - item.term_size + 1u - a.findere;
        const uint32_t W = (n + 31u) >> 5;
        const uint64_t w0 = a.bm_off[(uint64_t)q * a.nfiles + item.file_no] + (uint64_t)item.local * W;
        uint32_t held = 0u, lack = 0u;
        for (uint32_t w = 0; w < W; ++w) {
            held += __popc(a.any[w0 + w]);
            lack += __popc(a.miss[w0 + w]);
        }
        rec = SetRec{q, it, held, n - lack};
        if (a.threshold > 0.0) {
            // P: the denominator the search uses for (query, file); a (query, file) with P = 0 returns nothing
            const uint32_t P = item.use_valid != 0u ? a.valid[(uint64_t)item.file_no * a.nq + q] : n;
            const double v = ceil(a.threshold * (double)P);
            const uint32_t thr = !(v > 1.0) ? 1u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
            hit = P != 0u && (a.rank_by != 0u ? rec.all : rec.any) >= thr;
        } else {
            hit = true;
        }
    }
    // (every lane of every wave arrives here)
    const unsigned long long pos = pool_append(hit ? 1u : 0u, a.fill, lane);
    if (hit && pos < a.cap) a.pool[pos] = rec;
}

hipError_t launch_set_presence(SetPresenceArgs a, const std::vector<PageDev>& pages, uint32_t nq, uint32_t max_positions,
                               hipStream_t stream) {
    if (pages.empty() || nq == 0 || max_positions == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || a.cpp != a.pitch / 16u || nq > 0x7FFFFFFFu) return hipErrorInvalidValue;
    uint32_t valid = 0;
    for (const PageDev& pd : pages) {
        if (pd.valid_bytes > a.pitch) return hipErrorInvalidValue;
        valid = std::max(valid, pd.valid_bytes);
    }
    a.lx = prevalence_lx(valid);
    a.ly = 64u / a.lx;
    // four waves per work-group, one group of position blocks per wave and trip
    const uint32_t blocks = (max_positions + 31u) / 32u;
    const uint32_t groups = (blocks + a.ly - 1u) / a.ly;
    const uint32_t gy = std::min(1024u, (groups + 3u) / 4u);
    constexpr size_t kMaxGridZ = 65535;
    for (size_t p0 = 0; p0 < pages.size(); p0 += kMaxGridZ) {
        a.page0 = (uint32_t)p0;
        const dim3 grid(nq, gy, (uint32_t)std::min(kMaxGridZ, pages.size() - p0)), block(256);
        dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
            hipLaunchKernelGGL((set_presence_kernel<decltype(idx), decltype(h1)::value>), grid, block, 0, stream, a);
        });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_set_select(const SetSelectArgs& a, hipStream_t stream) {
    const uint64_t items = (uint64_t)a.nq * a.nitems;
    if (items == 0) return hipSuccess;
    const uint64_t blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_select_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
