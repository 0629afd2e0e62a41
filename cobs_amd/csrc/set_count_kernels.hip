// cobs_amd/csrc/set_count_kernels.hip -- gfx950 kernels of cobs_gpu_search_sets_quorum and cobs_gpu_set_prevalence: for every
// position of a query the number of members of every labelled SET that hold it, and the selection of the sets whose soft
// core reaches the threshold.  wave64.
//
// set_count_kernel.  The prevalence kernel's gather -- the same table access (RowTable, TableRef), the same AND over the
// H x (z + 1) rows of a position -- reduced over the columns of ONE set at a time.  The host inverts the segment records of
// the set search into RUNS (set_count_kernels.hpp): per (page, set with a member in that page) the 16-byte column chunks
// that hold members, with the members' mask.  A wave takes (query, run, group of positions).  With lx = the next power of
// two of the run's records (at most 64) its lanes sit lx side by side along the run's records and ly = 64 / lx positions
// side by side: a one-member set keeps all 64 lanes busy on 64 positions, a set of 8 192 consecutive documents puts 64 lanes
// on 64 neighbouring column chunks of one row, and its loads are contiguous.  Runs longer than 64 records loop with
// stride 64.  Per position a lane sums popc(acc & mask) over its records, the lx lanes add up in DPP steps of the VALU
// (group_sum_last, as in the prevalence kernel), and ONE lane adds the sum to the cell: one global atomic per
// (run, position) = (set, page, position), however many column chunks the set covers.  A wave walks two groups of
// positions at a time, the loads of both in flight at once.  The grid is (queries, slabs of position groups, runs).
//
// A labelling that follows the document order gives few runs per page and long ones; a chunk shared by two sets is read
// by both.  A labelling that scatters every set over every chunk (128 sets per chunk) reads every column chunk once per set
// in it: exact, and up to 128 times the loads.
//
// The masks hold members only, so nothing else is masked here, and a record's column chunk lies below pitch / 16 by
// construction.  Positions at or beyond n = T - z are never touched: their lanes load nothing and add nothing, and since
// p + z < T for every p < n no term at or beyond T is looked up.
//
// set_quorum_select_kernel.  One work item per (query, non-empty set of a labelled file): a walk over its n cells, core =
// the cells >= need(set) (computed on the host), any = the cells > 0, the threshold max(1, ceil(threshold * P)) in double on
// core, and a 16-byte record appended through the hit pool's append.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "set_count_kernels.hpp"
#include "wave_ops.hpp"                // group_sum_last, pool_append, dispatch_idx_flag

namespace cobs_amd {

// H1: one hash function (the COBS default), no loop over the hashes
template <typename IdxT, bool H1>
__global__ __launch_bounds__(256) void set_count_kernel(SetCountArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x;
    const SetRun run = a.runs[a.run0 + blockIdx.z];
    const PageDev pd = a.pages[run.page];
    const uint32_t z = a.t.findere;
    const uint32_t n = a.t.q_len[q] - a.t.term_size + 1u - z;   // the host made sure T > z
    const uint32_t H = H1 ? 1u : a.t.num_hashes;
    const RowTable<IdxT> tab(a.t, q, pd.tpage, H);
    const uint8_t* __restrict__ rows = a.data + pd.base;
    uint32_t* __restrict__ out = a.cells + a.cell_off[(uint64_t)q * a.cell_stride] + (uint64_t)run.set * n;
    uint32_t lx = 1u;                                            // (uniform per wave: the run is the work-group's)
    while (lx < run.nrec && lx < 64u) lx *= 2u;
    const uint32_t ly = 64u / lx;
    const uint32_t cx = lane & (lx - 1u), py = lane / lx;
    const uint32_t groups = (n + ly - 1u) / ly;
    const uint32_t nw = gridDim.y * 4u;
    const uint32_t rec1 = run.rec0 + run.nrec;

    // members among the 128 slots of `mask` at column chunk `col` that hold position p
    auto count = [&](uint32_t p, uint32_t col_chunk, const uint4& mask) -> uint32_t {
        uint4 acc = mask;
        const uint8_t* col = rows + (uint64_t)col_chunk * 16u;
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
        return __popc(acc.x) + __popc(acc.y) + __popc(acc.z) + __popc(acc.w);
    };

    for (uint32_t g = blockIdx.y * 4u + wave; g < groups; g += 2u * nw) {      // (uniform per wave)
        const uint32_t p0 = g * ly + py, p1 = p0 + nw * ly;
        const bool in0 = p0 < n, in1 = (uint64_t)g + nw < groups && p1 < n;    // (the last group may be partly filled)
        uint32_t c0 = 0u, c1 = 0u;
        for (uint32_t r = run.rec0 + cx; r < rec1; r += lx) {
            const uint32_t col_chunk = a.rec_col[r];
            const uint4 mask = a.rec_mask[r];
            if (in0) c0 += count(p0, col_chunk, mask);
            if (in1) c1 += count(p1, col_chunk, mask);
        }
        c0 = group_sum_last(c0, lx);
        c1 = group_sum_last(c1, lx);
        if (cx == lx - 1u) {
            if (in0 && c0 != 0u) atomicAdd(out + p0, c0);
            if (in1 && c1 != 0u) atomicAdd(out + p1, c1);
        }
    }
}

__global__ __launch_bounds__(256) void set_quorum_select_kernel(SetQuorumSelectArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    SetQuorumRec rec{0u, 0u, 0u, 0u};
    if (t < (uint64_t)a.nq * a.nitems) {
        const uint32_t q = (uint32_t)(t / a.nitems), it = (uint32_t)(t % a.nitems);
        const SetQuorumItem item = a.items[it];
        const uint32_t n = a.q_len[q] - item.term_size + 1u - a.findere;
        const uint32_t* __restrict__ c = a.cells + a.cell_off[(uint64_t)q * a.nfiles + item.file_no] + (uint64_t)item.local * n;
        uint32_t core = 0u, held = 0u;
        for (uint32_t p = 0; p < n; ++p) {
            const uint32_t v = c[p];
            core += v >= item.need ? 1u : 0u;
            held += v != 0u ? 1u : 0u;
        }
        rec = SetQuorumRec{q, it, core, held};
        if (a.threshold > 0.0) {
            // P: the denominator the search uses for (query, file); a (query, file) with P = 0 returns nothing
            const uint32_t P = item.use_valid != 0u ? a.valid[(uint64_t)item.file_no * a.nq + q] : n;
            const double v = ceil(a.threshold * (double)P);
            const uint32_t thr = !(v > 1.0) ? 1u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
            hit = P != 0u && core >= thr;
        } else {
            hit = true;
        }
    }
    // (every lane of every wave arrives here)
    const unsigned long long pos = pool_append(hit ? 1u : 0u, a.fill, lane);
    if (hit && pos < a.cap) a.pool[pos] = rec;
}

hipError_t launch_set_count(SetCountArgs a, size_t n_runs, uint32_t max_recs, uint32_t nq, uint32_t max_positions,
                            hipStream_t stream) {
    if (n_runs == 0 || nq == 0 || max_positions == 0) return hipSuccess;
    if (a.pitch == 0 || a.pitch % 16u != 0 || max_recs == 0 || nq > 0x7FFFFFFFu || n_runs > 0xFFFFFFF0ull) return hipErrorInvalidValue;
    // the narrowest ly of the chunk's runs sizes the slabs: four waves per work-group, two position groups per wave and
    // trip, up to four trips per wave, then more slabs (a run with fewer groups leaves its last slabs without work)
    uint32_t lx = 1;
    while (lx < max_recs && lx < 64u) lx *= 2u;
    const uint32_t ly = 64u / lx;
    const uint32_t groups = (max_positions + ly - 1u) / ly;
    const uint32_t gy = std::min(1024u, (groups + 31u) / 32u);
    constexpr size_t kMaxGridZ = 65535;
    for (size_t r0 = 0; r0 < n_runs; r0 += kMaxGridZ) {
        a.run0 = (uint32_t)r0;
        const dim3 grid(nq, gy, (uint32_t)std::min(kMaxGridZ, n_runs - r0)), block(256);
        dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
            hipLaunchKernelGGL((set_count_kernel<decltype(idx), decltype(h1)::value>), grid, block, 0, stream, a);
        });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_set_quorum_select(const SetQuorumSelectArgs& a, hipStream_t stream) {
    const uint64_t items = (uint64_t)a.nq * a.nitems;
    if (items == 0) return hipSuccess;
    const uint64_t blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_quorum_select_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
