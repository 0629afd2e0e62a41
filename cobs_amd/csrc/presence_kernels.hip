// cobs_amd/csrc/presence_kernels.hip -- gfx950 kernel of cobs_gpu_hit_positions: for a (query, document) pair the one
// bit of every row the query looks up, along the query.
//
// lane = term.  A wave takes 64 consecutive terms of one pair: every lane reads its H row indices from K1's table,
// loads the byte of the document's column in each of those rows, ANDs them and tests the document's bit; the ballot of
// that predicate IS the 64-bit output word.  With findere z > 0 a position needs terms p .. p + z: the word is ANDed
// with itself shifted by 1 .. z, the top z bits coming from the first z terms of the next 64 (a second ballot in which
// only z lanes load).  Terms >= T read as absent without a load, so bits >= T - z of the last word are zero.
//
// Bound: latency of two dependent loads per (term, hash) -- table entry, then one byte of a random row: one 64-byte
// sector moved for one useful bit.  Nothing is reused inside a wave; pairs of neighbouring documents hit the same
// sectors through L2.
#include <hip/hip_runtime.h>

#include "presence_kernels.hpp"
#include "wave_ops.hpp"      // dispatch_idx_flag

namespace cobs_amd {

// H1: one hash function (the COBS default), no loop over the hashes
template <typename IdxT, bool H1>
__global__ __launch_bounds__(256) void presence_kernel(PresenceArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const PresencePair pr = a.pairs[blockIdx.x];          // grid.x == npairs
    const uint32_t q = pr.query;
    const uint32_t T = a.t.q_len[q] - a.t.term_size + 1u;
    const uint32_t z = a.t.findere;
    const uint32_t nwords = (T - z + 63u) >> 6;            // the host made sure T > z
    const uint32_t H = H1 ? 1u : a.t.num_hashes;
    const RowTable<IdxT> tab(a.t, q, pr.tpage, H);

    auto present = [&](uint32_t t) -> bool {
        if (t >= T) return false;
        const IdxT* e = tab.term(t);
        uint32_t acc = 0xFFu;
        if (H1) {
            acc = pr.col[(uint64_t)e[0] * pr.pitch];
        } else {
#pragma unroll 4
            for (uint32_t j = 0; j < H; ++j) acc &= pr.col[(uint64_t)e[j * kRowTableLanes] * pr.pitch];
        }
        return ((acc >> pr.bit) & 1u) != 0u;
    };

    for (uint32_t w = blockIdx.y * 4u + wave; w < nwords; w += gridDim.y * 4u) {      // (uniform per wave)
        const uint32_t t0 = w * 64u;
        const uint64_t cur = __ballot(present(t0 + lane));
        uint64_t word = cur;
        if (z != 0u) {
            const uint64_t nxt = __ballot(lane < z && present(t0 + 64u + lane));
            for (uint32_t s = 1; s <= z; ++s) word &= (cur >> s) | (nxt << (64u - s));
        }
        if (lane == 0u) a.bits[pr.out + w] = word;
    }
}

hipError_t launch_presence(const PresenceArgs& a, uint32_t max_words, hipStream_t stream) {
    if (a.npairs == 0) return hipSuccess;
    // four words per work-group and trip; long queries spread over grid.y, at most four trips per wave up to 4096 words
    const uint32_t gy = max_words <= 16u ? 1u : (max_words + 15u) / 16u > 256u ? 256u : (max_words + 15u) / 16u;
    const dim3 grid(a.npairs, gy), block(256);
    dispatch_idx_flag(a.t.idx64 != 0, a.t.num_hashes == 1, [&](auto idx, auto h1) {
        hipLaunchKernelGGL((presence_kernel<decltype(idx), decltype(h1)::value>), grid, block, 0, stream, a);
    });
    return hipGetLastError();
}

}  // namespace cobs_amd
