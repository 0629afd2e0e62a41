// cobs_amd/csrc/hash_kernels.hip -- K1 of the COBS query path (gfx950, wave64): canonicalise + XXH64 + (hash % S_p)
// per sub-index, one thread per query position, written into the row-index table K2 reads (row_table.hpp)
//   (create_hashes, reference classic_search.cpp:66-107; canonicalize_kmer, util/query.cpp:143-199; modulo at
//    classic_index/mmap_search_file.cpp:35 and compact_index/mmap_search_file.cpp:58)
// and the thresholds of invalid_bases = skip from K1's valid positions.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "kernels.hpp"
#include "row_table.hpp"     // K1's row-index table: the writer below
#include "term_hash.hpp"     // rotl64 .. xxh64_view, comp4 / xxh64_31 / canon31, all_acgt
#include "wave_ops.hpp"

namespace cobs_amd {

// ---------------------------------------------------------------------------
// K1: one thread per query position (canonicalisation and XXH64: term_hash.hpp).

// invalid_bases != 0.  The z characters behind term i's k-mer (`tail`): position i < T - z scores the terms i .. i + z, so it
// is valid when they hold valid characters too (findere; z = 0: nothing to look at).
__device__ __forceinline__ bool window_tail_valid(const uint8_t* tail, uint32_t i, uint32_t T, uint32_t z) {
    if (i + z >= T) return false;               // no window of z + 1 terms starts here: not a scored position
    uint32_t good = 1u;
    for (uint32_t s = 0; s < z; ++s) good &= fwd_base(tail[s]) != 0 ? 1u : 0u;
    return good != 0;
}

// valid[q] += the lanes of this wave that hold a valid position of query q.  A thread per position of 10 000 reads would be
// ten million atomics onto ten thousand addresses: the lanes of a wave that share a query (a query's span is a multiple of
// 8 threads, so a wave sees at most eight) are counted by a ballot first, and one lane adds the sum.  Called by every lane
// that is still active, with converged control flow.
__device__ __forceinline__ void add_valid_position(uint32_t* valid, uint32_t q, bool ok) {
    const uint32_t lane = __lane_id();
    bool pending = true;
    for (;;) {
        const uint64_t waiting = __ballot(pending);
        if (waiting == 0) break;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)waiting) - 1u;
        const uint32_t lq = (uint32_t)__shfl((int)q, (int)leader);
        const bool mine = pending && q == lq;
        const uint64_t votes = __ballot(mine && ok);
        if (mine) pending = false;
        if (lane == leader && votes != 0) atomicAdd(valid + lq, (uint32_t)__popcll(votes));
    }
}

// invalid_bases = skip: the thresholds of one file from K1's valid positions, ceil(threshold * V) in double as the host's
// threshold_for computes it -- and at least 1: a query without a valid position matches nothing, not everything.  A
// threshold that is not > 0 (a NaN too) asks for every document, as threshold_of says on the host: 0.
__global__ __launch_bounds__(256) void skip_thresholds_kernel(SkipThresholdArgs a) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nq) return;
    const double v = ceil(a.threshold * (double)a.valid[q]);
    a.thresholds[q] = !(a.threshold > 0.0) ? 0u : !(v >= 1.0) ? 1u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

template <typename IdxT>
__global__ __launch_bounds__(256) void hash_kernel(HashArgs a, uint64_t total_threads) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the grid may be larger than the batch needs (a captured launch is replayed for other query lengths)
    if (gid >= total_threads || gid >= a.span_off[a.nq]) return;
    // query of this thread: last q with span_off[q] <= gid
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (a.span_off[mid] <= gid) lo = mid; else hi = mid;
    }
    const uint32_t q = lo;
    const uint64_t qbase = a.span_off[q];
    const uint32_t i = (uint32_t)(gid - qbase);
    const uint32_t len = a.q_len[q];
    const uint8_t* text = a.text + qbase;
    const uint32_t k = a.term_size;

    // canonicalize == 1: any character outside ACGT makes the query invalid
    // (the reference dies, classic_search.cpp:93-96).  Every character of a
    // query of length >= k lies in some k-mer.
    // (invalid_bases != 0: such a character only takes the terms that hold it out of the count, below)
    const bool lenient = a.canonicalize != 0 && a.invalid_bases != 0;
    if (a.canonicalize != 0 && !lenient && i < len) {
        if (fwd_base(text[i]) == 0) atomicMax(a.err_query, 0xFFFFFFFFu - q);   // first bad query wins
    }

    const uint64_t b0 = a.blk_off[q];
    const uint32_t nblk = (uint32_t)(a.blk_off[q + 1] - b0);
    const uint32_t T = len - k + 1;
    // every (query, sub-index) table has nblk blocks of 8 terms plus one all-padding
    // block that lanes without work in a trip of K2 point at
    const uint32_t tblk = nblk + 1u;
    if (i >= tblk * 8u) return;
    const uint32_t H = a.num_hashes;
    const uint32_t blk = i >> 3, sub = i & 7u;
    const RowTableWriter<IdxT> tab(a.table, b0, q, a.npages, H, tblk);

    bool term_ok = true;
    if (lenient) {
        if (i < T) {
            uint32_t good = 1u;
            for (uint32_t s = 0; s < k; ++s) good &= fwd_base(text[i + s]) != 0 ? 1u : 0u;
            term_ok = good != 0;
        }
        if (a.valid != nullptr) add_valid_position(a.valid, q, i < T && term_ok && window_tail_valid(text + i + k, i, T, a.findere));
    }

    if (i >= T || !term_ok) {       // padding term (or one that holds an invalid character): the all-zero row of every sub-index
        for (uint32_t p = 0; p < a.npages; ++p) {
            const IdxT zr = (IdxT)a.pages[p].sig;
            for (uint32_t j = 0; j < H; ++j) tab.out(p, blk, j, sub) = zr;
        }
        return;
    }

    KmerView kv{text + i, k, 0u};
    if (a.canonicalize != 0) {
        // util/query.cpp:143-199: first strict difference between the forward
        // base and the complement of the mirrored base decides; the middle base
        // of an odd k is not compared; ties keep the forward k-mer.
        uint32_t mode = 1;
        for (uint32_t s = 0; s < k / 2; ++s) {
            const int f = (int)fwd_base(text[i + s]);
            const int r = (int)rev_base(text[i + k - 1 - s]);
            if (f < r) break;
            if (f > r) { mode = 2; break; }
        }
        kv.mode = mode;
    }
    for (uint32_t j = 0; j < H; ++j) {
        const uint64_t h = xxh64_view(kv, (uint64_t)j);
        for (uint32_t p = 0; p < a.npages; ++p) {
            const PageDev pg = a.pages[p];
            tab.out(p, blk, j, sub) = (IdxT)fast_mod(h, pg.sig, pg.magic);
        }
    }
}

// K1 specialised for k = 31 (the COBS default): the 31-mer lives in eight 32-bit
// registers, complement and reversal are done four bases at a time, and the
// reference's comparison of the first 15 positions (util/query.cpp:155-190) becomes
// a big-endian integer comparison of forward vs reverse complement (canon31, term_hash.hpp).
template <typename IdxT>
__global__ __launch_bounds__(256) void hash_kernel_k31(HashArgs a, uint64_t total_threads) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total_threads || gid >= a.span_off[a.nq]) return;
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.span_off[mid] <= gid) lo = mid; else hi = mid;
    }
    const uint32_t q = lo;
    const uint64_t qbase = a.span_off[q];
    const uint32_t i = (uint32_t)(gid - qbase);
    const uint32_t len = a.q_len[q];
    const uint8_t* text = a.text + qbase;
    const bool lenient = a.canonicalize != 0 && a.invalid_bases != 0;
    if (a.canonicalize != 0 && !lenient && i < len) {
        if (fwd_base(text[i]) == 0) atomicMax(a.err_query, 0xFFFFFFFFu - q);   // first bad query wins
    }
    const uint64_t b0 = a.blk_off[q];
    const uint32_t nblk = (uint32_t)(a.blk_off[q + 1] - b0);
    const uint32_t T = len - 31u + 1u;
    const uint32_t tblk = nblk + 1u;
    if (i >= tblk * 8u) return;
    const uint32_t H = a.num_hashes;
    const uint32_t blk = i >> 3, sub = i & 7u;
    const RowTableWriter<IdxT> tab(a.table, b0, q, a.npages, H, tblk);
    // the k-mer and one following byte as 8 (unaligned) dwords; the text buffer is padded
    uint32_t f[8];
    if (i < T) load31(text + i, f);
    bool term_ok = true;
    if (lenient) {
        if (i < T) term_ok = valid31(f);
        if (a.valid != nullptr) add_valid_position(a.valid, q, i < T && term_ok && window_tail_valid(text + i + 31u, i, T, a.findere));
    }
    if (i >= T || !term_ok) {
        for (uint32_t p = 0; p < a.npages; ++p) {
            const IdxT zr = (IdxT)a.pages[p].sig;
            for (uint32_t j = 0; j < H; ++j) tab.out(p, blk, j, sub) = zr;
        }
        return;
    }
    uint32_t c[8];
    term31(f, a.canonicalize != 0, c);
    for (uint32_t j = 0; j < H; ++j) {
        const uint64_t h = xxh64_31(c, (uint64_t)j);
        for (uint32_t p = 0; p < a.npages; ++p) {
            const PageDev pg = a.pages[p];
            tab.out(p, blk, j, sub) = (IdxT)fast_mod(h, pg.sig, pg.magic);
        }
    }
}

// ---------------------------------------------------------------------------
// launchers

hipError_t launch_hash(const HashArgs& a, uint64_t total_threads, hipStream_t stream) {
    if (total_threads == 0) return hipSuccess;
    const uint64_t blocks = (total_threads + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (a.term_size == 31) {
        if (a.idx64) hipLaunchKernelGGL(hash_kernel_k31<uint64_t>, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total_threads);
        else hipLaunchKernelGGL(hash_kernel_k31<uint32_t>, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total_threads);
    } else {
        if (a.idx64) hipLaunchKernelGGL(hash_kernel<uint64_t>, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total_threads);
        else hipLaunchKernelGGL(hash_kernel<uint32_t>, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total_threads);
    }
    return hipGetLastError();
}

hipError_t launch_skip_thresholds(const SkipThresholdArgs& a, hipStream_t stream) {
    if (a.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(skip_thresholds_kernel, dim3((a.nq + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
