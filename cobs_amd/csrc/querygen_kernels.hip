// cobs_amd/csrc/querygen_kernels.hip -- gfx950 kernels of generate-queries (reference
// src/cobs.cpp:734-959): the document term scan that the reference runs on host threads
// (process_terms per document, a mutex-guarded hash set of negative terms).
//
// The kernels read a staged batch of documents (staging.hpp) through the stretch tables that
// build_kernel reads: a position is a term exactly when build_kernel would hash it (gap stretches
// hold none; in a raw stretch '\n' is an ordinary character).  Per batch:
//   qg_count_kernel    terms per 256 positions (wave ballot + popcount)
//   qg_scan_kernel     exclusive prefix of those counts (one work-group)
//   qg_doc_base_kernel the batch rank of every document's first term (one thread per stretch)
//   qg_emit_kernel     every term's document-local index (process_terms order); a drawn positive's
//                      k bytes go to its output slot; with -N an ACGT term is packed 2 bits per base
//                      (canonicalised with --canonical) and looked up in the table of the negative
//                      candidates' terms, a hit stores 1 into found[candidate]
// and once per call qg_insert_kernel fills that table.  Every store is a plain vector store or a
// vector atomic; exactly one thread owns every positive, and found[] is only ever set to 1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "querygen_kernels.hpp"

namespace cobs_amd {
namespace {

// the splitmix64 finaliser (build_kernels.hip's mix64, kept local so that file stays as it is)
__device__ __forceinline__ uint64_t qg_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ bool qg_has_newline(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u;
}

__device__ __forceinline__ bool qg_is_acgt(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// A 0, C 1, G 2, T 3 (lexicographic, so the canonical comparison is an integer comparison; the
// complement is 3 - code).  (c >> 1) & 3 gives A 0, C 1, G 3, T 2.
__device__ __forceinline__ uint64_t qg_code(uint32_t c) {
    const uint32_t x = (c >> 1) & 3u;
    return (uint64_t)(x ^ (x >> 1));
}

// Base i of the term -> bits 2 (i % 32) of word i / 32.  `fw` is the term, `rc` its reverse complement.
// canonicalize_kmer (util/query.cpp:143-199): the first strict difference among positions
// 0 .. k/2 - 1 decides, ties keep the forward k-mer.  -> false if the term holds a non-ACGT byte.
template <typename ByteAt>
__device__ __forceinline__ bool qg_pack(ByteAt at, uint32_t k, uint32_t words, bool canonical, uint64_t (&key)[kQgMaxWords]) {
    uint64_t fw[kQgMaxWords], rc[kQgMaxWords];
    bool ok = true;
#pragma unroll
    for (uint32_t w = 0; w < kQgMaxWords; ++w) {
        fw[w] = 0;
        rc[w] = 0;
        if (w < words) {
            const uint32_t n = min(32u, k - w * 32u);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t c = at(w * 32u + i);
                ok &= qg_is_acgt(c);
                fw[w] |= qg_code(c) << (2 * i);
                rc[w] |= (3ull - qg_code(at(k - 1u - (w * 32u + i)))) << (2 * i);
            }
        }
    }
    bool use_rc = false, decided = !canonical;
    const uint32_t half = k / 2u;
#pragma unroll
    for (uint32_t w = 0; w < kQgMaxWords; ++w) {
        if (!decided && w * 32u < half) {
            const uint32_t n = min(32u, half - w * 32u);
            const uint64_t m = n == 32u ? ~0ull : (1ull << (2 * n)) - 1ull;
            const uint64_t d = (fw[w] ^ rc[w]) & m;
            if (d != 0ull) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(d) & ~1u;
                use_rc = ((fw[w] >> bit) & 3ull) > ((rc[w] >> bit) & 3ull);
                decided = true;
            }
        }
    }
#pragma unroll
    for (uint32_t w = 0; w < kQgMaxWords; ++w) key[w] = use_rc ? rc[w] : fw[w];
    return ok;
}

__device__ __forceinline__ uint64_t qg_hash(const uint64_t (&key)[kQgMaxWords], uint32_t words) {
    uint64_t h = 0x243F6A8885A308D3ULL;
#pragma unroll
    for (uint32_t w = 0; w < kQgMaxWords; ++w)
        if (w < words) h = qg_mix64(h ^ key[w]);
    return h;
}

// Is position gid of the batch a term?  lo = the stretch that holds gid.  For k = 31 the 31 bytes
// (and one more) come as 8 unaligned dword loads, as in build_kernel; f receives them.
__device__ __forceinline__ bool qg_term_at(const QgBatchArgs& a, uint64_t gid, uint32_t lo, uint32_t (&f)[8]) {
    const uint32_t k = a.term_size;
    if (gid + k > a.seg_off[lo + 1]) return false;        // the term would leave its stretch
    const uint32_t colw = a.seg_col[lo];
    if (colw == kBuildGapStretch) return false;
    const bool raw = (colw & kBuildRawStretch) != 0u;
    const uint8_t* p = a.text + gid;
    if (k == 31u) {
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p - mis);
        uint32_t r[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) r[j] = w[j];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            f[j] = mis == 0 ? r[j] : (uint32_t)(((uint64_t)r[j] | ((uint64_t)r[j + 1] << 32)) >> (8 * mis));
        f[7] &= 0x00FFFFFFu;
        if (raw) return true;
        bool nl = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) nl |= qg_has_newline(f[j]);
        return !nl;                                       // a term does not span a sequence boundary
    }
    if (!raw)
        for (uint32_t i = 0; i < k; ++i)
            if (p[i] == '\n') return false;
    return true;
}

// the stretch of the block's first position (wave-uniform search); threads walk on from there
__device__ __forceinline__ uint32_t qg_block_seg(const QgBatchArgs& a, uint64_t base) {
    uint32_t lo = 0, hi = a.nsegs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.seg_off[mid] <= base) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool qg_valid(const QgBatchArgs& a, uint64_t gid, uint32_t lo, uint32_t (&f)[8]) {
    if (gid >= a.total) return false;
    while (a.seg_off[lo + 1] <= gid) ++lo;                // seg_off[nsegs] = total > gid
    return qg_term_at(a, gid, lo, f);
}

__global__ __launch_bounds__(256) void qg_count_kernel(QgBatchArgs a) {
    __shared__ uint32_t s_cnt[4];
    const uint64_t base = (uint64_t)blockIdx.x * 256u;
    const uint32_t lo = qg_block_seg(a, base);
    uint32_t f[8];
    const bool valid = qg_valid(a, base + threadIdx.x, lo, f);
    const unsigned long long vm = __ballot(valid);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = (uint32_t)__popcll(vm);
    __syncthreads();
    if (threadIdx.x == 0) a.blk_cnt[blockIdx.x] = (uint64_t)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// in place: c[i] -> c[0] + .. + c[i - 1], one work-group of 1024 threads, a contiguous chunk each
__global__ __launch_bounds__(1024) void qg_scan_kernel(uint64_t* c, uint64_t n) {
    __shared__ uint64_t s[1024];
    const uint64_t per = (n + 1023u) / 1024u;
    const uint64_t b = min(n, (uint64_t)threadIdx.x * per), e = min(n, b + per);
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += c[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {     // Hillis-Steele inclusive scan of the chunk sums
        const uint64_t v = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = s[threadIdx.x] - sum;
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t v = c[i];
        c[i] = run;
        run += v;
    }
}

// the batch rank at the start of every document stretch; a document's base is the smallest
__global__ __launch_bounds__(256) void qg_doc_base_kernel(QgBatchArgs a) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.nsegs) return;
    const uint32_t colw = a.seg_col[s];
    if (colw == kBuildGapStretch) return;
    const uint32_t j = (colw & ~kBuildRawStretch) - a.col_base;
    const uint64_t p = a.seg_off[s];
    const uint64_t q0 = p & ~255ull;
    uint64_t rank = a.blk_cnt[q0 >> 8];
    uint32_t lo = qg_block_seg(a, q0);
    uint32_t f[8];
    for (uint64_t q = q0; q < p; ++q) rank += qg_valid(a, q, lo, f) ? 1u : 0u;
    if (j < a.ndocs) atomicMin(a.doc_base + j, (unsigned long long)rank);
}

__global__ __launch_bounds__(256) void qg_emit_kernel(QgBatchArgs a) {
    __shared__ uint32_t s_cnt[4];
    const uint64_t base = (uint64_t)blockIdx.x * 256u;
    const uint64_t gid = base + threadIdx.x;
    uint32_t lo = qg_block_seg(a, base);
    uint32_t f[8];
    bool valid = false;
    if (gid < a.total) {
        while (a.seg_off[lo + 1] <= gid) ++lo;
        valid = qg_term_at(a, gid, lo, f);
    }
    // the term's rank in the batch: block base + terms of the earlier waves + lanes below
    const unsigned long long vm = __ballot(valid);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(vm);
    __syncthreads();
    uint64_t rank = a.blk_cnt[blockIdx.x] + (uint64_t)__popcll(vm & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += s_cnt[w];
    const uint32_t k = a.term_size;
    const uint8_t* p = a.text + gid;
    bool probe = false;
    uint64_t key[kQgMaxWords];
    if (valid && a.probe) {
        if (k == 31u)
            probe = qg_pack([&](uint32_t i) { return (f[i >> 2] >> (8 * (i & 3u))) & 0xFFu; }, 31u, 1u, a.canonical != 0u, key);
        else
            probe = qg_pack([&](uint32_t i) { return (uint32_t)p[i]; }, k, a.table.words, a.canonical != 0u, key);
    }
    const unsigned long long pm = __ballot(probe);
    if (lane == 0u && pm != 0ull) atomicAdd(a.probed, (unsigned long long)__popcll(pm));
    if (!valid) return;
    // a drawn positive: the document's positives are sorted by term index
    const uint32_t j = (a.seg_col[lo] & ~kBuildRawStretch);
    const uint64_t local = rank - a.doc_base[j - a.col_base];
    uint64_t pl = a.vis_pos_off[j], ph = a.vis_pos_off[j + 1];
    while (pl < ph) {
        const uint64_t mid = (pl + ph) >> 1;
        if (a.pos_local[mid] < local) pl = mid + 1; else ph = mid;
    }
    if (pl < a.vis_pos_off[j + 1] && a.pos_local[pl] == local) {
        uint8_t* out = a.pos_text + pl * k;
        for (uint32_t i = 0; i < k; ++i) out[i] = p[i];
        a.pos_hit[pl] = 1;
    }
    if (!probe) return;
    const QgTable& t = a.table;
    for (uint64_t slot = qg_hash(key, t.words) & t.mask;; slot = (slot + 1) & t.mask) {
        const uint32_t v = t.vals[slot];
        if (v == 0u) break;
        bool eq = true;
#pragma unroll
        for (uint32_t w = 0; w < kQgMaxWords; ++w)
            if (w < t.words) eq &= t.keys[slot * t.words + w] == key[w];
        if (eq) a.found[(v - 1u) / t.cand_terms] = 1;
    }
}

// one thread per term occurrence of the negative candidates; a slot is claimed with one CAS on its
// value word (a failed claim moves on to the next slot: no thread ever waits on another)
__global__ __launch_bounds__(256) void qg_insert_kernel(QgInsertArgs a) {
    const uint64_t id = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const QgTable& t = a.table;
    if (id >= a.num_cand * t.cand_terms) return;
    const uint64_t cand = id / t.cand_terms, off = id - cand * t.cand_terms;
    const uint8_t* p = a.cand_text + cand * a.size + off;
    uint64_t key[kQgMaxWords];
    qg_pack([&](uint32_t i) { return (uint32_t)p[i]; }, a.term_size, t.words, a.canonical != 0u, key);
    uint64_t slot = qg_hash(key, t.words) & t.mask;
    while (atomicCAS(t.vals + slot, 0u, (uint32_t)id + 1u) != 0u) slot = (slot + 1) & t.mask;
#pragma unroll
    for (uint32_t w = 0; w < kQgMaxWords; ++w)
        if (w < t.words) t.keys[slot * t.words + w] = key[w];
}

}  // namespace

hipError_t launch_qg_insert(const QgInsertArgs& a, hipStream_t stream) {
    const uint64_t total = a.num_cand * a.table.cand_terms;
    if (total == 0) return hipSuccess;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qg_insert_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_qg_batch(const QgBatchArgs& a, hipStream_t stream) {
    if (a.total == 0 || a.nsegs == 0) return hipSuccess;
    const uint64_t blocks = (a.total + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qg_count_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(qg_scan_kernel, dim3(1), dim3(1024), 0, stream, a.blk_cnt, blocks);
    hipError_t e = hipMemsetAsync(a.doc_base, 0xFF, (size_t)a.ndocs * 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(qg_doc_base_kernel, dim3((a.nsegs + 255u) / 256u), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(qg_emit_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
