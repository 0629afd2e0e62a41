// cobs_amd/csrc/topk_kernels.hip -- K3 of the COBS query path (gfx950, wave64): exact top-k per query
// (partial_sort of counts_to_result, reference classic_search.cpp:134-145) over score rows or K2's candidate pool,
// and the threshold filter over accumulated score rows (select_rows_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_types.hpp"
#include "kernels.hpp"
#include "wave_ops.hpp"      // pool_append

namespace cobs_amd {

// ---------------------------------------------------------------------------
// K3: exact top-k selection per query (the device side of counts_to_result's
// partial_sort, reference classic_search.cpp:127-145, for all three Score widths of
// :453-504): find the score s* of the k-th best document with a radix descent over the
// score bits (histogram levels of at most 12 bits each: one level for 8/10/12-bit scores,
// two up to 24 bits, three for 32-bit scores), emit every document with score > s* and, in
// ascending document order, as many documents with score == s* as are still needed, then
// order the <= k survivors by (score desc, document asc) in LDS (bitonic sort on
// (~score, doc) keys) -- the host copies the result as is.
// One work-group (4 waves) per query; wave w owns the contiguous quarter w of the
// documents so that ballot prefixes keep document order.

__device__ __forceinline__ uint32_t wave_prefix(unsigned long long mask, uint32_t lane) {
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane, uint32_t* total) {
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += t;
    }
    *total = __shfl(incl, 63);
    return incl - v;
}

// eight consecutive scores (u8, u16 or u32) starting at document i (a multiple of 8)
template <typename ST>
__device__ __forceinline__ void load_scores8(const ST* row, uint32_t i, uint32_t (&s)[8]) {
    if constexpr (sizeof(ST) == 1) {
        const uint2 v = *reinterpret_cast<const uint2*>(row + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = ((j < 4 ? v.x : v.y) >> ((j & 3) * 8)) & 0xFFu;
    } else if constexpr (sizeof(ST) == 2) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
    } else {
        const uint4 a = *reinterpret_cast<const uint4*>(row + i);
        const uint4 b = *reinterpret_cast<const uint4*>(row + i + 4);
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
        s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    }
}

// Dynamic LDS: hist[4 waves][NB] (NB = 2^level_bits <= 4096; reused by every level and, after
// the emission, as the sort buffer: 8192 eight-byte keys) | partial[256] | sh[16]
// POOL: the input is not a score row but the candidate pool of run_topk without score rows (K2's tile_topk):
// nslots (document, score) entries per query in ascending document order, unused ones marked with
// document 0xFFFFFFFF; the same selection and ordering over tiles x k candidates.
template <typename ST, bool POOL>
__device__ __forceinline__ void load_elems8(const void* rowp, uint32_t i, uint32_t w1, uint32_t doc_base, uint32_t thr,
                                            uint32_t (&s)[8], uint32_t (&d)[8], uint32_t& okmask) {
    okmask = 0u;
    if constexpr (POOL) {
        const uint4* e = reinterpret_cast<const uint4*>(reinterpret_cast<const uint2*>(rowp) + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 v = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);
            if (i + 2 * j < w1) v = e[j];            // two entries per load; the row is padded to 8 entries, i is a multiple of 8
            d[2 * j] = v.x; s[2 * j] = v.y; d[2 * j + 1] = v.z; s[2 * j + 1] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i + j < w1 && d[j] != 0xFFFFFFFFu && s[j] >= thr) okmask |= 1u << j;
    } else {
        load_scores8<ST>(reinterpret_cast<const ST*>(rowp), i, s);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d[j] = doc_base + i + j;
            if (i + j < w1 && s[j] >= thr) okmask |= 1u << j;
        }
    }
}

template <typename ST, bool POOL = false>
__global__ __launch_bounds__(256) void topk_kernel(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t NB = 1u << a.level_bits;
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    uint32_t* partial = hist + 4u * NB;
    uint32_t* sh = partial + 256;
    const uint32_t q = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const void* row = POOL ? (const void*)(reinterpret_cast<const uint2*>(a.counts) + (uint64_t)q * a.counts_stride)
                           : (const void*)(reinterpret_cast<const ST*>(a.counts) + (uint64_t)q * a.counts_stride + a.counts_offset);
    const uint32_t thr = a.thresholds ? a.thresholds[q] : 0u;
    uint32_t n = a.nslots;                       // real documents among the local slots (POOL: pool entries)
    if constexpr (!POOL) {
        if (a.doc_base >= a.num_docs) n = 0;
        else if (a.num_docs - a.doc_base < n) n = a.num_docs - a.doc_base;
    }
    const uint32_t k = a.k;
    // wave w owns the contiguous document range [w0, w1); 512 documents per iteration
    const uint32_t per = ((n + 3u) / 4u + 511u) / 512u * 512u;
    const uint32_t w0 = wave * per < n ? wave * per : n;
    const uint32_t w1 = w0 + per < n ? w0 + per : n;

    // ---- radix descent: after level l the top (l+1)*level_bits bits of s* are known
    uint32_t prefix = 0, n_above = 0, take_all = 0;
    uint32_t bits_left = a.score_bits;           // bits below the known prefix
    uint32_t* myh = hist + wave * NB;
    for (uint32_t level = 0; level < a.levels; ++level) {
        const uint32_t lb = bits_left < a.level_bits ? bits_left : a.level_bits;     // bits of this level
        const uint32_t shift = bits_left - lb;
        const uint32_t nb = 1u << lb, mask = nb - 1u;
        for (uint32_t i = tid; i < 4u * NB; i += 256) hist[i] = 0;
        __syncthreads();
        for (uint32_t i0 = w0; i0 < w1; i0 += 512) {
            const uint32_t i = i0 + lane * 8u;
            if (i < w1) {
                uint32_t sc[8], dc[8], ok;
                load_elems8<ST, POOL>(row, i, w1, a.doc_base, thr, sc, dc, ok);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t s = sc[j];
                    // the bits above this level must equal the prefix found so far
                    const bool in = level == 0 || (bits_left >= 32u ? true : (s >> bits_left) == prefix);
                    if ((ok >> j & 1u) && in) atomicAdd(&myh[(s >> shift) & mask], 1u);
                }
            }
        }
        __syncthreads();
        {   // parallel search of the bin holding the k-th best: per-thread segment sums, then thread 0
            const uint32_t seg = (nb + 255u) / 256u;
            uint32_t sum = 0;
            for (uint32_t b = tid * seg; b < (tid + 1) * seg && b < nb; ++b)
                sum += hist[b] + hist[NB + b] + hist[2 * NB + b] + hist[3 * NB + b];
            partial[tid] = sum;
            __syncthreads();
            if (tid == 0) {
                uint32_t above = n_above;
                int t = 255;
                for (; t >= 0; --t) {
                    if (above + partial[t] >= k) break;
                    above += partial[t];
                }
                int hb = -1;
                if (t >= 0) {
                    int b = (int)((uint32_t)(t + 1) * seg) - 1;
                    if (b >= (int)nb) b = (int)nb - 1;
                    for (; b >= (int)((uint32_t)t * seg); --b) {
                        const uint32_t c = hist[b] + hist[NB + b] + hist[2 * NB + b] + hist[3 * NB + b];
                        if (above + c >= k) { hb = b; break; }
                        above += c;
                    }
                }
                sh[0] = hb < 0 ? 0u : (uint32_t)hb;
                sh[1] = above;
                sh[2] = hb < 0 ? 1u : 0u;        // fewer than k passing documents: take them all
            }
            __syncthreads();
        }
        const uint32_t hb = sh[0];
        n_above = sh[1];
        take_all = sh[2];
        prefix = (lb >= 32u ? 0u : (prefix << lb)) | hb;
        bits_left = shift;
        if (take_all) break;                     // only possible at level 0 (block-uniform)
        if (level + 1 < a.levels) __syncthreads();        // hist is zeroed again
    }
    uint32_t cut = take_all ? thr : prefix;
    // ties: documents with score == cut, per wave (the last level's per-wave histogram bins)
    uint32_t eq_base = 0, eq_total = 0;
    if (!take_all) {
        const uint32_t lastbits = a.score_bits - (a.levels - 1u) * a.level_bits;
        const uint32_t bin = cut & ((lastbits >= 32u ? 0u : (1u << lastbits)) - 1u);
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t c = hist[w * NB + bin];
            if (w < wave) eq_base += c;
            eq_total += c;
        }
    }
    const uint32_t need_eq = take_all ? 0u : k - n_above;
    if (tid == 0) sh[5] = 0;                      // emission cursor of the documents above the cut
    __syncthreads();
    // ---- emission
    uint2* out = a.out + (uint64_t)q * (a.out_stride ? a.out_stride : k);
    for (uint32_t i0 = w0; i0 < w1; i0 += 512) {
        const uint32_t i = i0 + lane * 8u;
        uint32_t s8[8], d8[8];
        uint32_t gt = 0, eq = 0;
        if (i < w1) {
            uint32_t ok;
            load_elems8<ST, POOL>(row, i, w1, a.doc_base, thr, s8, d8, ok);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t s = s8[j];
                const bool pass = (ok >> j & 1u) != 0u;
                if (pass && (take_all || s > cut)) gt |= 1u << j;
                if (pass && !take_all && s == cut) eq |= 1u << j;
            }
        }
        if (__any(gt != 0u)) {
            uint32_t total;
            const uint32_t excl = wave_excl_scan((uint32_t)__popc(gt), lane, &total);
            uint32_t base = 0;
            if (lane == 63u) base = atomicAdd(&sh[5], total);
            base = __shfl(base, 63);
            uint32_t pos = base + excl;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (gt & (1u << j)) out[pos++] = make_uint2(d8[j], s8[j]);
        }
        if (__any(eq != 0u)) {
            uint32_t total;
            const uint32_t excl = wave_excl_scan((uint32_t)__popc(eq), lane, &total);
            uint32_t r = eq_base + excl;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (eq & (1u << j)) {
                    if (r < need_eq) out[n_above + r] = make_uint2(d8[j], s8[j]);
                    ++r;
                }
            eq_base += total;
        }
    }
    __syncthreads();
    const uint32_t cnt = take_all ? sh[5] : n_above + (eq_total < need_eq ? eq_total : need_eq);
    if (tid == 0 && a.out_count) a.out_count[q] = cnt;
    // (one tile of the candidate pool: what the survivors leave of its k entries is marked unused, as tile_topk does)
    if (a.pad_out)
        for (uint32_t i = cnt + tid; i < k; i += 256) out[i] = make_uint2(0xFFFFFFFFu, 0u);
    // ---- order the survivors: (score desc, doc asc) = ascending (~score << 32 | doc)
    if (a.sort_limit && cnt > 1u && cnt <= a.sort_limit) {      // block-uniform condition
        __syncthreads();                          // everybody has read sh[]: the key area may overlap it
        unsigned long long* key = reinterpret_cast<unsigned long long*>(smem);
        uint32_t m = 2;
        while (m < cnt) m <<= 1;
        for (uint32_t i = tid; i < m; i += 256) {
            unsigned long long kv = ~0ull;        // padding sorts last
            if (i < cnt) {
                const uint2 e = out[i];
                kv = ((unsigned long long)(~e.y) << 32) | e.x;
            }
            key[i] = kv;
        }
        __syncthreads();
        for (uint32_t size = 2; size <= m; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t t = tid; t < (m >> 1); t += 256) {
                    const uint32_t lo = (t / stride) * (stride << 1) + (t % stride), hi = lo + stride;
                    const bool up = ((lo & size) == 0u);
                    const unsigned long long x = key[lo], y = key[hi];
                    if ((x > y) == up) { key[lo] = y; key[hi] = x; }
                }
                __syncthreads();
            }
        }
        for (uint32_t i = tid; i < cnt; i += 256) {
            const unsigned long long kv = key[i];
            out[i] = make_uint2((uint32_t)kv, ~(uint32_t)(kv >> 32));
        }
    }
}

// ---------------------------------------------------------------------------
// The threshold filter over ACCUMULATED scores (reference classic_search.cpp:127-132).  A streamed sub-index that is
// larger than a stream buffer is counted row range by row range (pass.cpp): K2 sees partial counts there and cannot
// compare them with a threshold.  Its ranges add up in a scratch matrix of the sub-index's own width (no score rows of
// the whole index), and after the last range this kernel does what K2's epilogue does for a sub-index it sees whole:
// score >= threshold over real documents -> (query, file, document, score) records into the batch's hit pool, one
// wave-aggregated atomic per wave.  One thread per (query, 8 consecutive slots).
template <typename ST>
__global__ __launch_bounds__(256) void select_rows_kernel(SelectRowsArgs a) {
    const uint32_t groups = (a.nslots + 7u) / 8u;
    const uint64_t gid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t qq = gid / groups;
    const bool live = qq < a.nq;                      // (no early return: the scan below runs over whole waves)
    const uint32_t q = live ? (uint32_t)qq : 0u;
    const uint32_t i = (uint32_t)(gid - qq * groups) * 8u;
    uint32_t s8[8];
    uint32_t mask = 0u;
    if (live) {
        load_scores8<ST>(reinterpret_cast<const ST*>(a.scores) + (uint64_t)q * a.stride, i, s8);
        const uint32_t thr = a.thresholds[q];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i + j < a.nslots && a.doc0 + i + j < a.num_docs && s8[j] >= thr) mask |= 1u << j;
    }
    if (__any(mask != 0u)) {
        unsigned long long pos = pool_append((uint32_t)__popc(mask), a.hit_count, lane);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (mask & (1u << j)) {
                if (pos < a.hit_cap) a.hits[pos] = HitDev{q, a.part, a.doc0 + i + (uint32_t)j, s8[j]};
                ++pos;
            }
    }
}

// ---------------------------------------------------------------------------
// launchers

hipError_t launch_topk(const TopkArgs& a, hipStream_t stream) {
    if (a.nq == 0 || a.k == 0) return hipSuccess;
    if (a.level_bits == 0 || a.level_bits > 12 || a.levels == 0 || a.levels * a.level_bits < a.score_bits ||
        (a.levels - 1) * a.level_bits >= a.score_bits)
        return hipErrorInvalidValue;
    const uint32_t nb = 1u << a.level_bits;
    size_t lds = (size_t)(4 * nb + 256 + 16) * sizeof(uint32_t);
    // the sort reuses the histogram area: 8 bytes per survivor
    uint32_t m = 2;
    while (m < a.sort_limit) m <<= 1;
    if (a.sort_limit) lds = std::max(lds, (size_t)m * 8);
    auto kern = a.from_pool ? topk_kernel<uint32_t, true>
              : a.score_bytes == 1 ? topk_kernel<uint8_t> : a.score_bytes == 2 ? topk_kernel<uint16_t> : topk_kernel<uint32_t>;
    if (a.score_bytes != 1 && a.score_bytes != 2 && a.score_bytes != 4) return hipErrorInvalidValue;
    if (a.from_pool && ((a.counts_stride & 7u) != 0u || a.counts_stride < a.nslots)) return hipErrorInvalidValue;   // 64-byte rows
    if (lds > 64 * 1024 + 2048) return hipErrorInvalidValue;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(a.nq), dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_select_rows(const SelectRowsArgs& a, hipStream_t stream) {
    if (a.nq == 0 || a.nslots == 0) return hipSuccess;
    if ((a.stride % 8u) != 0 || (a.elem_bytes != 1 && a.elem_bytes != 2 && a.elem_bytes != 4)) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)a.nq * ((a.nslots + 7u) / 8u);
    const uint64_t blocks = (items + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    auto kern = a.elem_bytes == 1 ? select_rows_kernel<uint8_t> : a.elem_bytes == 2 ? select_rows_kernel<uint16_t> : select_rows_kernel<uint32_t>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
