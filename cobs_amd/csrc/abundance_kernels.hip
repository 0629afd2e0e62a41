// cobs_amd/csrc/abundance_kernels.hip -- gfx950 kernels of the k-mer abundance cutoff of index
// construction (semantics, table layout: abundance_kernels.hpp).
//
// Both kernels read a staged batch through the stretch tables build_kernel reads: a position is a
// term exactly when build_kernel would hash it, and a term is hashed by the very device code
// build_kernel uses (term_hash.hpp).
//   abundance_count_kernel  one thread per text byte: the term at that position is looked up in an
//                           open-addressing table keyed by (document, canonical bytes), linear
//                           probing; the first occurrence claims a slot with one 64-bit atomicCAS,
//                           every occurrence adds 1 to the slot's count while it is below c
//   abundance_emit_kernel   one thread per slot: a slot whose count reached c re-reads its term at
//                           the stored offset, hashes it with seeds 0 .. H-1 and sets the H bits of
//                           its document -- once per distinct kept term
// No thread ever waits for another: a lost claim is an ordinary occupied slot.  Every store is a
// vector atomic or a plain vector store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abundance_kernels.hpp"
#include "device_types.hpp"
#include "term_hash.hpp"

namespace cobs_amd {
namespace {

constexpr uint64_t kOffsetMask = (1ull << kAbundanceOffsetBits) - 1ull;
constexpr uint64_t kKeySeed = 0x5851F42D4C957F2DULL;      // the table's XXH64 seed (the rows use 0 .. H-1)

// the splitmix64 finaliser (build_kernels.hip's mix64, which stays where it is)
__device__ __forceinline__ uint64_t ab_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// A term as the hash function sees it: a 31-mer that takes build_kernel's register path (`fast`:
// canonicalize = 0, or all bases valid) is its eight canonical dwords, anything else a byte view.
struct Term {
    uint32_t c[8];
    KmerView kv;
    bool fast;
};

// The term that starts at p, by build_kernel's rules.  -> false if check_nl and the k characters
// hold a '\n' (the term would span a sequence boundary).
__device__ __forceinline__ bool term_load(const uint8_t* p, uint32_t k, uint32_t canonicalize, bool check_nl, Term& t) {
    t.fast = false;
    if (k == 31u) {
        uint32_t f[8];
        {
            const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
            const uint32_t* w = reinterpret_cast<const uint32_t*>(p - mis);
            uint32_t r[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) r[j] = w[j];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[j] = mis == 0 ? r[j] : (uint32_t)(((uint64_t)r[j] | ((uint64_t)r[j + 1] << 32)) >> (8 * mis));
        }
        f[7] &= 0x00FFFFFFu;
        if (check_nl) {
            bool nl = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) nl |= has_newline(f[j]);
            if (nl) return false;
        }
        bool fast = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) t.c[j] = f[j];
        if (canonicalize != 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) fast &= all_acgt(f[j]);
            fast &= all_acgt(f[7] | 0x41000000u);
            if (fast) canon31(f, t.c);
        }
        t.fast = fast;
        if (fast) return true;
    } else if (check_nl) {
        for (uint32_t i = 0; i < k; ++i)
            if (p[i] == '\n') return false;
    }
    t.kv = KmerView{p, k, 0u};
    if (canonicalize != 0) {
        uint32_t mode = 1;
        for (uint32_t s = 0; s < k / 2; ++s) {
            const int f = (int)fwd_base(p[s]);
            const int r = (int)rev_base(p[k - 1 - s]);
            if (f < r) break;
            if (f > r) { mode = 2; break; }
        }
        t.kv.mode = mode;
    }
    return true;
}

__device__ __forceinline__ uint64_t term_hash(const Term& t, uint64_t seed) {
    return t.fast ? xxh64_31(t.c, seed) : xxh64_view(t.kv, seed);
}

// equal bytes handed to the hash function?  (With canonicalize = 1 a 31-mer off the register path
// holds a 0 byte and one on it does not; with canonicalize = 0 every 31-mer is on it.)
__device__ __forceinline__ bool term_equal(const Term& x, const Term& y, uint32_t k) {
    if (x.fast != y.fast) return false;
    if (x.fast) {
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) d |= x.c[j] ^ y.c[j];
        return d == 0u;
    }
    for (uint32_t i = 0; i < k; ++i)
        if (x.kv.at(i) != y.kv.at(i)) return false;
    return true;
}

// the stretch that holds batch offset o (o < seg_off[nsegs])
__device__ __forceinline__ uint32_t stretch_of(const BuildArgs& b, uint64_t o) {
    uint32_t lo = 0, hi = b.nsegs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (b.seg_off[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// L1 is per CU and not refreshed by other CUs' atomics: table words are read at agent scope
__device__ __forceinline__ uint64_t load_owner(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_count(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void abundance_count_kernel(AbundanceArgs a) {
    const BuildArgs& b = a.b;
    // the position's stretch, as in build_kernel
    const uint64_t base = (uint64_t)blockIdx.x * 256u;
    uint32_t lo = stretch_of(b, base);
    const uint64_t gid = base + threadIdx.x;
    if (gid >= a.total) return;
    while (b.seg_off[lo + 1] <= gid) ++lo;            // seg_off[nsegs] = total > gid
    const uint32_t k = b.term_size;
    if (gid + k > b.seg_off[lo + 1]) return;          // the term would leave its stretch
    const uint32_t colw = b.seg_col[lo];
    if (colw == kBuildGapStretch) return;
    const bool raw = (colw & kBuildRawStretch) != 0u;
    const uint32_t doc = colw & ~kBuildRawStretch;
    Term t;
    if (!term_load(b.text + gid, k, b.canonicalize, !raw, t)) return;

    const uint64_t h = ab_mix64(term_hash(t, kKeySeed) ^ ((uint64_t)doc * 0x9E3779B97F4A7C15ULL));
    const uint64_t mine = (h & ~kOffsetMask) | (gid + 1u);        // tag = the top 24 bits, slot = the low ones
    const uint64_t s0 = b.seg_off[lo], s1 = b.seg_off[lo + 1];
    uint64_t slot = h & a.mask;
    for (;; slot = (slot + 1u) & a.mask) {            // the table is at most half full: a free slot ends every probe
        uint64_t v = load_owner(a.owner + slot);
        if (v == 0ull) {
            v = atomicCAS(a.owner + slot, 0ull, (unsigned long long)mine);
            if (v == 0ull) break;                     // first occurrence: the slot is this term's
        }
        if (((v ^ mine) >> kAbundanceOffsetBits) != 0ull) continue;       // another (document, term)
        const uint64_t o = (v & kOffsetMask) - 1u;
        // same document?  (mostly the same stretch; a document may have several)
        if ((o < s0 || o >= s1) && (b.seg_col[stretch_of(b, o)] & ~kBuildRawStretch) != doc) continue;
        Term u;
        term_load(b.text + o, k, b.canonicalize, false, u);
        if (term_equal(t, u, k)) break;
    }
    // saturating: add only while below c (racing threads may overshoot by at most one each)
    if (load_count(a.count + slot) < a.min_count) atomicAdd(a.count + slot, 1u);
}

__global__ __launch_bounds__(256) void abundance_emit_kernel(AbundanceArgs a) {
    const BuildArgs& b = a.b;
    const uint64_t slot = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (slot > a.mask) return;
    if (a.count[slot] < a.min_count) return;
    const uint64_t o = ((uint64_t)a.owner[slot] & kOffsetMask) - 1u;
    const uint32_t doc = b.seg_col[stretch_of(b, o)] & ~kBuildRawStretch;
    Term t;
    term_load(b.text + o, b.term_size, b.canonicalize, false, t);
    for (uint32_t j = 0; j < b.num_hashes; ++j) {
        const uint64_t row = fast_mod(term_hash(t, (uint64_t)j), b.signature_size, b.magic);
        set_term_bit(b, doc, row);
    }
}

}  // namespace

hipError_t launch_abundance(const AbundanceArgs& a, hipStream_t stream) {
    if (a.total == 0 || a.b.nsegs == 0) return hipSuccess;
    if (a.min_count < 2 || (a.mask & (a.mask + 1)) != 0 || a.mask + 1 < 2 * a.total) return hipErrorInvalidValue;
    if (a.total >= kOffsetMask) return hipErrorInvalidValue;
    const uint64_t blocks = (a.total + 255) / 256, eblocks = (a.mask + 256) / 256;
    if (blocks > 0x7FFFFFFFull || eblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(abundance_count_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(abundance_emit_kernel, dim3((uint32_t)eblocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
