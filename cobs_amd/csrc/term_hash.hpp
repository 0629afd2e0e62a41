// cobs_amd/csrc/term_hash.hpp -- the __device__ code that turns a term into its signature rows,
// shared by the kernels that hash terms: hash_kernels.hip (hash_kernel), build_kernels.hip (build_kernel,
// random_build_kernel, plant_kernel) and abundance_kernels.hip (the min_count builder).  One definition of the
// canonicalisation (canonicalize_kmer, reference util/query.cpp:143-199), of XXH64 (public xxHash
// specification) and of where a term's bit goes, so that every path sets the bits a query looks up.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"

namespace cobs_amd {

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// exact n % d with the precomputed m = floor((2^64-1)/d); the estimate
// q = hi64(n*m) is at most 2 below the true quotient.
__device__ __forceinline__ uint64_t fast_mod(uint64_t n, uint64_t d, uint64_t m) {
    uint64_t q = __umul64hi(n, m);
    uint64_t r = n - q * d;
    if (r >= d) r -= d;
    if (r >= d) r -= d;
    return r;
}

__device__ __forceinline__ uint32_t fwd_base(uint32_t c) {
    return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : 0u;
}
__device__ __forceinline__ uint32_t rev_base(uint32_t c) {
    return c == 'A' ? (uint32_t)'T' : c == 'C' ? (uint32_t)'G' : c == 'G' ? (uint32_t)'C'
         : c == 'T' ? (uint32_t)'A' : 0u;
}

constexpr uint64_t XP1 = 0x9E3779B185EBCA87ULL;
constexpr uint64_t XP2 = 0xC2B2AE3D27D4EB4FULL;
constexpr uint64_t XP3 = 0x165667B19E3779F9ULL;
constexpr uint64_t XP4 = 0x85EBCA77C2B2AE63ULL;
constexpr uint64_t XP5 = 0x27D4EB2F165667C5ULL;

__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) {
    return rotl64(acc + in * XP2, 31) * XP1;
}
__device__ __forceinline__ uint64_t xmerge(uint64_t h, uint64_t v) {
    return (h ^ xround(0, v)) * XP1 + XP4;
}

// canonical k-mer as a byte accessor: mode 0 raw, 1 forward-mapped, 2 reverse complement
struct KmerView {
    const uint8_t* p;
    uint32_t k;
    uint32_t mode;
    __device__ __forceinline__ uint32_t at(uint32_t i) const {
        if (mode == 0) return p[i];
        if (mode == 1) return fwd_base(p[i]);
        return rev_base(p[k - 1 - i]);
    }
    __device__ __forceinline__ uint64_t le64(uint32_t i) const {
        uint64_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) v |= (uint64_t)at(i + b) << (8 * b);
        return v;
    }
    __device__ __forceinline__ uint64_t le32(uint32_t i) const {
        uint64_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) v |= (uint64_t)at(i + b) << (8 * b);
        return v;
    }
};

// XXH64 of the viewed k bytes (public xxHash specification; any k)
__device__ inline uint64_t xxh64_view(const KmerView& kv, uint64_t seed) {
    const uint32_t len = kv.k;
    uint32_t pos = 0;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + XP1 + XP2, v2 = seed + XP2, v3 = seed, v4 = seed - XP1;
        do {
            v1 = xround(v1, kv.le64(pos));
            v2 = xround(v2, kv.le64(pos + 8));
            v3 = xround(v3, kv.le64(pos + 16));
            v4 = xround(v4, kv.le64(pos + 24));
            pos += 32;
        } while (pos + 32 <= len);
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xmerge(h, v1); h = xmerge(h, v2); h = xmerge(h, v3); h = xmerge(h, v4);
    } else {
        h = seed + XP5;
    }
    h += (uint64_t)len;
    while (pos + 8 <= len) {
        h ^= xround(0, kv.le64(pos));
        h = rotl64(h, 27) * XP1 + XP4;
        pos += 8;
    }
    if (pos + 4 <= len) {
        h ^= kv.le32(pos) * XP1;
        h = rotl64(h, 23) * XP2 + XP3;
        pos += 4;
    }
    while (pos < len) {
        h ^= (uint64_t)kv.at(pos) * XP5;
        h = rotl64(h, 11) * XP1;
        pos++;
    }
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
}

// a 31-mer held in eight 32-bit registers (byte 31 zero)
__device__ __forceinline__ uint32_t comp4(uint32_t w) {
    // A(0x41)<->T(0x54): xor 0x15, C(0x43)<->G(0x47): xor 0x04; C and G have bit 1 set
    const uint32_t m = (w >> 1) & 0x01010101u;
    return w ^ 0x15151515u ^ (m | (m << 4));
}

__device__ __forceinline__ uint64_t xxh64_31(const uint32_t (&c)[8], uint64_t seed) {
    // public XXH64 spec for len = 31 < 32: 3 x 8 bytes, 1 x 4 bytes, 3 x 1 byte
    uint64_t h = seed + XP5 + 31ull;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint64_t v = (uint64_t)c[2 * i] | ((uint64_t)c[2 * i + 1] << 32);
        h ^= xround(0, v);
        h = rotl64(h, 27) * XP1 + XP4;
    }
    h ^= (uint64_t)c[6] * XP1;
    h = rotl64(h, 23) * XP2 + XP3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        h ^= (uint64_t)((c[7] >> (8 * i)) & 0xFFu) * XP5;
        h = rotl64(h, 11) * XP1;
    }
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
}

// canonical form of a 31-mer of valid bases held in eight dwords (byte 31 zero): c = f or its
// reverse complement (util/query.cpp:143-199)
__device__ __forceinline__ void canon31(const uint32_t (&f)[8], uint32_t (&c)[8]) {
    // reverse complement: B[j] = comp(raw[31 - j]) for the 32-byte block, then drop B[0]
    uint32_t rv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) rv[j] = __builtin_bswap32(comp4(f[7 - j]));
    uint32_t rc[8];
#pragma unroll
    for (int j = 0; j < 7; ++j) rc[j] = (rv[j] >> 8) | (rv[j + 1] << 24);
    rc[7] = rv[7] >> 8;
    // first strict difference among positions 0..14 decides (big-endian compare);
    // the middle base (position 15) is never compared; ties keep the forward k-mer
    bool use_rc = false, decided = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t x = __builtin_bswap32(f[j]), y = __builtin_bswap32(rc[j]);
        if (j == 3) { x >>= 8; y >>= 8; }
        if (!decided && x != y) { use_rc = x > y; decided = true; }
    }
    if (use_rc) {
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = rc[j];
    }
}

__device__ __forceinline__ bool all_acgt(uint32_t w) {
    // (c >> 1) & 3 maps A C G T to 0 1 3 2; v_perm rebuilds the letters from that code
    const uint32_t code = (w >> 1) & 0x03030303u;
    return __builtin_amdgcn_perm(0u, 0x47544341u, code) == w;
}
// The 31-mer at p (any alignment; the text buffer is padded) as eight dwords, byte 31 zero: what xxh64_31 / canon31 take.
__device__ __forceinline__ void load31(const uint8_t* p, uint32_t (&f)[8]) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p - mis);
    uint32_t r[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) r[j] = w[j];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        f[j] = mis == 0 ? r[j] : (uint32_t)(((uint64_t)r[j] | ((uint64_t)r[j + 1] << 32)) >> (8 * mis));
    f[7] &= 0x00FFFFFFu;                      // byte 31 is not part of the 31-mer
}
// ... and whether all of its 31 characters are valid bases
// (the masked top byte of f[7] stands in as an 'A': the character behind the k-mer does not decide on it)
__device__ __forceinline__ bool valid31(const uint32_t (&f)[8]) {
    bool good = all_acgt(f[7] | 0x41000000u);
#pragma unroll
    for (int j = 0; j < 7; ++j) good = good && all_acgt(f[j]);
    return good;
}
// The 31-mer a term is hashed as: f itself, or (canonicalize) the smaller of f and its reverse complement.  What both
// hash_kernel_k31 (hash_kernels.hip) and the scan work-groups that hash their query's terms themselves (kernels.hip: SH)
// hand to xxh64_31.
__device__ __forceinline__ void term31(const uint32_t (&f)[8], bool canonicalize, uint32_t (&c)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) c[t] = f[t];
    if (canonicalize) canon31(f, c);
}

__device__ __forceinline__ bool has_newline(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u;
}

// Where a term's bit goes.  Scattered atomics run at 22-27 G/s on this part whatever their locality
// (they leave the L2 as 32-byte memory-side requests, profiles/r02_atomic_probe.txt) while plain
// byte stores reach 41 G/s and more: in byte-map mode a term stores a byte into its document's
// plane and pack_bytemap_kernel turns the planes of the launch into matrix bits afterwards.
__device__ __forceinline__ void set_term_bit(const BuildArgs& a, uint32_t doc, uint64_t row) {
    if (a.bytemap != nullptr) {
        a.bytemap[(uint64_t)(doc - a.col_base) * a.bm_stride + row] = 1;
    } else {
        const uint64_t byte_in_row = doc >> 3;
        const uint32_t bit = 1u << ((uint32_t)(byte_in_row & 3u) * 8u + (doc & 7u));
        atomicOr(a.matrix + (row * a.row_bytes + byte_in_row) / 4u, bit);
    }
}

}  // namespace cobs_amd
