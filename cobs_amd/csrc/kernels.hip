// cobs_amd/csrc/kernels.hip -- K2 of the COBS query path (gfx950, CDNA4, wave64): row gather + AND over the H hash
// rows + per-document count (+ optional threshold selection, + optional per-tile top-k)
//   (read_from_disk, aggregate_rows reference classic_search.cpp:279-307, compute_counts :643-1022, threshold filter of
//    counts_to_result :127-132).
// Nothing here is translated from the reference: its CPU code gathers rows into a scratch buffer and expands every row
// BYTE into eight counter lanes through a lookup table; at HBM speed that is VALU-bound.  Here each lane owns a 16-byte
// column chunk (128 documents) of the bit-sliced matrix and keeps the per-document counters bit-sliced as well
// ("vertical counters"): NP bit planes per 32-bit column word, updated with a Harley-Seal carry-save adder tree, so a
// gathered row costs ~4.4 VALU ops per 32 documents and the kernel stays on the HBM roofline.
//
// The file holds the device code of scan_kernel, its launch templates, and -- as a translation unit of its own -- the
// plain (FZ = false) instantiations, the LDS-staged ones among them, launch_scan (the scan_has_* predicates it dispatches by are in kernels.hpp).
// scan_findere.hip includes it with COBS_SCAN_FINDERE_UNIT defined and instantiates the findere (FZ = true) kernels, so
// no instantiation exists in both objects.  The device code stays in THIS file because bench.py keys the replay of
// profiles/traffic.json on a hash of kernels.hip and geometry.cpp: the hash has to see the scan kernel.
// (K1 is in hash_kernels.hip, K3 in topk_kernels.hip, construction in build_kernels.hip.)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_types.hpp"
#include "kernels.hpp"
#include "row_table.hpp"     // K1's row-index table: K2's reader
#include "term_hash.hpp"     // load31 .. xxh64_31, fast_mod: the self-hashing instantiations (SH) hash as K1 does
#include "wave_ops.hpp"      // dpp_mov and its control constants, csa, pool_append

namespace cobs_amd {

// ---------------------------------------------------------------------------
// K2: gather + AND + bit-sliced count.
//
// Work-group = (query q, tile of W sixteen-byte column chunks, W = 4..64); its NW
// waves x 64/W lane groups split the query's 8-term blocks round-robin and merge
// their partial plane counters (shuffles inside a wave, LDS across waves) at the
// end.  A lane owns one chunk: 128 documents, held as 4 column words x NP bit planes.

// (the carry-save adder csa -- two v_bitop3_b32 -- is in wave_ops.hpp)

// fold eight gathered row words into planes 0..2 of one column word; returns the
// carry into plane 3 ("eights")
template <int NP>
__device__ __forceinline__ uint32_t absorb8(uint32_t (&pl)[NP], uint32_t x0, uint32_t x1, uint32_t x2,
                                            uint32_t x3, uint32_t x4, uint32_t x5, uint32_t x6,
                                            uint32_t x7) {
    uint32_t t2a, t2b, f4a, f4b, e8;
    csa(t2a, pl[0], pl[0], x0, x1);
    csa(t2b, pl[0], pl[0], x2, x3);
    csa(f4a, pl[1], pl[1], t2a, t2b);
    csa(t2a, pl[0], pl[0], x4, x5);
    csa(t2b, pl[0], pl[0], x6, x7);
    csa(f4b, pl[1], pl[1], t2a, t2b);
    csa(e8, pl[2], pl[2], f4a, f4b);
    return e8;
}

// ripple a carry into planes FROM..NP-1
template <int NP, int FROM>
__device__ __forceinline__ void ripple(uint32_t (&pl)[NP], uint32_t carry) {
#pragma unroll
    for (int k = FROM; k < NP; ++k) {
        const uint32_t t = pl[k] & carry;
        pl[k] ^= carry;
        carry = t;
    }
}

// eights[w] = carry-outs of one 8-row block for the lane's 4 column words
template <int NP>
__device__ __forceinline__ void absorb_block(uint32_t (&pl)[4][NP], const uint4 (&X)[8],
                                             uint32_t (&e8)[4]) {
    e8[0] = absorb8<NP>(pl[0], X[0].x, X[1].x, X[2].x, X[3].x, X[4].x, X[5].x, X[6].x, X[7].x);
    e8[1] = absorb8<NP>(pl[1], X[0].y, X[1].y, X[2].y, X[3].y, X[4].y, X[5].y, X[6].y, X[7].y);
    e8[2] = absorb8<NP>(pl[2], X[0].z, X[1].z, X[2].z, X[3].z, X[4].z, X[5].z, X[6].z, X[7].z);
    e8[3] = absorb8<NP>(pl[3], X[0].w, X[1].w, X[2].w, X[3].w, X[4].w, X[5].w, X[6].w, X[7].w);
}

// one block on its own: its eights go straight into plane 3 and up
template <int NP>
__device__ __forceinline__ void retire_single(uint32_t (&pl)[4][NP], const uint32_t (&e8)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) ripple<NP, 3>(pl[w], e8[w]);
}

// two blocks: add both eights into plane 3 with one more CSA, ripple the sixteens
template <int NP>
__device__ __forceinline__ void retire_pair(uint32_t (&pl)[4][NP], const uint32_t (&ea)[4],
                                            const uint32_t (&eb)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t s16;
        csa(s16, pl[w][3], pl[w][3], ea[w], eb[w]);
        ripple<NP, 4>(pl[w], s16);
    }
}

// Half a block (generic-H row loop, round 6): four row words into planes 0..1 of one column word; the first half
// leaves its carry into plane 2 ("fours") pending, the second half adds both fours into plane 2 and returns the eights.
template <int NP>
__device__ __forceinline__ uint32_t absorb4(uint32_t (&pl)[NP], uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    uint32_t t2a, t2b, f4;
    csa(t2a, pl[0], pl[0], x0, x1);
    csa(t2b, pl[0], pl[0], x2, x3);
    csa(f4, pl[1], pl[1], t2a, t2b);
    return f4;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ uint4 load_row(const uint8_t* lane_base, uint64_t row, uint32_t pitch) {
    const u32x4* p = reinterpret_cast<const u32x4*>(lane_base + row * pitch);
    const u32x4 v = NT ? __builtin_nontemporal_load(p) : *p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Eight row indices of one (block, hash): 32-bit (two 16-byte loads) or, for sub-indexes with
// 2^32 or more rows (signature sizes of human-sized documents), 64-bit (four loads).
template <typename IdxT> struct Idx8;
template <> struct Idx8<uint32_t> { uint4 a, b; };
template <> struct Idx8<uint64_t> { uint4 a, b, c, d; };

__device__ __forceinline__ Idx8<uint32_t> load_idx8(const uint32_t* p) {
    const uint4* t = reinterpret_cast<const uint4*>(p);
    return Idx8<uint32_t>{t[0], t[1]};
}
__device__ __forceinline__ Idx8<uint64_t> load_idx8(const uint64_t* p) {
    const uint4* t = reinterpret_cast<const uint4*>(p);
    return Idx8<uint64_t>{t[0], t[1], t[2], t[3]};
}

template <bool NT>
__device__ __forceinline__ void issue_rows(uint4 (&X)[8], const uint8_t* lane_base, uint32_t pitch,
                                           const Idx8<uint32_t>& i) {
    X[0] = load_row<NT>(lane_base, i.a.x, pitch);
    X[1] = load_row<NT>(lane_base, i.a.y, pitch);
    X[2] = load_row<NT>(lane_base, i.a.z, pitch);
    X[3] = load_row<NT>(lane_base, i.a.w, pitch);
    X[4] = load_row<NT>(lane_base, i.b.x, pitch);
    X[5] = load_row<NT>(lane_base, i.b.y, pitch);
    X[6] = load_row<NT>(lane_base, i.b.z, pitch);
    X[7] = load_row<NT>(lane_base, i.b.w, pitch);
}

template <bool NT>
__device__ __forceinline__ void issue_rows4(uint4 (&X)[4], const uint8_t* lane_base, uint32_t pitch, const uint4& i) {
    X[0] = load_row<NT>(lane_base, i.x, pitch);
    X[1] = load_row<NT>(lane_base, i.y, pitch);
    X[2] = load_row<NT>(lane_base, i.z, pitch);
    X[3] = load_row<NT>(lane_base, i.w, pitch);
}

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)hi << 32 | lo; }

template <bool NT>
__device__ __forceinline__ void issue_rows(uint4 (&X)[8], const uint8_t* lane_base, uint32_t pitch,
                                           const Idx8<uint64_t>& i) {
    X[0] = load_row<NT>(lane_base, u64_of(i.a.x, i.a.y), pitch);
    X[1] = load_row<NT>(lane_base, u64_of(i.a.z, i.a.w), pitch);
    X[2] = load_row<NT>(lane_base, u64_of(i.b.x, i.b.y), pitch);
    X[3] = load_row<NT>(lane_base, u64_of(i.b.z, i.b.w), pitch);
    X[4] = load_row<NT>(lane_base, u64_of(i.c.x, i.c.y), pitch);
    X[5] = load_row<NT>(lane_base, u64_of(i.c.z, i.c.w), pitch);
    X[6] = load_row<NT>(lane_base, u64_of(i.d.x, i.d.y), pitch);
    X[7] = load_row<NT>(lane_base, u64_of(i.d.z, i.d.w), pitch);
}

__device__ __forceinline__ void and_rows(uint4 (&X)[8], const uint4 (&Y)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        X[t].x &= Y[t].x; X[t].y &= Y[t].y; X[t].z &= Y[t].z; X[t].w &= Y[t].w;
    }
}

// ---- findere (FZ instantiations of K2): a position counts only when the z + 1 consecutive terms of its window are all
// present.  Per document a saturating DEFICIT d = max(z - run, 0), run = present terms in a row up to here, bit-sliced
// in three planes (z <= 7) per column word: the window ending at term i is complete iff P_i and d_{i-1} == 0; then
// d_i = P_i ? max(d_{i-1} - 1, 0) : z.  Eight VALU per column word and term (v_bitop3), 12 VGPRs of state per lane.
// d starts at z: terms before position 0 are absent.
struct FzState {
    uint32_t d0[4], d1[4], d2[4];       // deficit planes of the lane's 4 column words
    uint32_t z0, z1, z2;                // z as all-zero / all-one masks per bit (wave-uniform)
};

__device__ __forceinline__ void fz_init(FzState& s, uint32_t z) {
    s.z0 = (z & 1u) ? ~0u : 0u;
    s.z1 = (z & 2u) ? ~0u : 0u;
    s.z2 = (z & 4u) ? ~0u : 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) { s.d0[w] = s.z0; s.d1[w] = s.z1; s.d2[w] = s.z2; }
}

// one term's presence word p of column word w -> its window word
__device__ __forceinline__ uint32_t fz_step(FzState& s, int w, uint32_t p) {
    const uint32_t d0 = s.d0[w], d1 = s.d1[w], d2 = s.d2[w];
    const uint32_t nz = __builtin_amdgcn_bitop3_b32(d0, d1, d2, 0xFE);      // d != 0
    const uint32_t win = __builtin_amdgcn_bitop3_b32(p, nz, nz, 0x30);      // p & ~nz
    // d - 1 saturating at 0: bit 0 = ~d0 & (d1 | d2), bit 1 = d1 ^ (~d0 & (d1 | d2)), bit 2 = d2 & (d0 | d1)
    const uint32_t e0 = __builtin_amdgcn_bitop3_b32(d0, d1, d2, 0x0E);
    const uint32_t e1 = __builtin_amdgcn_bitop3_b32(d0, d1, d2, 0xC2);
    const uint32_t e2 = __builtin_amdgcn_bitop3_b32(d0, d1, d2, 0xA8);
    // present: decremented; absent: z (select p ? e : z)
    s.d0[w] = __builtin_amdgcn_bitop3_b32(p, e0, s.z0, 0xCA);
    s.d1[w] = __builtin_amdgcn_bitop3_b32(p, e1, s.z1, 0xCA);
    s.d2[w] = __builtin_amdgcn_bitop3_b32(p, e2, s.z2, 0xCA);
    return win;
}

// N consecutive terms (in query order) of presence words -> window words, in place
template <int N>
__device__ __forceinline__ void fz_window(FzState& s, uint4 (&X)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t) {
        X[t].x = fz_step(s, 0, X[t].x);
        X[t].y = fz_step(s, 1, X[t].y);
        X[t].z = fz_step(s, 2, X[t].z);
        X[t].w = fz_step(s, 3, X[t].w);
    }
}

// ---- LDS-staged variant of the row pipeline (LDSS): rows travel HBM -> LDS (direct-to-LDS DMA,
// global_load_lds_dwordx4: 64 lanes x 16 B = 1 KiB per instruction) -> VGPR (ds_read_b128)
// instead of HBM -> VGPR.  hipcc neither counts asm memory operations nor pipelines LDS-DMA
// (it would drain it with vmcnt(0)), so the loop's VMEM operations are inline asm with counted
// s_waitcnt vmcnt(N); the waits name the registers they make valid so that the compiler
// cannot touch them earlier.  Kept as a measured A/B against the VGPR-direct pipeline
// (scripts/ab.py ... lds=1; result in profiles/).
__device__ __forceinline__ void asm_load_idx(u32x4& a, u32x4& b, const uint32_t* p) {
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16"
                 : "=&v"(a), "=&v"(b) : "v"(p) : "memory");
}
// one row: the wave's 64 lanes x 16 bytes land at LDS address lds_dst + lane * 16
__device__ __forceinline__ void asm_glds16(const uint8_t* gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds_rows(const uint8_t* lane_base, uint32_t pitch, const u32x4& a, const u32x4& b,
                                          uint32_t lds_dst) {
    asm_glds16(lane_base + (uint64_t)a.x * pitch, lds_dst);
    asm_glds16(lane_base + (uint64_t)a.y * pitch, lds_dst + 1024u);
    asm_glds16(lane_base + (uint64_t)a.z * pitch, lds_dst + 2048u);
    asm_glds16(lane_base + (uint64_t)a.w * pitch, lds_dst + 3072u);
    asm_glds16(lane_base + (uint64_t)b.x * pitch, lds_dst + 4096u);
    asm_glds16(lane_base + (uint64_t)b.y * pitch, lds_dst + 5120u);
    asm_glds16(lane_base + (uint64_t)b.z * pitch, lds_dst + 6144u);
    asm_glds16(lane_base + (uint64_t)b.w * pitch, lds_dst + 7168u);
}
#define COBS_WAIT_VM_IDX(N, A, B) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(A), "+v"(B) : : "memory")
#define COBS_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" : : : "memory")

// Phase timestamps of sampled work-groups (tuning builds only: make -C cobs_amd/csrc timing;
// scripts/phase_times.py).  COBS_STAMP(k) drains the memory queues first so that the time of a
// phase includes the loads it issued.
#ifdef COBS_SCAN_TIMING
#define COBS_STAMP(K)                                                                           \
    do {                                                                                        \
        if (a.dbg && (blockIdx.x % a.dbg_every) == 0u && blockIdx.x / a.dbg_every < a.dbg_slots) { \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                         \
            const uint64_t t_ = __builtin_amdgcn_s_memtime();                                   \
            if (lane == 0u) a.dbg[((uint64_t)(blockIdx.x / a.dbg_every) * 4u + wave) * 8u + (K)] = t_; \
        }                                                                                       \
    } while (0)
#else
#define COBS_STAMP(K) do { } while (0)
#endif

// LDS bytes in front of the expansion table / tile metadata: the merge buffers of the waves
// ([NW/2 (min 1)][NP][64 lanes] of uint4), the row staging ring of the LDS-staged variant, or --
// 8-bit scores -- the score staging buffer of the epilogue, whichever is largest
// (SH: ... or the row indices the work-group hashed for itself, which the merge buffers alias)
template <int NP, int NW, size_t OutBytes, bool LDSS, bool SH = false>
__host__ __device__ constexpr size_t scan_lds_front() {
    size_t f = LDSS ? (size_t)NW * 16384 : (size_t)(NW >= 2 ? NW / 2 : 1) * NP * 64 * sizeof(uint4);
    if (OutBytes == 1 && f < 64 * 144) f = 64 * 144;
    if (SH && f < kSelfHashEntries * sizeof(uint32_t)) f = kSelfHashEntries * sizeof(uint32_t);
    return f;
}

// 32 documents x NP (<= 8) bit planes -> the documents' 8-bit counts, in registers: byte b of every
// plane is gathered with v_perm_b32 (two 4x4 byte transposes), then an 8x8 bit transpose (three
// delta swaps) turns "bit i of byte k = bit k of document 8b+i" into one byte per document.
// out[j] = counts of documents 4j .. 4j+3.  24 VALU per 8 documents, no LDS table.
template <int NP>
__device__ __forceinline__ void planes_to_bytes32(const uint32_t (&P)[NP], uint32_t (&out)[8]) {
    static_assert(NP <= 8, "8-bit scores hold at most 8 planes");
    uint32_t q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = k < NP ? P[k] : 0u;
    uint32_t x[4], y[4];
    {
        const uint32_t t0 = __builtin_amdgcn_perm(q[1], q[0], 0x05010400u), t1 = __builtin_amdgcn_perm(q[1], q[0], 0x07030602u);
        const uint32_t t2 = __builtin_amdgcn_perm(q[3], q[2], 0x05010400u), t3 = __builtin_amdgcn_perm(q[3], q[2], 0x07030602u);
        x[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u); x[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
        x[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u); x[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
    }
    {
        const uint32_t t0 = __builtin_amdgcn_perm(q[5], q[4], 0x05010400u), t1 = __builtin_amdgcn_perm(q[5], q[4], 0x07030602u);
        const uint32_t t2 = __builtin_amdgcn_perm(q[7], q[6], 0x05010400u), t3 = __builtin_amdgcn_perm(q[7], q[6], 0x07030602u);
        y[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u); y[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
        y[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u); y[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t lo = x[b], hi = y[b], t;
        t = (lo ^ (lo >> 7)) & 0x00AA00AAu; lo = lo ^ t ^ (t << 7);
        t = (hi ^ (hi >> 7)) & 0x00AA00AAu; hi = hi ^ t ^ (t << 7);
        t = (lo ^ (lo >> 14)) & 0x0000CCCCu; lo = lo ^ t ^ (t << 14);
        t = (hi ^ (hi >> 14)) & 0x0000CCCCu; hi = hi ^ t ^ (t << 14);
        out[2 * b] = (lo & 0x0F0F0F0Fu) | ((hi << 4) & 0xF0F0F0F0u);
        out[2 * b + 1] = ((lo >> 4) & 0x0F0F0F0Fu) | (hi & 0xF0F0F0F0u);
    }
}
// LDS bytes between the score blocks of two lanes in the staging buffer of the 8-bit epilogue:
// 128 bytes of scores + 16 of padding, so that the 16-byte writes of 16 lanes hit 16 different banks
constexpr uint32_t kStageStride = 144u;

// (cross-lane steps as DPP modifiers of the VALU: dpp_mov and its control constants, wave_ops.hpp)

// sum of `c` over the W (power of two, 4..64) consecutive lanes of a lane group, in every lane of the group
__device__ __forceinline__ uint32_t group_allsum(uint32_t c, uint32_t W) {
    c += dpp_mov<kDppQuadXor1>(c);
    c += dpp_mov<kDppQuadXor2>(c);                      // every lane: the sum of its quad
    if (W >= 8u) c += dpp_mov<kDppHalfMirror>(c);       // + the other quad of the half row
    if (W >= 16u) c += dpp_mov<kDppRowMirror>(c);       // + the other half of the row
    if (W >= 32u) c += (uint32_t)__shfl_xor(c, 16);
    if (W >= 64u) c += (uint32_t)__shfl_xor(c, 32);
    return c;
}

// inclusive prefix sum of `v` over the lanes of a lane group (col = lane inside the group)
__device__ __forceinline__ uint32_t group_incl_scan(uint32_t v, uint32_t W, uint32_t col) {
    uint32_t t;
    t = dpp_mov<kDppRowShr + 1>(v); v += col >= 1u ? t : 0u;
    t = dpp_mov<kDppRowShr + 2>(v); v += col >= 2u ? t : 0u;
    if (W >= 8u) { t = dpp_mov<kDppRowShr + 4>(v); v += col >= 4u ? t : 0u; }
    if (W >= 16u) { t = dpp_mov<kDppRowShr + 8>(v); v += col >= 8u ? t : 0u; }
    // (the row steps stop at row boundaries: what crosses them is the TOTAL of the rows before)
    if (W >= 32u) v += dpp_mov<kDppBcast15, 0xA, 0xF, false>(v);      // rows 1 and 3 += lane 15 of the row before
    if (W >= 64u) v += dpp_mov<kDppBcast31, 0xC, 0xF, false>(v);      // rows 2 and 3 += lane 31 (complete after the step above)
    return v;
}

// Exact top-k of ONE tile, straight from the bit-sliced counters (run_topk without score rows): the k best
// documents of a tile under (score desc, document asc) are a superset of the tile's share of the query's k
// best (counts_to_result's partial_sort, classic_search.cpp:134-145), so K3 only has to merge tiles x k
// candidates instead of reading a score row per query twice.  Radix descent over the planes, highest first,
// on the candidate masks M (128 documents per lane): c = documents of M with the plane's bit set, summed over
// the tile with a butterfly; c >= k_rem -> the k_rem best all have the bit: M &= plane; else those c
// documents are in for sure (R |= ...), k_rem -= c, M &= ~plane.  What is left in M ties at the cut score:
// the first k_rem in document order (lane = chunk order, then word, then bit) join R.  All in registers of
// wave 0, NP rounds of ~12 VALU + log2(W) cross-lane adds; the LUT expansion and the score stores are not run.
template <int NP, bool MQ>
__device__ __forceinline__ void tile_topk(const ScanArgs& a, const uint32_t (&pl)[4][NP], uint32_t lane, uint32_t W,
                                          uint32_t tile, uint32_t qi, const uint32_t* tmeta, const uint32_t* tthr) {
    const uint32_t G = 64u / W;
    const uint32_t col = lane & (W - 1u), grp = lane / W;
    const uint32_t qraw = MQ ? qi * G + grp : qi;
    const bool live = (MQ || lane < W) && qraw < a.nq;            // lanes that hold the final planes of a real query
    const uint32_t q = qraw < a.nq ? qraw : a.nq - 1u;
    const uint32_t doc0 = tmeta[col * 3 + 2];
    uint32_t nvalid = live ? tmeta[col * 3 + 1] * 8u : 0u;         // row bytes inside the page ...
    nvalid = min(nvalid, a.num_docs > doc0 ? a.num_docs - doc0 : 0u);   // ... that belong to real documents
    const uint32_t thr = a.thresholds ? tthr[MQ ? grp : 0u] : 0u;
    uint32_t M[4], R[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t nw_ = nvalid > 32u * w ? min(nvalid - 32u * w, 32u) : 0u;
        uint32_t v = nw_ >= 32u ? 0xFFFFFFFFu : (1u << nw_) - 1u;
        if (a.thresholds) {      // count >= threshold on the planes (as the hits-only epilogue does)
            uint32_t ge = (NP < 32 && (thr >> (NP < 32 ? NP : 0)) != 0u) ? 0u : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < NP; ++k) ge = ((thr >> k) & 1u) ? (ge & pl[w][k]) : (ge | pl[w][k]);
            v &= ge;
        }
        M[w] = v;
        R[w] = 0u;
    }
    uint32_t krem = a.topk_k;
#pragma unroll
    for (int p = NP - 1; p >= 0; --p) {
        uint32_t A[4], c = 0u;
#pragma unroll
        for (int w = 0; w < 4; ++w) { A[w] = M[w] & pl[w][p]; c += (uint32_t)__popc(A[w]); }
        c = group_allsum(c, W);
        const bool take = c >= krem;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            R[w] |= take ? 0u : A[w];
            M[w] = take ? A[w] : (M[w] & ~pl[w][p]);
        }
        krem -= take ? 0u : c;
    }
    auto group_excl = [&](uint32_t v, uint32_t* total) {
        const uint32_t incl = group_incl_scan(v, W, col);
        *total = __shfl(incl, lane | (W - 1u));
        return incl - v;
    };
    {   // ties at the cut score: the first krem of M in document order
        uint32_t cm = 0u, tot;
#pragma unroll
        for (int w = 0; w < 4; ++w) cm += (uint32_t)__popc(M[w]);
        uint32_t before = group_excl(cm, &tot);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t pc = (uint32_t)__popc(M[w]);
            const uint32_t allow = krem > before ? krem - before : 0u;
            uint32_t x = M[w];
            if (allow < pc) {
                uint32_t y = x;
                for (uint32_t i = 0; i < allow; ++i) y &= y - 1u;          // y = x without its lowest `allow` bits
                x &= ~y;
            }
            R[w] |= x;
            before += pc;
        }
    }
    uint32_t cs = 0u, total;
#pragma unroll
    for (int w = 0; w < 4; ++w) cs += (uint32_t)__popc(R[w]);
    uint32_t pos = group_excl(cs, &total);
    uint2* dst = a.cand + (uint64_t)q * a.cand_stride + (uint64_t)(a.tile_base + tile) * a.topk_k;
    if (live) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t x = R[w];
            while (x != 0u) {
                const uint32_t d = (uint32_t)__ffs((int)x) - 1u;
                x &= x - 1u;
                uint32_t score = 0u;
#pragma unroll
                for (int k = 0; k < NP; ++k) score |= ((pl[w][k] >> d) & 1u) << k;
                dst[pos++] = make_uint2(doc0 + 32u * w + d, score);
            }
        }
        // entries the tile does not fill are marked (K3 skips them); the pool needs no clearing between runs
        for (uint32_t i = total + col; i < a.topk_k; i += W) dst[i] = make_uint2(0xFFFFFFFFu, 0u);
    }
}

// scan_kernel is ONE body on purpose.  Its stages were tried as __device__ __forceinline__ functions (the tile setup as a
// struct, the trip count, the findere priming, each row loop, the two merges, each epilogue) and every one of them moved
// the compiler's schedule: the row loops cost scan_kernel<8, 1, false, u8, false, u32> 29 spills (116 -> 128 VGPRs) and
// its findere twin a wave per SIMD; the tile struct moved AGPRs in <20|24|32, 4, false, u32, false, u32, false, false,
// true> and took <10, 1, true, u16, false, u32, false, true, true> from 136 to 138 VGPRs; the epilogues added 55
// instructions to the four-wave multi-query kernels; the LDS-staged loop lost 47.  With all of them inline the code
// object is instruction for instruction the one of the single-file version (profiles/scan_split_isa_diff.txt).  Only
// the hit pool's append (pool_append, wave_ops.hpp) is shared: it compiles to the same instructions.
// MQ ("multi-query", short queries): the G = 64 / W lane groups of a wave belong to G
// DIFFERENT queries (q = qi*G + grp) instead of splitting one query's blocks.  Every lane
// group then walks all blocks of its own query (divided over the NW waves only): G times
// more trips per wave, so the load pipeline reaches its steady state even for 100-bp reads,
// and the cross-lane merge disappears.
// TK: the epilogue is tile_topk (run_topk without score rows) instead of the score / hit epilogues -- its own
// instantiations, so that the kernels that write scores keep their register budget (as a run-time branch
// it cost the 100-bp multi-query kernel its fourth wave per SIMD: 126 -> 131 VGPRs).
// (the tile_topk instantiations of up to 10 planes are held to the 128 VGPRs of four waves per SIMD, like the
// kernels whose epilogue they replace: the selection's masks would otherwise cost the multi-query ones a wave;
// so are the generic-H instantiations of one and two waves per group, whose half-block row loop fits them -- the
// four-wave one would spill in that loop and is left to the compiler: geometry.cpp does not choose it)
// FZ: findere (ScanArgs::findere = z > 0) -- every term's presence words become window words (fz_window) before the
// counter tree, and a virtual wave walks a CONTIGUOUS range of the query's blocks, primed with the z terms in front of
// it (loaded, not counted).  Left to the compiler's register budget (the deficit planes cost 12 VGPRs).
// SH: self-hashing (ScanArgs::self_hash; H = 1, 31-mers, 32-bit indices, one query per group, score / hit epilogues).  There is
// no table from K1: during set-up the NW * 64 threads hash the query's terms -- load31, canon31, xxh64_31, fast_mod, K1's
// own device functions (term_hash.hpp) -- once per term, and reduce the hash by the signature size of EVERY sub-index the
// tile's chunks lie in (usually one; a narrow page under a wide tile: several) into an LDS array [sub-index][block + padding
// block][8].  An invalid term (invalid_bases != 0) and the padding terms name the zero row, as in K1's table.  The row loop
// takes its two Idx8 reads per trip from LDS: LDS index read | 8 row loads | CSA, the VMEM queue holds row loads only (the
// compiler counts them).  The array aliases the merge buffers, so a barrier separates the row loop from the merge.  Tile 0 of
// a launch with ScanArgs::record set reports what K1 reports: the first query with an invalid base, the valid positions.
template <int NP, int NW, bool H1, typename OutT, bool MQ, typename IdxT, bool LDSS = false, bool TK = false, bool FZ = false,
          bool SH = false>
__global__ __launch_bounds__(NW * 64, (!FZ && (SH || (TK && H1) || (!H1 && sizeof(IdxT) == 4 && !LDSS && (NW <= 2 || TK))) && NP <= 10) ? 4 : 1) void scan_kernel(ScanArgs a) {
    static_assert(!(FZ && LDSS), "findere: no LDS-staged variant");
    static_assert(!SH || (H1 && !MQ && !LDSS && !TK && !FZ && sizeof(IdxT) == 4), "self-hashing: H = 1, one query per group, 32-bit indices, score / hit epilogues");
    // row loads stay temporal: non-temporal loads measured 18 % slower (they bypass the Infinity Cache)
    constexpr bool NT = false;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // merge buffers: [NW/2 (min 1)][NP][64 lanes] of uint4, then the 256-entry expansion table.
    // LDSS: the front of the buffer is the row staging ring (2 x 8 KiB per wave); the merge
    // buffers, needed only after the row loop, alias it.
    constexpr size_t kFront = scan_lds_front<NP, NW, sizeof(OutT), LDSS, SH>();
    static_assert(!LDSS || kFront >= (size_t)(NW >= 2 ? NW / 2 : 1) * NP * 64 * sizeof(uint4), "ring holds the merge buffers");
    uint4* mbuf = reinterpret_cast<uint4*>(smem);
    // 16/32-bit scores expand their planes through a 256-entry table; 8-bit scores transpose in
    // registers (planes_to_bytes32) and have no table
    constexpr size_t kLut = sizeof(OutT) == 1 ? 0 : 256 * sizeof(uint4);
    uint4* lut = reinterpret_cast<uint4*>(smem + kFront);
    // per-chunk metadata of this tile (first local score slot, valid row bytes left in the
    // chunk, first document id) and per-lane-group thresholds: the epilogue reads them from
    // LDS instead of chasing a.pages[] / a.thresholds[] through global memory per iteration
    uint32_t* tmeta = reinterpret_cast<uint32_t*>(smem + kFront + kLut);   // [64][3]
    uint32_t* tthr = tmeta + 64 * 3;                                 // [64]
    if constexpr (sizeof(OutT) != 1 && !TK) {
        for (uint32_t v = threadIdx.x; v < 256u; v += NW * 64) {
            uint4 e;
            e.x = (v & 1u) | ((v & 2u) << 15);
            e.y = ((v >> 2) & 1u) | ((v & 8u) << 13);
            e.z = ((v >> 4) & 1u) | ((v & 32u) << 11);
            e.w = ((v >> 6) & 1u) | ((v & 128u) << 9);
            lut[v] = e;
        }
    }

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    COBS_STAMP(0);
    // A tile is W (power of two, <= 64) sixteen-byte column chunks of the chunk range
    // [chunk_begin, chunk_end).  With W < 64 one wave-load fetches G = 64 / W different
    // rows (terms): lane group g of wave w acts as "virtual wave" w*G + g with its own
    // stream of 8-term blocks.  Narrow tiles keep the slice of a small sub-index that
    // all queries of the batch hammer (rows x W*16 bytes) inside the 256 MB Infinity
    // Cache, and they fill the lanes when the whole index is narrower than a wave.
    const uint32_t W = a.tile_w;
    const uint32_t G = 64u / W;
    const uint32_t ntiles = (a.chunk_end - a.chunk_begin + W - 1u) / W;
    (void)ntiles;
    // tile-major order: co-resident groups read the same sub-index columns (query-major: 13 % slower)
    const uint32_t nqg = MQ ? (a.nq + G - 1u) / G : a.nq;         // query groups per tile
    const uint32_t tile = blockIdx.x / nqg;
    const uint32_t qi = blockIdx.x - tile * nqg;
    const uint32_t grp = lane / W, col = lane & (W - 1u);
    // MQ: per-lane query (groups past the end of the batch idle on the padding block)
    const uint32_t qraw = MQ ? qi * G + grp : qi;
    const bool qlive = qraw < a.nq;
    const uint32_t q = qlive ? qraw : a.nq - 1u;
    if (a.thresholds && wave == 0u && col == 0u) tthr[MQ ? grp : 0u] = a.thresholds[q];
    const uint32_t g = a.chunk_begin + tile * W + col;
    const uint32_t gc = g < a.chunk_end ? g : a.chunk_end - 1u;     // dead lanes duplicate a live one
    const uint32_t pg = gc / a.cpp;
    const uint32_t ch = gc - pg * a.cpp;
    const PageDev pdl = a.pages[pg];
    const uint8_t* lane_base = a.blob + pdl.base + (uint64_t)ch * 16u;
    const uint32_t pitch = a.pitch;
    if (threadIdx.x < W) {        // wave 0, lane group 0: one lane per chunk of the tile
        const uint32_t vb = (g < a.chunk_end && pdl.valid_bytes > ch * 16u) ? min(pdl.valid_bytes - ch * 16u, 16u) : 0u;
        tmeta[col * 3 + 0] = pdl.slot0 + ch * 128u;
        tmeta[col * 3 + 1] = vb;
        tmeta[col * 3 + 2] = pdl.doc0 + ch * 128u;
    }

    const uint32_t H = H1 ? 1u : a.num_hashes;
    // row indices of this lane's sub-index (row_table.hpp): [nblk + 1 blocks][hash][8]; block nblk is all padding
    const RowTable<IdxT> rt(a.table, a.blk_off, a.table_npages, q, pdl.tpage, H);
    const uint32_t nblk_q = rt.nblk;                             // table stride of query q
    const uint32_t nblk = qlive ? nblk_q : 0u;
    // (the loops below walk blocks from this pointer with their own offsets, b * 8 * H: rt.block(b), spelled out where
    // the software-pipelined loads take raw addresses)
    const IdxT* tab = rt.base;
    const uint32_t* sidx = nullptr;                              // SH: this lane's sub-index in the LDS array
    if constexpr (SH) {
        // (nothing is read through `tab`: the block count above is all this form takes from K1's bookkeeping)
        // the query's terms, hashed here: [sub-index of the tile][nblk_q + 1 blocks][8] in LDS
        uint32_t* const sh = reinterpret_cast<uint32_t*>(smem);
        const uint32_t len = a.q_len[q];
        const uint32_t T = len - 30u;                            // (31-mers; the host refuses shorter queries): nblk_q = ceil(T / 8)
        const uint32_t stride = (nblk_q + 1u) * 8u;
        const uint32_t c0 = a.chunk_begin + tile * W;
        const uint32_t pg0 = c0 / a.cpp, pg1 = (min(c0 + W, a.chunk_end) - 1u) / a.cpp;      // sub-indexes of the tile
        // (launch_scan refuses this form where the array does not hold every tile's indices -- scan_self_hash_fits,
        // kernels.hpp --, so this never holds for a launched grid; it keeps the writes below inside the array)
        if ((pg1 - pg0 + 1u) * stride > kSelfHashEntries) return;
        const uint8_t* text = a.text + a.span_off[q];
        const bool canon = a.canonicalize != 0;
        const bool lenient = canon && a.invalid_bases != 0;
        const bool rec = a.record != 0u && tile == 0u;
        uint32_t nvalid = 0u;
        bool bad = false;
        for (uint32_t i = threadIdx.x; i < stride; i += NW * 64) {
            bool ok = i < T;
            uint64_t h = 0;
            if (ok) {
                uint32_t f[8];
                load31(text + i, f);
                if (lenient || (rec && canon)) {
                    const bool good = valid31(f);
                    if (lenient) { ok = good; nvalid += good ? 1u : 0u; } else bad = bad || !good;
                }
                if (ok) {
                    uint32_t c[8];
                    term31(f, canon, c);
                    h = xxh64_31(c, 0);
                }
            }
            for (uint32_t sp = pg0; sp <= pg1; ++sp) {
                const uint64_t sig = a.pages[sp].sig;
                sh[(sp - pg0) * stride + i] = ok ? (uint32_t)fast_mod(h, sig, a.pages[sp].magic) : (uint32_t)sig;
            }
        }
        if (rec) {
            // every character of a query lies in some term: a query holds an invalid character iff one of its terms does
            if (bad) atomicMax(a.err_query, 0xFFFFFFFFu - q);
            if (lenient && a.valid != nullptr && nvalid != 0u) atomicAdd(a.valid + q, nvalid);
        }
        __syncthreads();
        sidx = sh + (pg - pg0) * stride;
    }
    const uint32_t vw = MQ ? wave : wave * G + grp;  // virtual wave of this lane
    const uint32_t NV = MQ ? (uint32_t)NW : NW * G;
    // findere: blocks [fz_first, fz_first + fz_per) of the query (a sliding window needs its terms in order)
    const uint32_t fz_per = FZ ? (nblk + NV - 1u) / NV : 0u;
    const uint32_t fz_first = FZ ? vw * fz_per : 0u;
    // block of this lane in trip i: vw + i * NV (findere: fz_first + i), or the padding block when it has run out
    auto blk_of = [&](uint32_t i) -> uint64_t {
        const uint32_t bidx = FZ ? (i < fz_per ? fz_first + i : nblk) : vw + i * NV;
        return (uint64_t)(bidx < nblk ? bidx : nblk_q) * 8u * H;
    };

    uint32_t pl[4][NP];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[w][k] = 0u;

    // trips of this wave (wave-uniform): as many as its first lane group needs
    uint32_t nw;
    if constexpr (MQ) {
        // the longest query among the wave's lane groups sets the trip count
        uint32_t need = FZ ? (nblk > fz_first ? min(nblk - fz_first, fz_per) : 0u)
                           : nblk > wave ? (nblk - wave + NW - 1u) / NW : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) need = max(need, (uint32_t)__shfl_xor(need, off));
        nw = __builtin_amdgcn_readfirstlane(need);
    } else if constexpr (FZ) {
        // the wave's first lane group has the first (and longest) of its ranges
        const uint32_t first = wave * G * fz_per;
        nw = __builtin_amdgcn_readfirstlane(nblk > first ? min(nblk - first, fz_per) : 0u);
    } else {
        const uint32_t first = wave * G;
        nw = nblk > first ? (nblk - first + NV - 1u) / NV : 0u;
    }
    uint32_t ea[4], eb[4];
    FzState fz;
    if constexpr (FZ) {
        fz_init(fz, a.findere);
        // prime the deficit with the z terms in front of the range: the last z terms of block fz_first - 1
        // (z <= 7 < 8), loaded and not counted; the deficit after them does not depend on what came before
        if (fz_first > 0u && fz_first < nblk) {
            const IdxT* pt = tab + (uint64_t)(fz_first - 1u) * 8u * H;
            for (uint32_t t = 8u - a.findere; t < 8u; ++t) {
                uint4 P[1];
                P[0] = load_row<NT>(lane_base, (uint64_t)pt[t], pitch);
                for (uint32_t j = 1; j < H; ++j) {
                    const uint4 r = load_row<NT>(lane_base, (uint64_t)pt[8u * j + t], pitch);
                    P[0].x &= r.x; P[0].y &= r.y; P[0].z &= r.z; P[0].w &= r.w;
                }
                fz_window<1>(fz, P);
            }
        }
    }
    COBS_STAMP(1);                 // page / block-offset loads done, LUT written
    if constexpr (LDSS) {
        static_assert(!LDSS || (H1 && !MQ && sizeof(IdxT) == 4), "LDS-staged variant: H = 1, one query per group, 32-bit indices");
        const uint32_t* tab32 = reinterpret_cast<const uint32_t*>(tab);
        // LDS byte address of this wave's ring (wave-uniform: it goes into M0)
        const uint32_t ring = __builtin_amdgcn_readfirstlane(
            (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem + wave * 16384u);
        const uint8_t* my = smem + wave * 16384u + lane * 16u;          // this lane's 16 bytes of row 0, buffer 0
        auto read_rows = [&](uint4 (&X)[8], uint32_t buf) {
#pragma unroll
            for (int r = 0; r < 8; ++r) X[r] = *reinterpret_cast<const uint4*>(my + buf * 8192u + r * 1024u);
        };
        if (nw > 0) {
            // VMEM queue, oldest first, at the top of step i: idx(i+1) [2 ops] | rows(i) [8 ops].
            // A step loads idx(i+2), waits for idx(i+1), issues rows(i+1) into the other buffer, and
            // only then waits for rows(i): two trips (16 KiB per wave) are in flight at every wait.
            u32x4 pa, pb, qa, qb;              // two index register sets used alternately (no copies)
            uint4 X[8];
            asm_load_idx(pa, pb, tab32 + blk_of(0));
            asm_load_idx(qa, qb, tab32 + blk_of(1));
            COBS_WAIT_VM_IDX(2, pa, pb);
            glds_rows(lane_base, pitch, pa, pb, ring);
            uint32_t i = 0;
            for (; i + 2 < nw; i += 2) {
                asm_load_idx(pa, pb, tab32 + blk_of(i + 2));
                COBS_WAIT_VM_IDX(10, qa, qb);
                glds_rows(lane_base, pitch, qa, qb, ring + 8192u);
                COBS_WAIT_VM(10);
                read_rows(X, 0u);
                absorb_block<NP>(pl, X, ea);
                asm_load_idx(qa, qb, tab32 + blk_of(i + 3));
                COBS_WAIT_VM_IDX(10, pa, pb);
                glds_rows(lane_base, pitch, pa, pb, ring);
                COBS_WAIT_VM(10);
                read_rows(X, 1u);
                absorb_block<NP>(pl, X, eb);
                retire_pair<NP>(pl, ea, eb);
            }
            // queue: idx(i+1) in (qa, qb) | rows(i) in buffer 0; one or two trips left
            if (i + 1 < nw) {
                COBS_WAIT_VM_IDX(8, qa, qb);
                glds_rows(lane_base, pitch, qa, qb, ring + 8192u);
                COBS_WAIT_VM(8);
                read_rows(X, 0u);
                absorb_block<NP>(pl, X, ea);
                COBS_WAIT_VM(0);
                read_rows(X, 1u);
                absorb_block<NP>(pl, X, eb);
                retire_pair<NP>(pl, ea, eb);
            } else {
                COBS_WAIT_VM_IDX(0, qa, qb);
                read_rows(X, 0u);
                absorb_block<NP>(pl, X, ea);
                retire_single<NP>(pl, ea);
            }
        }
        __syncthreads();                   // the merge buffers alias the rings: every wave is done reading
    } else if constexpr (SH) {
        // The H = 1 pipeline below with the row indices read from the LDS array: LDS index read and row loads of trip i+1 |
        // CSA of trip i.  The VMEM queue holds row loads only, 8..16 of them at every wait (the compiler counts them).
        auto lds_idx8 = [&](uint32_t i) {
            const uint32_t bidx = vw + i * NV;
            const uint4* t = reinterpret_cast<const uint4*>(sidx + (bidx < nblk ? bidx : nblk_q) * 8u);
            return Idx8<uint32_t>{t[0], t[1]};
        };
        if (nw > 0) {
            uint4 XA[8], XB[8];
            // (the indices of a trip are read right where its rows are issued: a prefetched set, as the table path keeps,
            // put these instantiations at 134 VGPRs -- three waves per SIMD --, or at 128 with 9 spills in this loop;
            // read in place they take 121 and no scratch.  The LDS read is short beside the 8 row loads in flight.)
            issue_rows<NT>(XA, lane_base, pitch, lds_idx8(0));
            uint32_t i = 0;
            for (; i + 2 < nw; i += 2) {
                // XA in flight = trip i
                issue_rows<NT>(XB, lane_base, pitch, lds_idx8(i + 1));
                absorb_block<NP>(pl, XA, ea);
                issue_rows<NT>(XA, lane_base, pitch, lds_idx8(i + 2));
                absorb_block<NP>(pl, XB, eb);
                retire_pair<NP>(pl, ea, eb);
            }
            if (i + 1 < nw) {
                issue_rows<NT>(XB, lane_base, pitch, lds_idx8(i + 1));
                absorb_block<NP>(pl, XA, ea);
                absorb_block<NP>(pl, XB, eb);
                retire_pair<NP>(pl, ea, eb);
            } else {
                absorb_block<NP>(pl, XA, ea);
                retire_single<NP>(pl, ea);
            }
        }
        __syncthreads();                   // the merge buffers alias the index array: every wave is done reading
    } else if constexpr (H1) {
        // Three-stage software pipeline, branch-free in the steady state:
        //   row indices of trip i+2 | row loads of trip i+1 | CSA of trip i
        // so that 8..16 row loads (8..16 KiB per wave) are always in flight.
        if (nw > 0) {
            uint4 XA[8], XB[8];
            Idx8<IdxT> i0 = load_idx8(tab + blk_of(0));
            COBS_STAMP(2);         // first row indices landed
            issue_rows<NT>(XA, lane_base, pitch, i0);
            // (requesting the second index set before the first rows -- one dependent round trip less at the start --
            // measured equal on 50 / 100-bp reads and C3 and 1.4 % slower on 150-bp reads, round 3: occupancy hides it)
            Idx8<IdxT> i1 = load_idx8(tab + blk_of(1));
            COBS_STAMP(3);         // first rows landed
            uint32_t i = 0;
            for (; i + 2 < nw; i += 2) {
                // XA in flight = trip i, i1 = indices of trip i+1
                i0 = load_idx8(tab + blk_of(i + 2));
                issue_rows<NT>(XB, lane_base, pitch, i1);
                if constexpr (FZ) fz_window<8>(fz, XA);
                absorb_block<NP>(pl, XA, ea);
                i1 = load_idx8(tab + blk_of(i + 3));
                issue_rows<NT>(XA, lane_base, pitch, i0);
                if constexpr (FZ) fz_window<8>(fz, XB);
                absorb_block<NP>(pl, XB, eb);
                retire_pair<NP>(pl, ea, eb);
            }
            // XA in flight = trip i; one or two trips left
            if (i + 1 < nw) {
                issue_rows<NT>(XB, lane_base, pitch, i1);
                if constexpr (FZ) fz_window<8>(fz, XA);
                absorb_block<NP>(pl, XA, ea);
                if constexpr (FZ) fz_window<8>(fz, XB);
                absorb_block<NP>(pl, XB, eb);
                retire_pair<NP>(pl, ea, eb);
            } else {
                if constexpr (FZ) fz_window<8>(fz, XA);
                absorb_block<NP>(pl, XA, ea);
                retire_single<NP>(pl, ea);
            }
        }
    } else if constexpr (sizeof(IdxT) == 4) {
        // general H (aggregate_rows, reference classic_search.cpp:279-307: AND the H hash rows of each term, then count),
        // 32-bit row indices -- in HALF blocks of four terms (round 6).  Whole blocks kept three 8-row register sets live
        // (two in flight + the AND accumulator: 96 VGPRs beside 40 of planes), 189-215 VGPRs, two waves per SIMD; with
        // four-row sets (48 VGPRs) these instantiations fit the 128 VGPRs of FOUR waves per SIMD like the H = 1 kernels:
        // the same row bytes in flight per SIMD, twice the waves to hide a gather's latency behind.  The (block, half,
        // hash) triples of a wave form one stream of sub-trips through the usual three-stage pipeline -- row indices of
        // sub-trip s+2 | row loads of s+1 | AND / CSA of s; a block's first half folds into planes 0..1 and leaves its
        // fours pending, the second half adds both fours into plane 2 and ripples the eights.
        if (nw > 0) {
            uint4 XA[4], XB[4], ACC[4];
            uint32_t f4a[4] = {0u, 0u, 0u, 0u};
            const uint32_t total = nw * H * 2u;        // (even: the pipeline below always ends on a pair)
            uint32_t li = 0, lh = 0, lj = 0;           // (trip, half, hash) of the next index load
            auto next_idx = [&]() -> uint4 {           // trips >= nw point at the padding block
                const uint4 r = *reinterpret_cast<const uint4*>(tab + blk_of(li) + 8u * lj + 4u * lh);
                if (++lj == H) { lj = 0; if (++lh == 2u) { lh = 0; ++li; } }
                return r;
            };
            uint32_t cj = 0, ch = 0;                   // hash / half of the sub-trip being consumed
            auto consume = [&](const uint4 (&X)[4]) {
                if (cj == 0) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) ACC[t] = X[t];
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) { ACC[t].x &= X[t].x; ACC[t].y &= X[t].y; ACC[t].z &= X[t].z; ACC[t].w &= X[t].w; }
                }
                if (++cj == H) {
                    cj = 0;
                    if constexpr (FZ) fz_window<4>(fz, ACC);
                    const uint32_t g0 = absorb4<NP>(pl[0], ACC[0].x, ACC[1].x, ACC[2].x, ACC[3].x);
                    const uint32_t g1 = absorb4<NP>(pl[1], ACC[0].y, ACC[1].y, ACC[2].y, ACC[3].y);
                    const uint32_t g2 = absorb4<NP>(pl[2], ACC[0].z, ACC[1].z, ACC[2].z, ACC[3].z);
                    const uint32_t g3 = absorb4<NP>(pl[3], ACC[0].w, ACC[1].w, ACC[2].w, ACC[3].w);
                    if (ch == 0u) {
                        f4a[0] = g0; f4a[1] = g1; f4a[2] = g2; f4a[3] = g3;
                        ch = 1u;
                    } else {
                        const uint32_t g[4] = {g0, g1, g2, g3};
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            uint32_t e8;
                            csa(e8, pl[w][2], pl[w][2], f4a[w], g[w]);
                            ripple<NP, 3>(pl[w], e8);
                        }
                        ch = 0u;
                    }
                }
            };
            uint4 i0 = next_idx();
            issue_rows4<NT>(XA, lane_base, pitch, i0);
            uint4 i1 = next_idx();
            uint32_t sidx = 0;
            for (; sidx + 2 < total; sidx += 2) {
                i0 = next_idx();
                issue_rows4<NT>(XB, lane_base, pitch, i1);
                consume(XA);
                i1 = next_idx();
                issue_rows4<NT>(XA, lane_base, pitch, i0);
                consume(XB);
            }
            issue_rows4<NT>(XB, lane_base, pitch, i1);
            consume(XA);
            consume(XB);
        }
    } else {
        // general H, 64-bit row indices (a sub-index of 2^32 - 1 rows or more): whole blocks.
        // The (block, hash) pairs of a wave form one stream of "sub-trips" that runs through the
        // same three-stage pipeline as the H = 1 loop -- row indices of sub-trip s+2 | row loads of
        // s+1 | AND / CSA of s -- so that 8..16 rows are always in flight (the first version
        // issued a block's rows only after the previous block had been counted).
        if (nw > 0) {
            uint4 XA[8], XB[8], ACC[8];
            const uint32_t total = nw * H;
            uint32_t li = 0, lj = 0;                   // (trip, hash) of the next index load
            auto next_idx = [&]() {
                const Idx8<IdxT> r = load_idx8(tab + blk_of(li) + 8u * lj);     // trips >= nw point at the padding block
                if (++lj == H) { lj = 0; ++li; }
                return r;
            };
            uint32_t cj = 0;                           // hash of the sub-trip being consumed
            auto consume = [&](const uint4 (&X)[8]) {
                if (cj == 0) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) ACC[t] = X[t];
                } else {
                    and_rows(ACC, X);
                }
                if (++cj == H) {
                    cj = 0;
                    if constexpr (FZ) fz_window<8>(fz, ACC);
                    absorb_block<NP>(pl, ACC, ea);
                    retire_single<NP>(pl, ea);
                }
            };
            Idx8<IdxT> i0 = next_idx();
            issue_rows<NT>(XA, lane_base, pitch, i0);
            Idx8<IdxT> i1 = next_idx();
            uint32_t sidx = 0;
            for (; sidx + 2 < total; sidx += 2) {
                i0 = next_idx();
                issue_rows<NT>(XB, lane_base, pitch, i1);
                consume(XA);
                i1 = next_idx();
                issue_rows<NT>(XA, lane_base, pitch, i0);
                consume(XB);
            }
            if (sidx + 1 < total) {
                issue_rows<NT>(XB, lane_base, pitch, i1);
                consume(XA);
                consume(XB);
            } else {
                consume(XA);
            }
        }
    }

    COBS_STAMP(4);                 // row loop done
    // ---- merge the G lane groups of this wave (bit-sliced adds across lanes)
    for (uint32_t s = MQ ? 64u : W; s < 64u; s <<= 1) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t carry = 0u;
#pragma unroll
            for (int kk = 0; kk < NP; ++kk) {
                const uint32_t o = __shfl_down(pl[w][kk], s);
                uint32_t h;
                csa(h, pl[w][kk], pl[w][kk], o, carry);
                carry = h;
            }
        }
    }

    // ---- merge the NW partial counters (tree over waves, bit-sliced adds) ----
#pragma unroll
    for (int s = 1; s < NW; s <<= 1) {
        uint4* buf = mbuf + (size_t)(wave / (2 * s)) * NP * 64;
        if ((wave & (2 * s - 1)) == (uint32_t)s) {
#pragma unroll
            for (int k = 0; k < NP; ++k)
                buf[k * 64 + lane] = make_uint4(pl[0][k], pl[1][k], pl[2][k], pl[3][k]);
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
    if constexpr (TK) {
        // run_topk without score rows: wave 0 holds the final planes and selects the tile's k best from them
        __syncthreads();                 // tile metadata / thresholds written at the start are read below (NW = 1: no barrier so far)
        // (the lane number is taken afresh from the hardware: keeping threadIdx-derived values alive across the row loop
        // is what pushed the 8-plane multi-query instantiation over its 128 registers -- 3 spills, the library's only
        // scratch user in round 3)
        if (wave == 0u)
            tile_topk<NP, MQ>(a, pl, __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), W, tile, qi, tmeta, tthr);
        return;
    }
    if constexpr (sizeof(OutT) == 1) {
        // ---- 8-bit scores with the score rows wanted: wave 0 holds the final planes; its lanes
        // transpose them to bytes in registers, stage the 128 bytes of their chunk in LDS, and all
        // threads of the group copy the tile out in 16-byte pieces (coalesced stores)
        if (a.write_counts || !a.thresholds) {
            uint8_t* stage = smem;                       // the merge buffers are done with
            if (wave == 0u && (MQ || lane < W)) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t o[8];
                    planes_to_bytes32<NP>(pl[w], o);
                    uint4* dst = reinterpret_cast<uint4*>(stage + lane * kStageStride + w * 32);
                    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
                    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
                }
            }
            __syncthreads();
            COBS_STAMP(5);             // scores staged
            const uint32_t npieces = (MQ ? 64u : W) * 8u;            // 16 documents each
#pragma unroll 1
            for (uint32_t pc0 = wave * 64u; pc0 < npieces; pc0 += NW * 64) {   // wave-uniform bounds
                const uint32_t pc = pc0 + lane;
                const bool act = pc < npieces;
                const uint32_t L = act ? pc >> 3 : 0u, rb = (pc & 7u) * 2u;   // lane that staged it, first row byte
                const uint32_t chunk = MQ ? (L & (W - 1u)) : L;
                const uint32_t q2raw = MQ ? qi * G + L / W : qi;
                const uint32_t q2 = q2raw < a.nq ? q2raw : a.nq - 1u;
                const uint32_t vb = tmeta[chunk * 3 + 1];                     // valid row bytes of the chunk
                const bool valid = act && q2raw < a.nq && rb < vb;
                const uint4 v = *reinterpret_cast<const uint4*>(stage + L * kStageStride + rb * 8u);
                const uint32_t slot = tmeta[chunk * 3 + 0] + rb * 8u;
                if (valid && a.write_counts) {
                    OutT* crow = reinterpret_cast<OutT*>(a.counts) + (uint64_t)q2 * a.counts_stride + a.counts_offset;
                    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                    // (two 8-byte stores per piece.  Round 4 measured the alternatives, interleaved inside one process: one 16-byte
                    // store where all slots are multiples of 16 is 2.8 % SLOWER on 50-bp reads and 1.3 % on 150-bp reads; 8-byte
                    // pieces laid out so that a wave-store covers 512 contiguous bytes came out 4 % faster in one build and 2 %
                    // slower in the next -- below what separates two processes on one box: profiles/r04_short_read_experiments.txt)
                    u32x2* dst = reinterpret_cast<u32x2*>(crow + slot);       // slots are multiples of 8, not of 16
                    const u32x2 v0 = {v.x, v.y}, v1 = {v.z, v.w};
                    dst[0] = v0;
                    if (rb + 1u < vb) dst[1] = v1;
                }
                if (a.thresholds) {
                    // counts_to_result filter: score >= threshold over real documents only
                    const uint32_t thr = tthr[MQ ? L / W : 0u];
                    const uint32_t doc = tmeta[chunk * 3 + 2] + rb * 8u;
                    const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
                    uint32_t mask = 0u;
                    if (valid) {
                        const uint32_t nd = rb + 1u < vb ? 16u : 8u;
#pragma unroll
                        for (uint32_t d = 0; d < 16; ++d) {
                            const uint32_t cnt = (vv[d >> 2] >> ((d & 3u) * 8u)) & 0xFFu;
                            if (d < nd && cnt >= thr && doc + d < a.num_docs) mask |= 1u << d;
                        }
                    }
                    if (__any(mask != 0u)) {
                        unsigned long long pos = pool_append((uint32_t)__popc(mask), a.hit_count, lane);
                        while (mask != 0u) {
                            const uint32_t d = (uint32_t)__ffs((int)mask) - 1u;
                            mask &= mask - 1u;
                            if (pos < a.hit_cap)
                                a.hits[pos] = HitDev{q2, a.part, doc + d, (vv[d >> 2] >> ((d & 3u) * 8u)) & 0xFFu};
                            ++pos;
                        }
                    }
                }
            }
            COBS_STAMP(6);             // scores stored
            return;
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < NP; ++k)
            mbuf[k * 64 + lane] = make_uint4(pl[0][k], pl[1][k], pl[2][k], pl[3][k]);
    }
    __syncthreads();

    COBS_STAMP(5);                 // merged planes are in LDS
    // ---- expand planes -> per-document counts; every thread handles row bytes ----
    const uint32_t* planes = reinterpret_cast<const uint32_t*>(mbuf);   // [NP][64*4 words]
    if (!a.write_counts && a.thresholds) {
        // Hits only (threshold > 0, the scores themselves are not wanted): compare in bit-sliced
        // form -- one 32-bit word = 32 documents, count >= threshold in NP boolean ops -- and
        // expand nothing unless a document passes.  With the usual thresholds hardly any word
        // holds a hit, so this replaces the whole LUT expansion (short reads: a third of the kernel).
        const uint32_t nwords = MQ ? 256u : W * 4u;
#pragma unroll 1
        for (uint32_t w0 = wave * 64u; w0 < nwords; w0 += NW * 64) {     // wave-uniform bounds
            const uint32_t w = w0 + lane;
            const bool act = w < nwords;
            const uint32_t pl_lane = act ? w >> 2 : 0u, comp = w & 3u;
            const uint32_t chunk = MQ ? (pl_lane & (W - 1u)) : pl_lane;
            const uint32_t q2raw = MQ ? qi * G + pl_lane / W : qi;
            const uint32_t q2 = q2raw < a.nq ? q2raw : a.nq - 1u;
            const uint32_t thr = tthr[MQ ? pl_lane / W : 0u];
            const uint32_t vbc = tmeta[chunk * 3 + 1];                       // valid row bytes of the chunk (0: dead)
            const bool valid = act && vbc != 0u && q2raw < a.nq;
            // ge bit d = (count of document d >= thr), from the lowest plane up:
            //   threshold bit 1: ge &= plane, threshold bit 0: ge |= plane
            uint32_t ge = (NP < 32 && (thr >> (NP < 32 ? NP : 0)) != 0u) ? 0u : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint32_t pk = planes[(k * 64 + pl_lane) * 4 + comp];
                ge = ((thr >> k) & 1u) ? (ge & pk) : (ge | pk);
            }
            // real documents only: row bytes inside the page, document ids below num_docs
            const uint32_t vb = vbc > comp * 4u ? vbc - comp * 4u : 0u;                       // valid bytes of the word
            if (vb < 4u) ge &= vb == 0u ? 0u : (1u << (vb * 8u)) - 1u;
            const uint32_t doc0 = tmeta[chunk * 3 + 2] + comp * 32u;
            const uint32_t nd = a.num_docs > doc0 ? a.num_docs - doc0 : 0u;
            if (nd < 32u) ge &= nd == 0u ? 0u : (1u << nd) - 1u;
            if (!valid) ge = 0u;
            if (__any(ge != 0u)) {
                unsigned long long pos = pool_append((uint32_t)__popc(ge), a.hit_count, lane);
                while (ge != 0u) {
                    const uint32_t d = (uint32_t)__ffs((int)ge) - 1u;
                    ge &= ge - 1u;
                    uint32_t score = 0u;
#pragma unroll
                    for (int k = 0; k < NP; ++k)
                        score |= ((planes[(k * 64 + pl_lane) * 4 + comp] >> d) & 1u) << k;
                    if (pos < a.hit_cap) a.hits[pos] = HitDev{q2, a.part, doc0 + d, score};
                    ++pos;
                }
            }
        }
        return;
    }
    if constexpr (sizeof(OutT) == 1) return;         // 8-bit scores left through one of the two paths above
    const uint32_t nbytes = MQ ? 1024u : W * 16u;    // MQ: every lane group holds a query's tile
    // MQ: 1024 / (NW * 64) = 4..16 iterations per thread.  Unrolled by four so that the score stores
    // of consecutive iterations use different registers: with one register set the next iteration's
    // first write to the store's data registers waits (vmcnt) until the store has left the CU --
    // measured 2 500 cycles per iteration, half of a short-read work-group's life.
    // (A counted loop: with the thread-dependent start as induction variable the unroller gives up.)
    constexpr int kUnroll = MQ ? 4 : 1;
    const uint32_t niter = MQ ? 1024u / (NW * 64) : (nbytes + NW * 64 - 1u) / (NW * 64);
#pragma unroll kUnroll
    for (uint32_t it = 0; it < niter; ++it) {
        const uint32_t b = threadIdx.x + it * (NW * 64);             // row byte inside the tile
        if (!MQ && b >= nbytes) break;
        const uint32_t pl_lane = b >> 4, cb = b & 15u;               // lane that held the planes
        const uint32_t chunk = MQ ? (pl_lane & (W - 1u)) : pl_lane;
        const uint32_t q2raw = MQ ? qi * G + pl_lane / W : qi;
        const uint32_t q2 = q2raw < a.nq ? q2raw : a.nq - 1u;
        const uint32_t thr = a.thresholds ? tthr[MQ ? pl_lane / W : 0u] : 0u;
        OutT* crow = reinterpret_cast<OutT*>(a.counts) + (uint64_t)q2 * a.counts_stride + a.counts_offset;
        const bool valid = q2raw < a.nq && cb < tmeta[chunk * 3 + 1];

        // one LDS lookup spreads the 8 document bits of a plane byte into 8 sixteen-bit
        // fields (4 dwords); shifting the dwords by the plane number adds that plane to all
        // 8 counters at once.  Planes 16.. go to a second accumulator (32-bit scores).
        uint32_t lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};
        const uint32_t sh = (cb & 3u) * 8u;
        uint32_t cnt[8];
        if constexpr (sizeof(OutT) == 1) {
            static_assert(sizeof(OutT) != 1 || NP <= 8, "8-bit scores hold at most 8 planes");
            const uint2* lut8 = reinterpret_cast<const uint2*>(lut);
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint32_t v = (planes[(k * 64 + pl_lane) * 4 + (cb >> 2)] >> sh) & 0xFFu;
                const uint2 e = lut8[v];
                lo[0] |= e.x << k; lo[1] |= e.y << k;
            }
#pragma unroll
            for (int d = 0; d < 8; ++d) cnt[d] = (lo[d >> 2] >> ((d & 3) * 8)) & 0xFFu;
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const uint32_t v = (planes[(k * 64 + pl_lane) * 4 + (cb >> 2)] >> sh) & 0xFFu;
                const uint4 e = lut[v];
                if (k < 16) {
                    lo[0] |= e.x << k; lo[1] |= e.y << k; lo[2] |= e.z << k; lo[3] |= e.w << k;
                } else {
                    hi[0] |= e.x << (k - 16); hi[1] |= e.y << (k - 16);
                    hi[2] |= e.z << (k - 16); hi[3] |= e.w << (k - 16);
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                cnt[2 * m] = (lo[m] & 0xFFFFu) | ((hi[m] & 0xFFFFu) << 16);
                cnt[2 * m + 1] = (lo[m] >> 16) | (hi[m] & 0xFFFF0000u);
            }
        }
        const uint32_t slot = tmeta[chunk * 3 + 0] + cb * 8u;
        if (valid && a.write_counts) {
            if constexpr (sizeof(OutT) == 1) {
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                u32x2* dst = reinterpret_cast<u32x2*>(crow + slot);
                const u32x2 v = {lo[0], lo[1]};
                *dst = v;          // (non-temporal stores measured equal: scripts/ab.py, 50..150-bp reads, C2, C3)
            } else if constexpr (sizeof(OutT) == 2) {
                u32x4* dst = reinterpret_cast<u32x4*>(crow + slot);
                const u32x4 v = {lo[0], lo[1], lo[2], lo[3]};
                *dst = v;          // (non-temporal stores measured equal: scripts/ab.py, 50..150-bp reads, C2, C3)
            } else {
                *reinterpret_cast<uint4*>(crow + slot) = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
                *reinterpret_cast<uint4*>(crow + slot + 4) = make_uint4(cnt[4], cnt[5], cnt[6], cnt[7]);
            }
        }
        if (a.thresholds) {
            // counts_to_result filter: score >= threshold over real documents only
            const uint32_t doc = tmeta[chunk * 3 + 2] + cb * 8u;
            uint32_t mask = 0u;
            if (valid) {
#pragma unroll
                for (int d = 0; d < 8; ++d)
                    if (cnt[d] >= thr && doc + d < a.num_docs) mask |= 1u << d;
            }
            if (__any(mask != 0u)) {
                unsigned long long pos = pool_append((uint32_t)__popc(mask), a.hit_count, lane);
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    if (mask & (1u << d)) {
                        if (pos < a.hit_cap) a.hits[pos] = HitDev{q2, a.part, doc + d, cnt[d]};
                        ++pos;
                    }
                }
            }
        }
    }
    COBS_STAMP(6);                 // scores stored
}

// ---------------------------------------------------------------------------
// launch side (host): one instantiation per (planes, waves, single hash, score type, multi-query, index width,
// LDS-staged, tile top-k, findere).  This file instantiates the FZ = false ones, scan_findere.hip the FZ = true ones.

template <int NP, int NW, bool H1, typename OutT, bool MQ = false, typename IdxT = uint32_t, bool LDSS = false, bool TK = false,
          bool FZ = false, bool SH = false>
static hipError_t launch_scan_inst(const ScanArgs& a, hipStream_t stream) {
    const uint32_t per_group = MQ ? 64u / a.tile_w : 1u;
    const uint64_t groups = (uint64_t)((a.chunk_end - a.chunk_begin + a.tile_w - 1) / a.tile_w) *
                            ((a.nq + per_group - 1u) / per_group);
    if (groups == 0) return hipSuccess;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    constexpr size_t front = scan_lds_front<NP, NW, sizeof(OutT), LDSS, SH>();
    constexpr size_t lds = front + (sizeof(OutT) == 1 ? 0 : 256 * sizeof(uint4)) + 64 * 4 * sizeof(uint32_t);
    auto kern = scan_kernel<NP, NW, H1, OutT, MQ, IdxT, LDSS, TK, FZ, SH>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((uint32_t)groups), dim3(NW * 64), lds, stream, a);
    return hipGetLastError();
}

// The launch dispatch over (waves per group x a flag): calls launch(std::integral_constant<int, NW>{},
// std::bool_constant<FLAG>{}) for nw = 1, 2 or 4 (anything else counts as 4), as dispatch_idx_flag does for
// (index width x flag).
template <typename F>
inline hipError_t dispatch_waves_flag(int nw, bool flag, F&& launch) {
    using std::integral_constant;
    if (nw == 1) return flag ? launch(integral_constant<int, 1>{}, std::true_type{}) : launch(integral_constant<int, 1>{}, std::false_type{});
    if (nw == 2) return flag ? launch(integral_constant<int, 2>{}, std::true_type{}) : launch(integral_constant<int, 2>{}, std::false_type{});
    return flag ? launch(integral_constant<int, 4>{}, std::true_type{}) : launch(integral_constant<int, 4>{}, std::false_type{});
}

// multi-query variant: H = 1 (short queries); the flag is "run_topk without score rows"
template <int NP, typename OutT, bool FZ>
static hipError_t launch_scan_mq(const ScanArgs& a, int nw, hipStream_t stream) {
    return dispatch_waves_flag(nw, a.cand != nullptr, [&](auto w, auto tk) {
        return launch_scan_inst<NP, decltype(w)::value, true, OutT, true, uint32_t, false, decltype(tk)::value, FZ>(a, stream);
    });
}

template <int NP, typename OutT, bool FZ>
static hipError_t launch_scan_np(const ScanArgs& a, bool h1, int nw, hipStream_t stream) {
    if (a.cand) {           // run_topk without score rows: 32-bit row indices (scan_has_tile_topk)
        if (a.idx64) return hipErrorInvalidValue;
        return dispatch_waves_flag(nw, h1, [&](auto w, auto h) {
            return launch_scan_inst<NP, decltype(w)::value, decltype(h)::value, OutT, false, uint32_t, false, true, FZ>(a, stream);
        });
    }
    if (a.idx64) {
        // sub-indexes with >= 2^32 rows: 64-bit row indices; two waves per group cover every
        // query length well enough for this rare geometry (keeps the instantiation count down)
        return h1 ? launch_scan_inst<NP, 2, true, OutT, false, uint64_t, false, false, FZ>(a, stream)
                  : launch_scan_inst<NP, 2, false, OutT, false, uint64_t, false, false, FZ>(a, stream);
    }
    return dispatch_waves_flag(nw, h1, [&](auto w, auto h) {
        return launch_scan_inst<NP, decltype(w)::value, decltype(h)::value, OutT, false, uint32_t, false, false, FZ>(a, stream);
    });
}

// every plain (FZ = false) or every findere (FZ = true) instantiation, by planes
template <bool FZ>
static hipError_t launch_scan_fz(const ScanArgs& a, int planes, int nw, bool multi_query, hipStream_t stream) {
    const bool h1 = a.num_hashes == 1;
    if (multi_query) {
        if (a.idx64 || !scan_has_multi_query(planes, a.num_hashes, a.tile_w)) return hipErrorInvalidValue;
        switch (planes) {
        case 4: return launch_scan_mq<4, uint8_t, FZ>(a, nw, stream);
        case 8: return launch_scan_mq<8, uint8_t, FZ>(a, nw, stream);
        case 10: return launch_scan_mq<10, uint16_t, FZ>(a, nw, stream);
        default: return launch_scan_mq<12, uint16_t, FZ>(a, nw, stream);
        }
    }
    switch (planes) {
    case 4: return launch_scan_np<4, uint8_t, FZ>(a, h1, nw, stream);
    case 8: return launch_scan_np<8, uint8_t, FZ>(a, h1, nw, stream);
    case 10: return launch_scan_np<10, uint16_t, FZ>(a, h1, nw, stream);
    case 12: return launch_scan_np<12, uint16_t, FZ>(a, h1, nw, stream);
    case 16: return launch_scan_np<16, uint16_t, FZ>(a, h1, nw, stream);
    case 20: return launch_scan_np<20, uint32_t, FZ>(a, h1, nw, stream);
    case 24: return launch_scan_np<24, uint32_t, FZ>(a, h1, nw, stream);
    case 32: return launch_scan_np<32, uint32_t, FZ>(a, h1, nw, stream);
    default: return hipErrorInvalidValue;
    }
}

// the findere half (scan_findere.hip), called by launch_scan below
hipError_t launch_scan_findere(const ScanArgs& a, int planes, int nw, bool multi_query, hipStream_t stream);

#ifndef COBS_SCAN_FINDERE_UNIT      // what follows is defined once, in the translation unit of this file

int scan_planes_for(uint64_t max_terms) {
    int need = 1;
    while (need < 64 && (max_terms >> need) != 0) ++need;     // bit width of max_terms
    static const int avail[] = {4, 8, 10, 12, 16, 20, 24, 32};
    for (int v : avail)
        if (v >= need) return v;
    return -1;
}

template <int NP, typename OutT>
static hipError_t launch_scan_sh(const ScanArgs& a, int nw, hipStream_t stream) {
    if (nw == 1) return launch_scan_inst<NP, 1, true, OutT, false, uint32_t, false, false, false, true>(a, stream);
    if (nw == 2) return launch_scan_inst<NP, 2, true, OutT, false, uint32_t, false, false, false, true>(a, stream);
    return launch_scan_inst<NP, 4, true, OutT, false, uint32_t, false, false, false, true>(a, stream);
}


hipError_t launch_scan(const ScanArgs& a, uint32_t ntiles, int planes, int nw, bool multi_query, uint64_t max_blocks,
                       hipStream_t stream) {
    (void)ntiles;
    if (a.cand && (a.lds_staged || a.topk_k == 0 || !scan_has_tile_topk(a.num_hashes, a.idx64 != 0))) return hipErrorInvalidValue;
    if (a.findere > 7u || (a.findere && a.lds_staged)) return hipErrorInvalidValue;
    if (a.lds_staged) {     // measured variant (A/B): rows through LDS
        if (multi_query || a.idx64 || !scan_has_lds_staged(planes, a.num_hashes, nw)) return hipErrorInvalidValue;
        return nw == 2 ? launch_scan_inst<10, 2, true, uint16_t, false, uint32_t, true>(a, stream)
                       : launch_scan_inst<10, 4, true, uint16_t, false, uint32_t, true>(a, stream);
    }
    if (a.self_hash) {      // the work-groups hash for themselves: no table
        if (multi_query || a.cand || a.findere || !a.text || !scan_has_self_hash(planes, a.num_hashes, 31u, a.idx64 != 0)) return hipErrorInvalidValue;
        // (the bound the work-groups test before they write their LDS array, for the longest query and the widest tile)
        if (!scan_self_hash_fits(a.npages, a.cpp, a.tile_w, max_blocks)) return hipErrorInvalidValue;
        switch (planes) {
        case 4: return launch_scan_sh<4, uint8_t>(a, nw, stream);
        case 8: return launch_scan_sh<8, uint8_t>(a, nw, stream);
        case 10: return launch_scan_sh<10, uint16_t>(a, nw, stream);
        default: return launch_scan_sh<12, uint16_t>(a, nw, stream);
        }
    }
    // findere: its own instantiations, so that z = 0 launches exactly the plain kernels
    return a.findere ? launch_scan_findere(a, planes, nw, multi_query, stream)
                     : launch_scan_fz<false>(a, planes, nw, multi_query, stream);
}

#endif  // COBS_SCAN_FINDERE_UNIT

}  // namespace cobs_amd
