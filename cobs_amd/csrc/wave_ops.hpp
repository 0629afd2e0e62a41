// cobs_amd/csrc/wave_ops.hpp -- small device helpers more than one kernel file uses (gfx950, wave64): DPP cross-lane
// moves, the lane-group sum and the wave scan built from them, the hit pool's append, the carry-save adder, a bit mask, and the launch dispatch over
// (index width x single hash).  Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace cobs_amd {

// Cross-lane steps inside a row of 16 lanes as DPP modifiers of the VALU (v_add_u32 ..._dpp: no trip through the
// LDS crossbar, which a ds_bpermute-based __shfl costs -- ~100 cycles of latency per dependent step).
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF, bool BOUND_ZERO = true>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, BOUND_ZERO);
}
constexpr int kDppQuadXor1 = 0xB1;       // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;       // quad_perm:[2,3,0,1]
constexpr int kDppRowMirror = 0x140;     // lane i <- lane 15 - i of its row
constexpr int kDppHalfMirror = 0x141;    // lane i <- lane 7 - i of its half row
constexpr int kDppRowShr = 0x110;        // + n: lane i <- lane i - n of its row (0 shifted in)
constexpr int kDppBcast15 = 0x142;       // lane 15 of a row -> every lane of the next row
constexpr int kDppBcast31 = 0x143;       // lane 31 -> every lane of rows 2 and 3

// sum of `c` over the W (power of two, 1..64) consecutive lanes of a lane group; the LAST lane of the group holds it
// (up to 16 lanes every lane does).  Every lane of the wave takes part.
__device__ __forceinline__ uint32_t group_sum_last(uint32_t c, uint32_t W) {
    if (W >= 2u) c += dpp_mov<kDppQuadXor1>(c);
    if (W >= 4u) c += dpp_mov<kDppQuadXor2>(c);
    if (W >= 8u) c += dpp_mov<kDppHalfMirror>(c);
    if (W >= 16u) c += dpp_mov<kDppRowMirror>(c);
    if (W >= 32u) c += dpp_mov<kDppBcast15, 0xA, 0xF, false>(c);      // rows 1 and 3 += the total of the row before
    if (W >= 64u) c += dpp_mov<kDppBcast31, 0xC, 0xF, false>(c);      // rows 2 and 3 += the total of the first half
    return c;
}

// inclusive prefix sum over the 64 lanes of a wave: four row steps, then lane 15 / lane 31 broadcasts (GFX9 DPP)
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t v) {
    v += dpp_mov<kDppRowShr + 1>(v);
    v += dpp_mov<kDppRowShr + 2>(v);
    v += dpp_mov<kDppRowShr + 4>(v);
    v += dpp_mov<kDppRowShr + 8>(v);
    v += dpp_mov<kDppBcast15, 0xA, 0xF, false>(v);      // rows 1 and 3 += the total of the row before
    v += dpp_mov<kDppBcast31, 0xC, 0xF, false>(v);      // rows 2 and 3 += the total of the first half
    return v;
}

// Append to a pool with a 64-bit fill counter, one atomic per wave: lane `lane` brings n records (0: none) and gets
// the position of its first one; its records go to consecutive positions from there.  The caller writes them and
// checks every position against the pool's capacity (the counter may run past it: that is how overflow shows).  Called
// by all 64 lanes of a wave, with converged control flow.
__device__ __forceinline__ unsigned long long pool_append(uint32_t n, unsigned long long* counter, uint32_t lane) {
    const uint32_t incl = wave_incl_scan_dpp(n);
    const uint32_t total = __shfl(incl, 63);
    unsigned long long base = 0ull;
    if (lane == 63u) base = atomicAdd(counter, (unsigned long long)total);
    base = __shfl(base, 63);
    return base + incl - n;
}

// carry-save adder: (h, l) = a + b + c per bit position.  gfx950 has a three-input boolean op (v_bitop3_b32, 8-bit
// truth table), so majority (0xE8) and parity (0x96) are one instruction each: a CSA is 2 VALU ops.
__device__ __forceinline__ void csa(uint32_t& h, uint32_t& l, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t hh = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    const uint32_t ll = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    h = hh;
    l = ll;
}

// the low r bits (r >= 32: all)
__device__ __forceinline__ uint32_t low_bits(uint32_t r) { return r >= 32u ? 0xFFFFFFFFu : (1u << r) - 1u; }

// The launch dispatch over (64-bit row indices x a flag, usually "one hash function"): calls
// launch(IdxT{}, std::bool_constant<FLAG>{}) with the matching pair, for a generic lambda that names its kernel as
// kernel<decltype(idx), decltype(flag)::value>.
template <typename F>
inline void dispatch_idx_flag(bool idx64, bool flag, F&& launch) {
    if (idx64) {
        if (flag) launch(uint64_t{}, std::true_type{});
        else launch(uint64_t{}, std::false_type{});
    } else {
        if (flag) launch(uint32_t{}, std::true_type{});
        else launch(uint32_t{}, std::false_type{});
    }
}

}  // namespace cobs_amd
