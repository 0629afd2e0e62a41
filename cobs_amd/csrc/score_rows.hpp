// cobs_amd/csrc/score_rows.hpp -- how the kernels that run behind a pass's scan read its score rows (u8, u16 or u32
// [nq][nslots]): 16 bytes per lane along the slot dimension.  Shared by group_kernels.hip and best_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cobs_amd {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename ST>
__device__ __forceinline__ uint32_t score_of(const u32x4& v, uint32_t j) {
    if (sizeof(ST) == 1) return (v[j / 4u] >> (8u * (j % 4u))) & 0xFFu;
    if (sizeof(ST) == 2) return (v[j / 2u] >> (16u * (j % 2u))) & 0xFFFFu;
    return v[j];
}

// 16 bytes of one score row (rows of u8 scores are 8-byte aligned only: local_counts is a multiple of 8); a lane at the
// end of a u8 row whose last 8 slots do not exist loads the 8 that do
__device__ __forceinline__ u32x4 load_scores(const uint8_t* p, bool half) {
    if (half) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(p);
        return u32x4{w[0], w[1], 0u, 0u};
    }
    u32x4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 16);
    return v;
}

}  // namespace cobs_amd
