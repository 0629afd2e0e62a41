// cobs_amd/csrc/walk_ops.hpp -- the device helpers the two scans that walk a query in order share (the coverage scan,
// coverage_kernels.hip, and the window scan, window_kernels.hip): one definition, so that the parts the window scan takes
// from the coverage scan stay the same code.  Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_ops.hpp"      // csa

namespace cobs_amd {

// eight words into the three planes p[0..2]; returns the carry into the plane above them
__device__ __forceinline__ uint32_t absorb8(uint32_t* p, const uint32_t (&x)[8]) {
    uint32_t t2a, t2b, f4a, f4b, e8;
    csa(t2a, p[0], p[0], x[0], x[1]);
    csa(t2b, p[0], p[0], x[2], x[3]);
    csa(f4a, p[1], p[1], t2a, t2b);
    csa(t2a, p[0], p[0], x[4], x[5]);
    csa(t2b, p[0], p[0], x[6], x[7]);
    csa(f4b, p[1], p[1], t2a, t2b);
    csa(e8, p[2], p[2], f4a, f4b);
    return e8;
}

__device__ __forceinline__ uint32_t word_of(const uint4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

__device__ __forceinline__ uint4 load_row(const uint8_t* lane_base, uint64_t row, uint32_t pitch) {
    return *reinterpret_cast<const uint4*>(lane_base + row * pitch);
}

}  // namespace cobs_amd
