// fse_planes_dev.hpp -- the device pieces the plane transforms (fse_planes.hip,
// fsehip.h section 2d) and the delta transforms (fse_delta.hip, section 2e)
// share: the launch shape, the under-aligned access types and the byte
// transposes on v_perm_b32.  Element i of a 16-element group is the dwords
// [i * W / 4, (i + 1) * W / 4) of the lane's 4 W.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fse_status.h"

namespace fsehip {

namespace {

constexpr uint32_t PL_T = 256;         // threads per workgroup
constexpr uint32_t PL_MAX_WGS = 2048;  // the capped grid: 8 workgroups per CU; one pass covers 2048 * 256 groups

// a 16-byte / 4-byte access at an address aligned to less than its size
// (global memory takes them; the element side is aligned to W only)
struct __attribute__((packed, aligned(2))) U128u {
    uint32_t x, y, z, w;
};
struct __attribute__((packed, aligned(1))) U32u {
    uint32_t v;
};

// bytes of {hi, lo} picked by sel: selector 0..3 = lo's bytes, 4..7 = hi's
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// 4 x 4 byte transpose: out[k] byte j = in[j] byte k (its own inverse)
__device__ __forceinline__ void tr4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t out[4]) {
    const uint32_t ab_lo = perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    const uint32_t ab_hi = perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    const uint32_t cd_lo = perm(d, c, 0x05010400u);
    const uint32_t cd_hi = perm(d, c, 0x07030602u);
    out[0] = perm(cd_lo, ab_lo, 0x05040100u);  // a0 b0 c0 d0
    out[1] = perm(cd_lo, ab_lo, 0x07060302u);
    out[2] = perm(cd_hi, ab_hi, 0x05040100u);
    out[3] = perm(cd_hi, ab_hi, 0x07060302u);
}

// 16 elements (4 W dwords) -> W planes of 4 dwords
template <int W>
__device__ __forceinline__ void deinterleave(const uint32_t (&e)[4 * W], uint32_t (&p)[W][4]) {
    if constexpr (W == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[0][q] = perm(e[2 * q + 1], e[2 * q], 0x06040200u);
            p[1][q] = perm(e[2 * q + 1], e[2 * q], 0x07050301u);
        }
    } else {
        constexpr int D = W / 4;  // dwords per element
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int h = 0; h < D; ++h) {
                uint32_t t[4];
                tr4(e[(4 * q + 0) * D + h], e[(4 * q + 1) * D + h], e[(4 * q + 2) * D + h], e[(4 * q + 3) * D + h], t);
#pragma unroll
                for (int k = 0; k < 4; ++k) p[4 * h + k][q] = t[k];
            }
    }
}

// the inverse
template <int W>
__device__ __forceinline__ void interleave(const uint32_t (&p)[W][4], uint32_t (&e)[4 * W]) {
    if constexpr (W == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            e[2 * q] = perm(p[1][q], p[0][q], 0x05010400u);
            e[2 * q + 1] = perm(p[1][q], p[0][q], 0x07030602u);
        }
    } else {
        constexpr int D = W / 4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int h = 0; h < D; ++h) {
                uint32_t t[4];
                tr4(p[4 * h + 0][q], p[4 * h + 1][q], p[4 * h + 2][q], p[4 * h + 3][q], t);
#pragma unroll
                for (int j = 0; j < 4; ++j) e[(4 * q + j) * D + h] = t[j];
            }
    }
}

// workgroups for `items` lanes' worth of work, capped
inline uint32_t grid_for(uint64_t items) {
    return (uint32_t)(items < (uint64_t)PL_MAX_WGS * PL_T ? (items + PL_T - 1u) / PL_T : PL_MAX_WGS);
}

inline int done() { return hipGetLastError() == hipSuccess ? FSE_OK : FSE_ERR_HIP; }

}  // namespace

}  // namespace fsehip
