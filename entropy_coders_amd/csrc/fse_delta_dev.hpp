// fse_delta_dev.hpp -- the device pieces the delta merge (fse_delta.hip,
// fsehip.h section 2e) and the pack merge (fse_pack.hip, section 2j) share:
// the restart group's prefix sum over one workgroup, and the plane loads that
// feed it.  Over the transposes of fse_planes_dev.hpp and the DPP scans of
// fse_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_device.hpp"
#include "fse_planes_dev.hpp"

namespace fsehip {

namespace {

template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp0_64(uint64_t v) {
    return (uint64_t)dpp0<CTRL, ROWS>((uint32_t)v) | ((uint64_t)dpp0<CTRL, ROWS>((uint32_t)(v >> 32)) << 32);
}
// wave_incl_sum on both halves, each step's add carrying from the low half to the high one
__device__ __forceinline__ uint64_t wave_incl_sum64(uint64_t v) {
    v += dpp0_64<0x111, 0xf>(v);  // row_shr:1
    v += dpp0_64<0x112, 0xf>(v);  // row_shr:2
    v += dpp0_64<0x114, 0xf>(v);  // row_shr:4
    v += dpp0_64<0x118, 0xf>(v);  // row_shr:8
    v += dpp0_64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp0_64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// The zigzag deltas of 16 consecutive elements of one restart group, a group
// per workgroup and 16 elements per lane in lane order, become the elements:
// un-zigzag, sum inside the lane, scan the lane totals across the wave, add
// the totals of the waves before (`tot`: 4 entries, written and read round the
// one barrier).  Every thread of the workgroup calls this; a lane with no
// elements passes zeros.
template <int W>
__device__ __forceinline__ void delta_sum(uint32_t (&e)[4 * W], typename Acc<W>::type* tot) {
    using A = typename Acc<W>::type;
    A x[16], acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const A z = get<W>(e, i);
        acc += (z >> 1) ^ (A)(0 - (z & 1u));
        x[i] = acc;
    }
    A incl;
    if constexpr (W == 8) incl = wave_incl_sum64(acc);
    else incl = wave_incl_sum(acc);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) tot[wave] = incl;
    __syncthreads();
    A before = incl - acc;
#pragma unroll
    for (uint32_t v = 0; v < PL_T / 64 - 1; ++v) before += v < wave ? tot[v] : (A)0;
#pragma unroll
    for (int j = 0; j < 4 * W; ++j) e[j] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) put<W>(e, i, x[i] + before);
}

// W aligned 16-byte plane loads of group g -> the lane's element dwords
template <int W>
__device__ __forceinline__ void load_planes(const uint8_t* __restrict__ image, uint64_t stride, uint64_t g,
                                            uint32_t (&e)[4 * W]) {
    uint32_t p[W][4];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint4 v = *reinterpret_cast<const uint4*>(image + k * stride + (g << 4));
        p[k][0] = v.x;
        p[k][1] = v.y;
        p[k][2] = v.z;
        p[k][3] = v.w;
    }
    if constexpr (W == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = p[0][j];
    } else {
        interleave<W>(p, e);
    }
}

}  // namespace

}  // namespace fsehip
