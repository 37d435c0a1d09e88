// fse_pack_dev.hpp -- the device pieces the pack transforms (fse_pack.hip,
// fsehip.h section 2j) and the versioned pack's (fse_vpack.hip, section 2k)
// share: the tile's member by binary search, the plane and element accesses
// of one lane's 16-element group, and the group of a planes or delta member
// in and out of its planes.  Over the transposes of fse_planes_dev.hpp and
// the restart group's sum of fse_delta_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_delta_dev.hpp"
#include "fse_pack_host.h"

namespace fsehip {

namespace {

static_assert(FSEHIP_DELTA_RESTART == 16u * PL_T, "a tile is one restart group");

struct __attribute__((packed, aligned(1))) P16b {
    uint16_t v;
};

// the last member whose first tile is at or before `tile`: members without
// elements share their first tile with the next one and are never the last
__device__ __forceinline__ uint32_t member_of(const PackDesc* __restrict__ descs, uint32_t n, uint64_t tile) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (descs[mid].first_tile <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the group's 4 W dwords z -> W aligned 16-byte stores into member D's planes
template <int W>
__device__ __forceinline__ void store_planes(const PackDesc* __restrict__ D, uint64_t g, const uint32_t (&z)[4 * W],
                                             uint8_t* __restrict__ image) {
    if constexpr (W == 1) {
        *reinterpret_cast<uint4*>(image + D->plane[0] + (g << 4)) = make_uint4(z[0], z[1], z[2], z[3]);
    } else {
        uint32_t p[W][4];
        deinterleave<W>(z, p);
#pragma unroll
        for (int k = 0; k < W; ++k)
            *reinterpret_cast<uint4*>(image + D->plane[k] + (g << 4)) = make_uint4(p[k][0], p[k][1], p[k][2], p[k][3]);
    }
}

// the inverse: W aligned 16-byte loads from member D's planes -> the group's dwords
template <int W>
__device__ __forceinline__ void load_member_planes(const PackDesc* __restrict__ D, uint64_t g,
                                                   const uint8_t* __restrict__ planes, uint32_t (&e)[4 * W]) {
    uint32_t p[W][4];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint4 v = *reinterpret_cast<const uint4*>(planes + D->plane[k] + (g << 4));
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

// the group's elements e to d (aligned to W): exactly the group's bytes, `rem`
// of them in the member's ragged last group
template <int W>
__device__ __forceinline__ void store_group(uint8_t* d, bool whole, uint32_t rem, const uint32_t (&e)[4 * W]) {
    if (whole) {
        if constexpr (W == 1) {
            *reinterpret_cast<U128b*>(d) = U128b{e[0], e[1], e[2], e[3]};
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<U128u*>(d + 16 * j) = U128u{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) {
            if (4u * j + 4u <= rem) {
                reinterpret_cast<U32u*>(d + 4 * j)->v = e[j];
            } else if (4u * j < rem) {  // W <= 2: the last 1..3 bytes
                if constexpr (W == 2) {
                    reinterpret_cast<P16b*>(d + 4 * j)->v = (uint16_t)e[j];
                } else if constexpr (W == 1) {
#pragma unroll
                    for (uint32_t b = 0; b < 3; ++b)
                        if (4u * j + b < rem) d[4 * j + b] = (uint8_t)(e[j] >> (8u * b));
                }
            }
        }
    }
}

// group g of member D (16 elements at the lane's place) into its planes
template <int W, bool DELTA>
__device__ __forceinline__ void split_group(const PackDesc* __restrict__ D, uint64_t g, uint8_t* __restrict__ image) {
    const uint64_t n_elems = D->n_elems;
    if (g >= (n_elems + 15u) >> 4) return;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(D->ptr) + g * (16u * W);
    const bool whole = (g << 4) + 16u <= n_elems;
    // source bytes of the group; in the member's ragged last one whole dwords
    // that hold one are loaded (up to roundup(n_elems * W, 4), never more)
    const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
    uint32_t e[4 * W], z[4 * W];
    load_group<W>(s, whole, rem, e);
    if constexpr (DELTA) {
        delta_zigzag<W>(s, (g & (PL_T - 1u)) == 0, e, z);
    } else {
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) z[j] = e[j];
    }
    if (!whole) zero_pad<W>(z, rem);
    store_planes<W>(D, g, z, image);
}

// The inverse.  Every thread of the workgroup calls it (the delta sum has a
// barrier).  Stores are exactly the member's bytes, at the alignment of its
// elements.
template <int W, bool DELTA>
__device__ __forceinline__ void merge_group(const PackDesc* __restrict__ D, uint64_t g,
                                            const uint8_t* __restrict__ planes, uint64_t* tot) {
    const uint64_t n_elems = D->n_elems;
    const bool active = g < (n_elems + 15u) >> 4;
    uint32_t e[4 * W];
    if (active) {
        load_member_planes<W>(D, g, planes, e);
    } else {
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) e[j] = 0;
    }
    if constexpr (DELTA) delta_sum<W>(e, reinterpret_cast<typename Acc<W>::type*>(tot));
    if (!active) return;
    uint8_t* d = reinterpret_cast<uint8_t*>(D->ptr) + g * (16u * W);
    const bool whole = (g << 4) + 16u <= n_elems;
    store_group<W>(d, whole, whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W, e);
}

}  // namespace

}  // namespace fsehip
