// fse_vpack.hip -- the transforms of the versioned pack (fsehip.h section
// 2k), gfx950: the pack frame's tile kernels with a third member kind, the
// zigzag difference of a member's elements against a base tensor's (section
// 2h).  Over the device functions of fse_pack_dev.hpp (planes and delta
// groups, the tile's member) and the diff_zigzag / diff_unzigzag of
// fse_planes_dev.hpp.
//
//   vpack_split_kernel   every member's elements (and a diff member's base)
//                        -> the image (pads zeroed)
//   vpack_merge_kernel   planes (and a diff member's base) -> every member's
//                        elements; a diff member's destination may be its
//                        base itself
//
// Tiles, the member search and the uniform switch are fse_pack.hip's.  A
// member's base pointer is bases[m], a device array parallel to the
// descriptors, read with scalar loads for diff members only.  A diff tile
// moves three streams (elements, base, planes) through registers: no LDS, no
// barrier, no restart, so the delta sum's LDS set flips at delta tiles alone.
// The finish, check and member-status kernels are fse_pack.hip's, on the
// other head.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_pack_dev.hpp"

namespace fsehip {

namespace {

// group g of diff member D against its base into the member's planes; up to
// roundup(n_elems * W, 4) bytes of either source are read, never more
template <int W>
__device__ __forceinline__ void diff_split_group(const PackDesc* __restrict__ D, const uint8_t* __restrict__ base,
                                                 uint64_t g, uint8_t* __restrict__ image) {
    const uint64_t n_elems = D->n_elems;
    if (g >= (n_elems + 15u) >> 4) return;
    const bool whole = (g << 4) + 16u <= n_elems;
    const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
    uint32_t x[4 * W], b[4 * W], z[4 * W];
    load_group<W>(reinterpret_cast<const uint8_t*>(D->ptr) + g * (16u * W), whole, rem, x);
    load_group<W>(base + g * (16u * W), whole, rem, b);
    diff_zigzag<W, 4 * W>(x, b, z);
    if (!whole) zero_pad<W>(z, rem);  // the pad belongs to the image
    store_planes<W>(D, g, z, image);
}

// The inverse.  The destination may be the base itself, so neither pointer is
// __restrict__: the lane loads its 16 base elements before it stores the same
// 16, and no other lane touches them.
template <int W>
__device__ __forceinline__ void diff_merge_group(const PackDesc* __restrict__ D, const uint8_t* base, uint64_t g,
                                                 const uint8_t* __restrict__ planes) {
    const uint64_t n_elems = D->n_elems;
    if (g >= (n_elems + 15u) >> 4) return;
    const bool whole = (g << 4) + 16u <= n_elems;
    const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
    const uint8_t* s = base + g * (16u * W);
    if constexpr (W == 8) {
        if (!whole) {
            // one lane of the member, at most 15 elements: element by element
            // from the planes' bytes, two dwords each, as diff_merge_kernel<8>,
            // so that the whole groups' path alone sets the kernel's registers
            uint8_t* d = reinterpret_cast<uint8_t*>(D->ptr) + g * (16u * W);
            for (uint32_t i = 0; 8u * i < rem; ++i) {
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) v |= (uint64_t)planes[D->plane[k] + (g << 4) + i] << (8 * k);
                const uint64_t bv = (uint64_t)reinterpret_cast<const U32u*>(s + 8 * i)->v |
                                    ((uint64_t)reinterpret_cast<const U32u*>(s + 8 * i + 4)->v << 32);
                const uint64_t x = bv + ((v >> 1) ^ (0 - (v & 1u)));
                reinterpret_cast<U32u*>(d + 8 * i)->v = (uint32_t)x;
                reinterpret_cast<U32u*>(d + 8 * i + 4)->v = (uint32_t)(x >> 32);
            }
            return;
        }
    }
    uint32_t z[4 * W], b[4 * W], e[4 * W];
    load_member_planes<W>(D, g, planes, z);
    if (whole) {
        if constexpr (W == 1) {
            const U128b v = *reinterpret_cast<const U128b*>(s);
            b[0] = v.x;
            b[1] = v.y;
            b[2] = v.z;
            b[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const U128u v = *reinterpret_cast<const U128u*>(s + 16 * j);
                b[4 * j] = v.x;
                b[4 * j + 1] = v.y;
                b[4 * j + 2] = v.z;
                b[4 * j + 3] = v.w;
            }
        }
    } else {
        // whole dwords that hold a base byte, up to roundup(n_elems * W, 4)
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) b[j] = 4u * j < rem ? reinterpret_cast<const U32u*>(s + 4 * j)->v : 0u;
    }
    diff_unzigzag<W, 4 * W>(z, b, e);
    store_group<W>(reinterpret_cast<uint8_t*>(D->ptr) + g * (16u * W), whole, rem, e);
}

template <int W>
__device__ __forceinline__ void split_tile(const PackDesc* __restrict__ D, const uint64_t* __restrict__ bases,
                                           uint32_t m, uint64_t g, uint8_t* __restrict__ image) {
    if (D->kind == FSEHIP_KIND_DIFF) diff_split_group<W>(D, reinterpret_cast<const uint8_t*>(bases[m]), g, image);
    else if (D->kind == FSEHIP_KIND_DELTA) split_group<W, true>(D, g, image);
    else split_group<W, false>(D, g, image);
}

template <int W>
__device__ __forceinline__ void merge_tile(const PackDesc* __restrict__ D, const uint64_t* __restrict__ bases,
                                           uint32_t m, uint64_t g, const uint8_t* __restrict__ planes, uint64_t* tot) {
    if (D->kind == FSEHIP_KIND_DIFF) diff_merge_group<W>(D, reinterpret_cast<const uint8_t*>(bases[m]), g, planes);
    else if (D->kind == FSEHIP_KIND_DELTA) merge_group<W, true>(D, g, planes, tot);
    else merge_group<W, false>(D, g, planes, nullptr);
}

uint32_t tile_grid(uint64_t tiles) { return (uint32_t)(tiles < PL_MAX_WGS ? tiles : PL_MAX_WGS); }

}  // namespace

__global__ __launch_bounds__(PL_T) void vpack_split_kernel(const PackDesc* __restrict__ descs,
                                                           const uint64_t* __restrict__ bases, uint32_t n,
                                                           uint64_t tiles, uint8_t* __restrict__ image) {
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t m = member_of(descs, n, tile);
        const PackDesc* D = descs + m;
        const uint64_t g = (tile - D->first_tile) * PL_T + threadIdx.x;
        switch (D->w) {
            case 1: split_tile<1>(D, bases, m, g, image); break;
            case 2: split_tile<2>(D, bases, m, g, image); break;
            case 4: split_tile<4>(D, bases, m, g, image); break;
            default: split_tile<8>(D, bases, m, g, image); break;
        }
    }
}

// `tot` alternates between two sets from one delta tile to the next, as in
// pack_merge_kernel; tiles of the plane and diff kinds have no barrier and
// leave the set alone.
__global__ __launch_bounds__(PL_T) void vpack_merge_kernel(const PackDesc* __restrict__ descs,
                                                           const uint64_t* __restrict__ bases, uint32_t n,
                                                           uint64_t tiles, const uint8_t* __restrict__ planes,
                                                           const int32_t* __restrict__ result) {
    if (result && *result == FSE_ERR_BAD_FRAME) return;
    __shared__ uint64_t tot[2][PL_T / 64];
    uint32_t set = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t m = member_of(descs, n, tile);
        const PackDesc* D = descs + m;
        const uint64_t g = (tile - D->first_tile) * PL_T + threadIdx.x;
        switch (D->w) {
            case 1: merge_tile<1>(D, bases, m, g, planes, tot[set]); break;
            case 2: merge_tile<2>(D, bases, m, g, planes, tot[set]); break;
            case 4: merge_tile<4>(D, bases, m, g, planes, tot[set]); break;
            default: merge_tile<8>(D, bases, m, g, planes, tot[set]); break;
        }
        if (D->kind == FSEHIP_KIND_DELTA) set ^= 1u;
    }
}

int launch_vpack_split(const PackDesc* d_descs, const uint64_t* d_bases, uint32_t n, uint64_t tiles, uint8_t* image,
                       void* stream) {
    if (tiles == 0) return FSE_OK;
    hipLaunchKernelGGL(vpack_split_kernel, dim3(tile_grid(tiles)), dim3(PL_T), 0, static_cast<hipStream_t>(stream),
                       d_descs, d_bases, n, tiles, image);
    return done();
}

int launch_vpack_merge(const PackDesc* d_descs, const uint64_t* d_bases, uint32_t n, uint64_t tiles,
                       const uint8_t* planes, const int32_t* result, void* stream) {
    if (tiles == 0) return FSE_OK;
    hipLaunchKernelGGL(vpack_merge_kernel, dim3(tile_grid(tiles)), dim3(PL_T), 0, static_cast<hipStream_t>(stream),
                       d_descs, d_bases, n, tiles, planes, result);
    return done();
}

}  // namespace fsehip
