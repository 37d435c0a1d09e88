// fse_pack.hip -- the transforms of the pack frame (fsehip.h section 2j),
// gfx950: many tensors' byte planes in and out of one image, one launch each
// way.  Bandwidth kernels over the device functions of fse_planes_dev.hpp and
// the restart group's sum of fse_delta_dev.hpp: every byte crosses HBM once,
// aligned 16-byte accesses on the image side, registers only but for the
// delta merge's four wave totals.
//
//   pack_split_kernel          every member's elements -> the image (pads zeroed)
//   pack_merge_kernel          planes -> every member's elements; the planes
//                              lie where the descriptors say: in the decoded
//                              image, or in the range scratch of a
//                              selected-member decode
//   pack_finish_kernel         encode: the head bytes and the length
//   pack_check_kernel          decode: the head on the device == the caller's
//   pack_bad_fill_kernel       decode: BAD_FRAME into every status
//   pack_member_status_kernel  members: w plane statuses -> one per member
//
// Work comes in tiles: one workgroup's 256 lanes take up to 256 consecutive
// 16-element groups of ONE member, which is one delta restart group.  The
// tile's member is found by a binary search over the descriptors' first
// tiles, on the workgroup's tile number alone: every lane of the workgroup
// gets the same member, so the descriptor is read with scalar loads and the
// switch on its width and kind never diverges inside a wave (nor does the
// barrier inside delta_sum).  A member of a few elements uses a fraction of
// its tile's lanes; that is accepted (DESIGN.md section 5 "Pack").
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

// The inverse.  Every thread of the workgroup calls it (the delta sum has a
// barrier); true when the sum's LDS set was used.  Stores are exactly the
// member's bytes, at the alignment of its elements.
template <int W, bool DELTA>
__device__ __forceinline__ void merge_group(const PackDesc* __restrict__ D, uint64_t g,
                                            const uint8_t* __restrict__ planes, uint64_t* tot) {
    const uint64_t n_elems = D->n_elems;
    const bool active = g < (n_elems + 15u) >> 4;
    uint32_t e[4 * W];
    if (active) {
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
    } else {
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) e[j] = 0;
    }
    if constexpr (DELTA) delta_sum<W>(e, reinterpret_cast<typename Acc<W>::type*>(tot));
    if (!active) return;
    uint8_t* d = reinterpret_cast<uint8_t*>(D->ptr) + g * (16u * W);
    if ((g << 4) + 16u <= n_elems) {
        if constexpr (W == 1) {
            *reinterpret_cast<U128b*>(d) = U128b{e[0], e[1], e[2], e[3]};
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<U128u*>(d + 16 * j) = U128u{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]};
        }
    } else {
        const uint32_t rem = (uint32_t)(n_elems - (g << 4)) * W;  // destination bytes of the group
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

}  // namespace

__global__ __launch_bounds__(PL_T) void pack_split_kernel(const PackDesc* __restrict__ descs, uint32_t n, uint64_t tiles,
                                                          uint8_t* __restrict__ image) {
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const PackDesc* D = descs + member_of(descs, n, tile);
        const uint64_t g = (tile - D->first_tile) * PL_T + threadIdx.x;
        const bool delta = D->kind == FSEHIP_KIND_DELTA;
        switch (D->w) {
            case 1:
                if (delta) split_group<1, true>(D, g, image);
                else split_group<1, false>(D, g, image);
                break;
            case 2:
                if (delta) split_group<2, true>(D, g, image);
                else split_group<2, false>(D, g, image);
                break;
            case 4:
                if (delta) split_group<4, true>(D, g, image);
                else split_group<4, false>(D, g, image);
                break;
            default:
                if (delta) split_group<8, true>(D, g, image);
                else split_group<8, false>(D, g, image);
                break;
        }
    }
}

// `tot` alternates between two sets from one delta tile to the next, as in
// delta_merge_kernel: a wave may write the next delta tile's totals while
// another still reads this one's, and cannot get a delta tile further before
// that one passed the next barrier.  Tiles of the plane kind have no barrier
// and leave the set alone.
__global__ __launch_bounds__(PL_T) void pack_merge_kernel(const PackDesc* __restrict__ descs, uint32_t n, uint64_t tiles,
                                                          const uint8_t* __restrict__ planes,
                                                          const int32_t* __restrict__ result) {
    if (result && *result == FSE_ERR_BAD_FRAME) return;
    __shared__ uint64_t tot[2][PL_T / 64];
    uint32_t set = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const PackDesc* D = descs + member_of(descs, n, tile);
        const uint64_t g = (tile - D->first_tile) * PL_T + threadIdx.x;
        const bool delta = D->kind == FSEHIP_KIND_DELTA;
        switch (D->w) {
            case 1:
                if (delta) merge_group<1, true>(D, g, planes, tot[set]);
                else merge_group<1, false>(D, g, planes, nullptr);
                break;
            case 2:
                if (delta) merge_group<2, true>(D, g, planes, tot[set]);
                else merge_group<2, false>(D, g, planes, nullptr);
                break;
            case 4:
                if (delta) merge_group<4, true>(D, g, planes, tot[set]);
                else merge_group<4, false>(D, g, planes, nullptr);
                break;
            default:
                if (delta) merge_group<8, true>(D, g, planes, tot[set]);
                else merge_group<8, false>(D, g, planes, nullptr);
                break;
        }
        if (delta) set ^= 1u;
    }
}

__global__ __launch_bounds__(PL_T) void pack_finish_kernel(const uint8_t* __restrict__ head, uint64_t head_bytes,
                                                           uint8_t* __restrict__ out, uint64_t* __restrict__ out_len) {
    const uint64_t t = (uint64_t)blockIdx.x * PL_T + threadIdx.x;
    for (uint64_t i = t; i < head_bytes; i += (uint64_t)gridDim.x * PL_T) out[i] = head[i];
    if (t == 0) *out_len += head_bytes;
}

__global__ __launch_bounds__(PL_T) void pack_check_kernel(const uint8_t* __restrict__ head, uint64_t head_bytes,
                                                          const uint8_t* __restrict__ in, int32_t* __restrict__ result,
                                                          bool zero_count) {
    const uint64_t t = (uint64_t)blockIdx.x * PL_T + threadIdx.x;
    bool same = true;
    for (uint64_t i = t; i < head_bytes; i += (uint64_t)gridDim.x * PL_T) same = same && in[i] == head[i];
    if (!same) result[0] = FSE_ERR_BAD_FRAME;
    if (t == 0 && zero_count) result[1] = 0;
}

__global__ __launch_bounds__(PL_T) void pack_bad_fill_kernel(int32_t* __restrict__ result, int32_t* __restrict__ status,
                                                             uint64_t n_status) {
    if (result[0] != FSE_ERR_BAD_FRAME) return;
    const uint64_t t = (uint64_t)blockIdx.x * PL_T + threadIdx.x;
    if (t == 0) result[1] = (int32_t)n_status;
    if (status)
        for (uint64_t i = t; i < n_status; i += (uint64_t)gridDim.x * PL_T) status[i] = FSE_ERR_BAD_FRAME;
}

__global__ __launch_bounds__(PL_T) void pack_member_status_kernel(const PackDesc* __restrict__ descs, uint32_t n_sel,
                                                                  const int32_t* __restrict__ plane_status,
                                                                  int32_t* __restrict__ member_status,
                                                                  int32_t* __restrict__ result) {
    const int32_t frame_st = result[0];
    for (uint64_t s = (uint64_t)blockIdx.x * PL_T + threadIdx.x; s < n_sel; s += (uint64_t)gridDim.x * PL_T) {
        int32_t st = frame_st;
        const uint32_t w = descs[s].n_elems ? descs[s].w : 0u;  // a member without elements has no plane range
        for (uint32_t k = 0; k < w && st == FSE_OK; ++k) st = plane_status[descs[s].status0 + k];
        if (member_status) member_status[s] = st;
        if (st != FSE_OK) atomicAdd(&result[1], 1);
    }
}

namespace {

uint32_t tile_grid(uint64_t tiles) { return (uint32_t)(tiles < PL_MAX_WGS ? tiles : PL_MAX_WGS); }

}  // namespace

int launch_pack_split(const PackDesc* d_descs, uint32_t n, uint64_t tiles, uint8_t* image, void* stream) {
    if (tiles == 0) return FSE_OK;
    hipLaunchKernelGGL(pack_split_kernel, dim3(tile_grid(tiles)), dim3(PL_T), 0, static_cast<hipStream_t>(stream),
                       d_descs, n, tiles, image);
    return done();
}

int launch_pack_merge(const PackDesc* d_descs, uint32_t n, uint64_t tiles, const uint8_t* planes,
                      const int32_t* result, void* stream) {
    if (tiles == 0) return FSE_OK;
    hipLaunchKernelGGL(pack_merge_kernel, dim3(tile_grid(tiles)), dim3(PL_T), 0, static_cast<hipStream_t>(stream),
                       d_descs, n, tiles, planes, result);
    return done();
}

int launch_pack_finish(const uint8_t* d_head, uint64_t head_bytes, uint8_t* out, uint64_t* out_len, void* stream) {
    hipLaunchKernelGGL(pack_finish_kernel, dim3(grid_for(head_bytes)), dim3(PL_T), 0, static_cast<hipStream_t>(stream),
                       d_head, head_bytes, out, out_len);
    return done();
}

int launch_pack_check(const uint8_t* d_head, uint64_t head_bytes, const uint8_t* in, int32_t* result, int32_t* status,
                      uint64_t n_status, bool zero_count, void* stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pack_check_kernel, dim3(grid_for(head_bytes)), dim3(PL_T), 0, hs, d_head, head_bytes, in, result,
                       zero_count);
    if (!zero_count)
        hipLaunchKernelGGL(pack_bad_fill_kernel, dim3(grid_for(n_status ? n_status : 1u)), dim3(PL_T), 0, hs, result,
                           status, n_status);
    return done();
}

int launch_pack_member_status(const PackDesc* d_descs, uint32_t n_sel, const int32_t* plane_status,
                              int32_t* member_status, int32_t* result, void* stream) {
    if (n_sel == 0) return FSE_OK;
    hipLaunchKernelGGL(pack_member_status_kernel, dim3(grid_for(n_sel)), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), d_descs, n_sel, plane_status, member_status, result);
    return done();
}

}  // namespace fsehip
