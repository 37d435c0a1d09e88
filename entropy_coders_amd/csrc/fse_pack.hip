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
// its tile's lanes; that is accepted (DESIGN.md section 5 "Pack").  The tile
// search and the group functions live in fse_pack_dev.hpp, shared with the
// versioned pack's kernels (fse_vpack.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_pack_dev.hpp"

namespace fsehip {

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
