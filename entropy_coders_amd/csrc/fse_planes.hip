// fse_planes.hip -- the byte-plane transforms of the plane frame (fsehip.h
// section 2d), gfx950.  Bandwidth kernels: no LDS, registers only.
//
//   planes_split_kernel<W>         raw elements -> plane image (pads zeroed)
//   planes_merge_kernel<W>         plane image -> raw elements, a whole tensor
//   planes_merge_pieces_kernel<W>  plane pieces of element ranges -> their
//                                  destinations, any alignment
//   planes_finish_kernel           encode: header bytes and the length
//   planes_check_kernel            decode: header on the device == the caller's
//   planes_range_status_kernel     ranges: w plane statuses -> one per range
//
// Split and merge give a lane 16 consecutive elements: W 16-byte accesses on
// the element side and one aligned 16-byte access per plane on the image
// side; the bytes change places in registers with v_perm_b32 (the transposes
// of fse_planes_dev.hpp, shared with the delta transforms).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_planes_dev.hpp"
#include "fse_elem_host.h"

namespace fsehip {

template <int W>
__global__ __launch_bounds__(PL_T) void planes_split_kernel(const uint8_t* __restrict__ src, uint64_t n_elems,
                                                            uint8_t* __restrict__ image) {
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t g = (uint64_t)blockIdx.x * PL_T + threadIdx.x; g < groups; g += step) {
        const uint8_t* s = src + g * (16u * W);
        uint32_t e[4 * W];
        if ((g << 4) + 16u <= n_elems) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const U128u v = *reinterpret_cast<const U128u*>(s + 16 * j);
                e[4 * j] = v.x;
                e[4 * j + 1] = v.y;
                e[4 * j + 2] = v.z;
                e[4 * j + 3] = v.w;
            }
        } else {
            // the ragged last group: whole dwords that hold a source byte (up to
            // roundup(n_elems * W, 4), never more), the rest zero: the pad
            const uint32_t rem = (uint32_t)(n_elems - (g << 4)) * W;  // source bytes of the group, < 16 W
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                uint32_t v = 0;
                if (4u * j < rem) v = reinterpret_cast<const U32u*>(s + 4 * j)->v;
                if (W == 2 && 4u * j + 2u == rem) v &= 0xFFFFu;  // half a dword left: the other half may be anything
                e[j] = v;
            }
        }
        uint32_t p[W][4];
        deinterleave<W>(e, p);
#pragma unroll
        for (int k = 0; k < W; ++k)
            *reinterpret_cast<uint4*>(image + k * stride + (g << 4)) = make_uint4(p[k][0], p[k][1], p[k][2], p[k][3]);
    }
}

template <int W>
__global__ __launch_bounds__(PL_T) void planes_merge_kernel(const uint8_t* __restrict__ image, uint64_t n_elems,
                                                            uint8_t* __restrict__ dst,
                                                            const int32_t* __restrict__ result) {
    if (result && *result == FSE_ERR_BAD_FRAME) return;
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t g = (uint64_t)blockIdx.x * PL_T + threadIdx.x; g < groups; g += step) {
        uint32_t p[W][4];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(image + k * stride + (g << 4));
            p[k][0] = v.x;
            p[k][1] = v.y;
            p[k][2] = v.z;
            p[k][3] = v.w;
        }
        uint32_t e[4 * W];
        interleave<W>(p, e);
        uint8_t* d = dst + g * (16u * W);
        if ((g << 4) + 16u <= n_elems) {
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<uint4*>(d + 16 * j) = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
        } else {
            const uint32_t rem = (uint32_t)(n_elems - (g << 4)) * W;  // destination bytes of the group
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (4u * j + 4u <= rem) *reinterpret_cast<uint32_t*>(d + 4 * j) = e[j];
                else if (W == 2 && 4u * j + 2u == rem) *reinterpret_cast<uint16_t*>(d + 4 * j) = (uint16_t)e[j];
            }
        }
    }
}

// Element ranges: blockIdx.y picks the range, a lane takes 4 consecutive
// elements of it: W dword loads (one per plane piece) and W dword stores, at
// whatever alignment the piece and the destination have; the last 1..3
// elements of a range move bytewise, so the loads stay inside the pieces and
// the stores are exactly the range's bytes.
template <int W>
__global__ __launch_bounds__(PL_T) void planes_merge_pieces_kernel(const uint8_t* __restrict__ scratch, PlanePieces P,
                                                                   uint8_t* __restrict__ dst,
                                                                   const int32_t* __restrict__ result) {
    if (*result == FSE_ERR_BAD_FRAME) return;
    const uint32_t r = blockIdx.y;
    const uint64_t count = P.count[r];
    const uint8_t* piece = scratch + P.off[r];
    uint8_t* out = dst + P.dst[r] * W;
    const uint64_t quads = (count + 3u) >> 2;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t q = (uint64_t)blockIdx.x * PL_T + threadIdx.x; q < quads; q += step) {
        const uint64_t i = q << 2;
        if (i + 4u <= count) {
            uint32_t p[W];
#pragma unroll
            for (int k = 0; k < W; ++k) p[k] = reinterpret_cast<const U32u*>(piece + k * count + i)->v;
            uint32_t e[W];
            if constexpr (W == 2) {
                e[0] = perm(p[1], p[0], 0x05010400u);
                e[1] = perm(p[1], p[0], 0x07030602u);
            } else {
#pragma unroll
                for (int h = 0; h < W / 4; ++h) {
                    uint32_t t[4];
                    tr4(p[4 * h], p[4 * h + 1], p[4 * h + 2], p[4 * h + 3], t);
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[j * (W / 4) + h] = t[j];
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) reinterpret_cast<U32u*>(out + i * W + 4 * j)->v = e[j];
        } else {
            for (uint64_t x = i; x < count; ++x)
#pragma unroll
                for (int k = 0; k < W; ++k) out[x * W + k] = piece[k * count + x];
        }
    }
}

struct Hdr16 {
    uint8_t b[16];
};

__global__ void planes_finish_kernel(Hdr16 hdr, uint8_t* __restrict__ out, uint64_t* __restrict__ out_len) {
    const uint32_t t = threadIdx.x;
    if (t < 16u) out[t] = hdr.b[t];
    if (t == 0) *out_len += 16u;
}

__global__ __launch_bounds__(PL_T) void planes_check_kernel(Hdr16 hdr, const uint8_t* __restrict__ in,
                                                            int32_t* __restrict__ result,
                                                            int32_t* __restrict__ status, uint64_t n_status,
                                                            bool zero_count) {
    bool same = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) same = same && in[i] == hdr.b[i];
    const uint64_t t = (uint64_t)blockIdx.x * PL_T + threadIdx.x;
    if (t == 0) {
        if (!same) result[0] = FSE_ERR_BAD_FRAME;
        if (zero_count) result[1] = 0;
        else if (!same) result[1] = (int32_t)n_status;
    }
    if (!same && status)
        for (uint64_t i = t; i < n_status; i += (uint64_t)gridDim.x * PL_T) status[i] = FSE_ERR_BAD_FRAME;
}

__global__ __launch_bounds__(PL_T) void planes_range_status_kernel(uint32_t w, const int32_t* __restrict__ plane_status,
                                                                   uint32_t n_ranges, int32_t* __restrict__ range_status,
                                                                   int32_t* __restrict__ result) {
    const int32_t frame_st = result[0];
    for (uint64_t r = (uint64_t)blockIdx.x * PL_T + threadIdx.x; r < n_ranges; r += (uint64_t)gridDim.x * PL_T) {
        int32_t st = frame_st;
        for (uint32_t k = 0; k < w && st == FSE_OK; ++k) st = plane_status[(uint64_t)w * r + k];
        if (range_status) range_status[r] = st;
        if (st != FSE_OK) atomicAdd(&result[1], 1);
    }
}

int launch_planes_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((n_elems + 15u) >> 4));
    const uint8_t* s = static_cast<const uint8_t*>(src);
    if (w == 2) hipLaunchKernelGGL(planes_split_kernel<2>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    else if (w == 4) hipLaunchKernelGGL(planes_split_kernel<4>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    else hipLaunchKernelGGL(planes_split_kernel<8>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    return done();
}

int launch_planes_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                        void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((n_elems + 15u) >> 4));
    uint8_t* d = static_cast<uint8_t*>(dst);
    if (w == 2) hipLaunchKernelGGL(planes_merge_kernel<2>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    else if (w == 4) hipLaunchKernelGGL(planes_merge_kernel<4>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    else hipLaunchKernelGGL(planes_merge_kernel<8>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    return done();
}

int launch_planes_pieces(uint32_t w, const uint8_t* scratch, const PlanePieces& P, uint8_t* dst,
                         const int32_t* result, void* stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    uint64_t longest = 0;
    for (uint32_t i = 0; i < P.n; ++i) longest = longest > P.count[i] ? longest : P.count[i];
    if (P.n == 0 || longest == 0) return FSE_OK;
    const dim3 grid(grid_for((longest + 3u) >> 2), P.n);
    if (w == 2) hipLaunchKernelGGL(planes_merge_pieces_kernel<2>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    else if (w == 4) hipLaunchKernelGGL(planes_merge_pieces_kernel<4>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    else hipLaunchKernelGGL(planes_merge_pieces_kernel<8>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    return done();
}

int launch_elem_finish(const uint8_t hdr[16], uint8_t* out, uint64_t* out_len, void* stream) {
    Hdr16 h;
    for (int i = 0; i < 16; ++i) h.b[i] = hdr[i];
    hipLaunchKernelGGL(planes_finish_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), h, out, out_len);
    return done();
}

int launch_elem_check(const uint8_t hdr[16], const uint8_t* in, int32_t* result, int32_t* status,
                      uint64_t n_status, bool zero_count, void* stream) {
    Hdr16 h;
    for (int i = 0; i < 16; ++i) h.b[i] = hdr[i];
    hipLaunchKernelGGL(planes_check_kernel, dim3(status ? grid_for(n_status ? n_status : 1u) : 1u), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), h, in, result, status, n_status, zero_count);
    return done();
}

int launch_elem_range_status(uint32_t w, const int32_t* plane_status, uint32_t n_ranges, int32_t* range_status,
                             int32_t* result, void* stream) {
    if (n_ranges == 0) return FSE_OK;
    hipLaunchKernelGGL(planes_range_status_kernel, dim3(grid_for(n_ranges)), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), w, plane_status, n_ranges, range_status, result);
    return done();
}

}  // namespace fsehip
