// fse_diff.hip -- the transforms of the diff frame (fsehip.h section 2h),
// gfx950: the zigzag difference of a tensor's elements against a base
// tensor's, fused into the byte-plane split and merge of fse_planes_dev.hpp.
// Bandwidth kernels: every byte crosses HBM once; no LDS, no barrier.
//
//   diff_split_kernel<W>         elements and base -> diff image (pads zeroed)
//   diff_merge_kernel<W>         diff image and base -> elements, a whole tensor
//   diff_merge_pieces_kernel<W>  plane pieces of element ranges and the ranges'
//                                base elements -> the ranges' destinations, any
//                                alignment
//
// A lane takes 16 consecutive elements, as in fse_planes.hip; W = 1 has one
// plane and no transpose.  An element depends on its own base element only:
// no restart, no sum across lanes.  Arithmetic is mod 2^(8 W): 32-bit
// registers truncated for W <= 2, 64-bit at W = 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_elem_host.h"
#include "fse_planes_dev.hpp"

namespace fsehip {

template <int W>
__global__ __launch_bounds__(PL_T) void diff_split_kernel(const uint8_t* __restrict__ src,
                                                          const uint8_t* __restrict__ base, uint64_t n_elems,
                                                          uint8_t* __restrict__ image) {
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t g = (uint64_t)blockIdx.x * PL_T + threadIdx.x; g < groups; g += step) {
        const bool whole = (g << 4) + 16u <= n_elems;
        // source bytes of the group, of either source; in the ragged last one
        // whole dwords that hold one are loaded (up to roundup(n_elems * W, 4)
        // of each, never more)
        const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
        uint32_t x[4 * W], b[4 * W], z[4 * W];
        load_group<W>(src + g * (16u * W), whole, rem, x);
        load_group<W>(base + g * (16u * W), whole, rem, b);
        diff_zigzag<W, 4 * W>(x, b, z);
        if (!whole) zero_pad<W>(z, rem);  // the pad belongs to the image
        if constexpr (W == 1) {
            *reinterpret_cast<uint4*>(image + (g << 4)) = make_uint4(z[0], z[1], z[2], z[3]);
        } else {
            uint32_t p[W][4];
            deinterleave<W>(z, p);
#pragma unroll
            for (int k = 0; k < W; ++k)
                *reinterpret_cast<uint4*>(image + k * stride + (g << 4)) = make_uint4(p[k][0], p[k][1], p[k][2], p[k][3]);
        }
    }
}

// dst may be base itself (the in-place decode), so neither is __restrict__:
// a lane loads its 16 base elements before it stores the same 16, and no
// other lane touches them.
template <int W>
__global__ __launch_bounds__(PL_T) void diff_merge_kernel(const uint8_t* __restrict__ image, const uint8_t* base,
                                                          uint64_t n_elems, uint8_t* dst,
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
        uint32_t z[4 * W];
        if constexpr (W == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = p[0][j];
        } else {
            interleave<W>(p, z);
        }
        const uint8_t* s = base + g * (16u * W);
        uint8_t* d = dst + g * (16u * W);
        uint32_t b[4 * W], e[4 * W];
        // two straight paths, each with its loads, its sums and its stores
        if ((g << 4) + 16u <= n_elems) {
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
            diff_unzigzag<W, 4 * W>(z, b, e);
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<uint4*>(d + 16 * j) = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
        } else {
            // the ragged last group: whole dwords that hold a base byte, up to
            // roundup(n_elems * W, 4); stores of exactly the group's bytes
            const uint32_t rem = (uint32_t)(n_elems - (g << 4)) * W;
            if constexpr (W == 8) {
                // one lane of the grid, at most 15 elements: element by
                // element from the planes' bytes, two dwords each, so that the
                // whole groups' path alone sets the kernel's registers
                for (uint32_t i = 0; 8u * i < rem; ++i) {
                    uint64_t v = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) v |= (uint64_t)image[k * stride + (g << 4) + i] << (8 * k);
                    const uint64_t bv = (uint64_t)reinterpret_cast<const U32u*>(s + 8 * i)->v |
                                        ((uint64_t)reinterpret_cast<const U32u*>(s + 8 * i + 4)->v << 32);
                    const uint64_t x = bv + ((v >> 1) ^ (0 - (v & 1u)));
                    *reinterpret_cast<uint32_t*>(d + 8 * i) = (uint32_t)x;
                    *reinterpret_cast<uint32_t*>(d + 8 * i + 4) = (uint32_t)(x >> 32);
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) b[j] = 4u * j < rem ? reinterpret_cast<const U32u*>(s + 4 * j)->v : 0u;
            diff_unzigzag<W, 4 * W>(z, b, e);
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (4u * j + 4u <= rem) {
                    *reinterpret_cast<uint32_t*>(d + 4 * j) = e[j];
                } else if (4u * j < rem) {  // W <= 2: the last 1..3 bytes
                    if constexpr (W == 2) {
                        *reinterpret_cast<uint16_t*>(d + 4 * j) = (uint16_t)e[j];
                    } else if constexpr (W == 1) {
#pragma unroll
                        for (uint32_t c = 0; c < 3; ++c)
                            if (4u * j + c < rem) d[4 * j + c] = (uint8_t)(e[j] >> (8u * c));
                    }
                }
            }
        }
    }
}

// Element ranges: blockIdx.y picks the range, a lane takes 4 consecutive
// elements of it: W dword loads (one per plane piece; one in all at W = 1), W
// dword loads of the base and W dword stores, at whatever alignment the
// piece, the base and the destination have; the last 1..3 elements of a range
// move element by element, so the loads stay inside the pieces and the base's
// range and the stores are exactly the range's bytes.
template <int W>
__global__ __launch_bounds__(PL_T) void diff_merge_pieces_kernel(const uint8_t* __restrict__ scratch, DiffPieces P,
                                                                 const uint8_t* __restrict__ base,
                                                                 uint8_t* __restrict__ dst,
                                                                 const int32_t* __restrict__ result) {
    using A = typename Acc<W>::type;
    if (*result == FSE_ERR_BAD_FRAME) return;
    const uint32_t r = blockIdx.y;
    const uint64_t count = P.count[r];
    const uint8_t* piece = scratch + P.off[r];
    const uint8_t* from = base + P.src[r] * W;
    uint8_t* out = dst + P.dst[r] * W;
    const uint64_t quads = (count + 3u) >> 2;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t q = (uint64_t)blockIdx.x * PL_T + threadIdx.x; q < quads; q += step) {
        const uint64_t i = q << 2;
        if (i + 4u <= count) {
            uint32_t z[W], b[W], e[W];
            if constexpr (W == 1) {
                z[0] = reinterpret_cast<const U32u*>(piece + i)->v;
            } else {
                uint32_t p[W];
#pragma unroll
                for (int k = 0; k < W; ++k) p[k] = reinterpret_cast<const U32u*>(piece + k * count + i)->v;
                if constexpr (W == 2) {
                    z[0] = perm(p[1], p[0], 0x05010400u);
                    z[1] = perm(p[1], p[0], 0x07030602u);
                } else {
#pragma unroll
                    for (int h = 0; h < W / 4; ++h) {
                        uint32_t t[4];
                        tr4(p[4 * h], p[4 * h + 1], p[4 * h + 2], p[4 * h + 3], t);
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j * (W / 4) + h] = t[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) b[j] = reinterpret_cast<const U32u*>(from + i * W + 4 * j)->v;
            diff_unzigzag<W, W>(z, b, e);
#pragma unroll
            for (int j = 0; j < W; ++j) reinterpret_cast<U32u*>(out + i * W + 4 * j)->v = e[j];
        } else {
            for (uint64_t x = i; x < count; ++x) {
                A v = 0, bv = 0;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    v |= (A)piece[k * count + x] << (8 * k);
                    bv |= (A)from[x * W + k] << (8 * k);
                }
                const A e = bv + ((v >> 1) ^ (A)(0 - (v & 1u)));
#pragma unroll
                for (int k = 0; k < W; ++k) out[x * W + k] = (uint8_t)(e >> (8 * k));
            }
        }
    }
}

int launch_diff_split(uint32_t w, const void* src, const void* base, uint64_t n_elems, uint8_t* image, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((n_elems + 15u) >> 4));
    const uint8_t* s = static_cast<const uint8_t*>(src);
    const uint8_t* b = static_cast<const uint8_t*>(base);
    if (w == 1) hipLaunchKernelGGL(diff_split_kernel<1>, grid, dim3(PL_T), 0, hs, s, b, n_elems, image);
    else if (w == 2) hipLaunchKernelGGL(diff_split_kernel<2>, grid, dim3(PL_T), 0, hs, s, b, n_elems, image);
    else if (w == 4) hipLaunchKernelGGL(diff_split_kernel<4>, grid, dim3(PL_T), 0, hs, s, b, n_elems, image);
    else hipLaunchKernelGGL(diff_split_kernel<8>, grid, dim3(PL_T), 0, hs, s, b, n_elems, image);
    return done();
}

int launch_diff_merge(uint32_t w, const uint8_t* image, const void* base, uint64_t n_elems, void* dst,
                      const int32_t* result, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((n_elems + 15u) >> 4));
    const uint8_t* b = static_cast<const uint8_t*>(base);
    uint8_t* d = static_cast<uint8_t*>(dst);
    if (w == 1) hipLaunchKernelGGL(diff_merge_kernel<1>, grid, dim3(PL_T), 0, hs, image, b, n_elems, d, result);
    else if (w == 2) hipLaunchKernelGGL(diff_merge_kernel<2>, grid, dim3(PL_T), 0, hs, image, b, n_elems, d, result);
    else if (w == 4) hipLaunchKernelGGL(diff_merge_kernel<4>, grid, dim3(PL_T), 0, hs, image, b, n_elems, d, result);
    else hipLaunchKernelGGL(diff_merge_kernel<8>, grid, dim3(PL_T), 0, hs, image, b, n_elems, d, result);
    return done();
}

int launch_diff_pieces(uint32_t w, const uint8_t* scratch, const DiffPieces& P, const void* base, uint8_t* dst,
                       const int32_t* result, void* stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    uint64_t longest = 0;
    for (uint32_t i = 0; i < P.n; ++i) longest = longest > P.count[i] ? longest : P.count[i];
    if (P.n == 0 || longest == 0) return FSE_OK;
    const dim3 grid(grid_for((longest + 3u) >> 2), P.n);
    const uint8_t* b = static_cast<const uint8_t*>(base);
    if (w == 1) hipLaunchKernelGGL(diff_merge_pieces_kernel<1>, grid, dim3(PL_T), 0, hs, scratch, P, b, dst, result);
    else if (w == 2) hipLaunchKernelGGL(diff_merge_pieces_kernel<2>, grid, dim3(PL_T), 0, hs, scratch, P, b, dst, result);
    else if (w == 4) hipLaunchKernelGGL(diff_merge_pieces_kernel<4>, grid, dim3(PL_T), 0, hs, scratch, P, b, dst, result);
    else hipLaunchKernelGGL(diff_merge_pieces_kernel<8>, grid, dim3(PL_T), 0, hs, scratch, P, b, dst, result);
    return done();
}

}  // namespace fsehip
