// fse_delta.hip -- the transforms of the delta frame (fsehip.h section 2e),
// gfx950: element delta with a restart every FSEHIP_DELTA_RESTART = 4096
// elements and zigzag, fused into the byte-plane split and merge of
// fse_planes_dev.hpp.  Bandwidth kernels: every byte crosses HBM once.
//
//   delta_split_kernel<W>         raw elements -> delta image (pads zeroed)
//   delta_merge_kernel<W>         delta image -> raw elements, a whole tensor
//   delta_merge_pieces_kernel<W>  plane pieces of element ranges, each from
//                                 its restart group's first element on -> the
//                                 ranges' destinations, any alignment
//
// A lane takes 16 consecutive elements, as in fse_planes.hip; W = 1 has one
// plane and no transpose.  Split needs one element before the lane's own (one
// extra load, a line its neighbour reads anyway; never across a restart).
// Merge is a prefix sum, and the restart bounds it: 256 lanes x 16 elements
// are one restart group, so one workgroup sums one group per iteration -- a
// lane-local sum, a DPP scan of the lane totals inside each wave, the 4 wave
// totals through LDS with one barrier -- and no workgroup ever waits for
// another.  Arithmetic is mod 2^(8 W): 32-bit sums truncated for W <= 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_delta_dev.hpp"
#include "fse_elem_host.h"

namespace fsehip {

namespace {

constexpr uint32_t DL_GROUPS = FSEHIP_DELTA_RESTART / 16;  // 16-element groups in a restart group
static_assert(DL_GROUPS == PL_T, "one workgroup's lanes cover exactly one restart group");

struct __attribute__((packed, aligned(1))) U64b {
    uint32_t x, y;
};
struct __attribute__((packed, aligned(1))) U16b {
    uint16_t v;
};

}  // namespace

template <int W>
__global__ __launch_bounds__(PL_T) void delta_split_kernel(const uint8_t* __restrict__ src, uint64_t n_elems,
                                                           uint8_t* __restrict__ image) {
    using A = typename Acc<W>::type;
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t step = (uint64_t)gridDim.x * PL_T;
    for (uint64_t g = (uint64_t)blockIdx.x * PL_T + threadIdx.x; g < groups; g += step) {
        const uint8_t* s = src + g * (16u * W);
        const bool whole = (g << 4) + 16u <= n_elems;
        // source bytes of the group; in the ragged last one whole dwords that
        // hold one are loaded (up to roundup(n_elems * W, 4), never more)
        const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
        // (the load, the deltas and the pad below are load_group, delta_zigzag
        // and zero_pad of fse_planes_dev.hpp written out: this kernel's code
        // is kept as it was measured)
        uint32_t e[4 * W];
        if (whole) {
            if constexpr (W == 1) {
                const U128b v = *reinterpret_cast<const U128b*>(s);
                e[0] = v.x;
                e[1] = v.y;
                e[2] = v.z;
                e[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const U128u v = *reinterpret_cast<const U128u*>(s + 16 * j);
                    e[4 * j] = v.x;
                    e[4 * j + 1] = v.y;
                    e[4 * j + 2] = v.z;
                    e[4 * j + 3] = v.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) e[j] = 4u * j < rem ? reinterpret_cast<const U32u*>(s + 4 * j)->v : 0u;
        }
        // the element before the lane's first: zero at a restart
        A prev = 0;
        if (g & (DL_GROUPS - 1u)) {
            if constexpr (W == 1) prev = s[-1];
            else if constexpr (W == 2) prev = *reinterpret_cast<const uint16_t*>(s - 2);
            else if constexpr (W == 4) prev = *reinterpret_cast<const uint32_t*>(s - 4);
            else prev = *reinterpret_cast<const uint64_t*>(s - 8);
        }
        uint32_t z[4 * W];
#pragma unroll
        for (int j = 0; j < 4 * W; ++j) z[j] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const A x = get<W>(e, i);
            const A d = x - prev;
            prev = x;
            put<W>(z, i, (A)(d << 1) ^ (A)(0 - ((d >> (8 * W - 1)) & 1u)));
        }
        if (!whole) {
            // the pad, and whatever the last loaded dword held behind the source
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (4u * j >= rem) z[j] = 0;
                else if (4u * j + 4u > rem) z[j] &= (1u << (8u * (rem - 4u * j))) - 1u;
            }
        }
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

// One restart group per workgroup and iteration; the tile loop and the barrier
// inside delta_sum are uniform across the workgroup.  `tot` alternates between
// two sets: a wave may write the next tile's totals while another still reads
// this tile's, and cannot get a tile further before that one passed the next
// barrier.
template <int W>
__global__ __launch_bounds__(PL_T) void delta_merge_kernel(const uint8_t* __restrict__ image, uint64_t n_elems,
                                                           uint8_t* __restrict__ dst,
                                                           const int32_t* __restrict__ result) {
    if (result && *result == FSE_ERR_BAD_FRAME) return;
    __shared__ typename Acc<W>::type tot[2][PL_T / 64];
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t tiles = (groups + DL_GROUPS - 1u) / DL_GROUPS;
    uint32_t set = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, set ^= 1u) {
        const uint64_t g = tile * DL_GROUPS + threadIdx.x;
        const bool active = g < groups;
        uint32_t e[4 * W];
        if (active) {
            load_planes<W>(image, stride, g, e);
        } else {
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) e[j] = 0;
        }
        delta_sum<W>(e, tot[set]);
        if (!active) continue;
        uint8_t* d = dst + g * (16u * W);
        if ((g << 4) + 16u <= n_elems) {
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<uint4*>(d + 16 * j) = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
        } else {
            const uint32_t rem = (uint32_t)(n_elems - (g << 4)) * W;  // destination bytes of the group
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (4u * j + 4u <= rem) {
                    *reinterpret_cast<uint32_t*>(d + 4 * j) = e[j];
                } else if (4u * j < rem) {  // W <= 2: the last 1..3 bytes
                    if constexpr (W == 2) {
                        *reinterpret_cast<uint16_t*>(d + 4 * j) = (uint16_t)e[j];
                    } else if constexpr (W == 1) {
#pragma unroll
                        for (uint32_t b = 0; b < 3; ++b)
                            if (4u * j + b < rem) d[4 * j + b] = (uint8_t)(e[j] >> (8u * b));
                    }
                }
            }
        }
    }
}

// Element ranges: blockIdx.y picks the range, whose plane pieces start at its
// restart group's first element (P.skip elements before the range's own) and
// are 16-byte aligned; blockIdx.x walks the piece's restart groups as the
// whole-tensor kernel does.  Stores are exactly the range's bytes: a lane
// with all 16 elements inside it stores W x 16 bytes at whatever alignment
// the destination has, a lane on an edge element by element.
template <int W>
__global__ __launch_bounds__(PL_T) void delta_merge_pieces_kernel(const uint8_t* __restrict__ scratch, DeltaPieces P,
                                                                  uint8_t* __restrict__ dst,
                                                                  const int32_t* __restrict__ result) {
    if (*result == FSE_ERR_BAD_FRAME) return;
    __shared__ typename Acc<W>::type tot[2][PL_T / 64];
    const uint32_t r = blockIdx.y;
    const uint64_t count = P.count[r], skip = P.skip[r];
    const uint64_t groups = (count + 15u) >> 4, stride = groups << 4;
    const uint64_t tiles = (groups + DL_GROUPS - 1u) / DL_GROUPS;
    const uint8_t* piece = scratch + P.off[r];
    uint8_t* out = dst + P.dst[r] * W;  // where piece element `skip` goes
    uint32_t set = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, set ^= 1u) {
        const uint64_t g = tile * DL_GROUPS + threadIdx.x;
        const bool active = g < groups;
        uint32_t e[4 * W];
        if (active) {
            load_planes<W>(piece, stride, g, e);
        } else {
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) e[j] = 0;
        }
        delta_sum<W>(e, tot[set]);
        if (!active) continue;
        const uint64_t i0 = g << 4;
        if (i0 >= skip && i0 + 16u <= count) {
            uint8_t* d = out + (i0 - skip) * W;
#pragma unroll
            for (int j = 0; j < W; ++j)
                *reinterpret_cast<U128b*>(d + 16 * j) = U128b{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]};
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const uint64_t i = i0 + u;
                if (i < skip || i >= count) continue;
                uint8_t* d = out + (i - skip) * W;
                if constexpr (W == 1) *d = (uint8_t)get<W>(e, u);
                else if constexpr (W == 2) reinterpret_cast<U16b*>(d)->v = (uint16_t)get<W>(e, u);
                else if constexpr (W == 4) reinterpret_cast<U32u*>(d)->v = e[u];
                else *reinterpret_cast<U64b*>(d) = U64b{e[2 * u], e[2 * u + 1]};
            }
        }
    }
}

namespace {

// one workgroup per restart group, capped as the plane kernels' grid
uint32_t tiles_for(uint64_t n_elems) {
    const uint64_t tiles = (n_elems + FSEHIP_DELTA_RESTART - 1u) / FSEHIP_DELTA_RESTART;
    return (uint32_t)(tiles < PL_MAX_WGS ? tiles : PL_MAX_WGS);
}

}  // namespace

int launch_delta_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((n_elems + 15u) >> 4));
    const uint8_t* s = static_cast<const uint8_t*>(src);
    if (w == 1) hipLaunchKernelGGL(delta_split_kernel<1>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    else if (w == 2) hipLaunchKernelGGL(delta_split_kernel<2>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    else if (w == 4) hipLaunchKernelGGL(delta_split_kernel<4>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    else hipLaunchKernelGGL(delta_split_kernel<8>, grid, dim3(PL_T), 0, hs, s, n_elems, image);
    return done();
}

int launch_delta_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                       void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const dim3 grid(tiles_for(n_elems));
    uint8_t* d = static_cast<uint8_t*>(dst);
    if (w == 1) hipLaunchKernelGGL(delta_merge_kernel<1>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    else if (w == 2) hipLaunchKernelGGL(delta_merge_kernel<2>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    else if (w == 4) hipLaunchKernelGGL(delta_merge_kernel<4>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    else hipLaunchKernelGGL(delta_merge_kernel<8>, grid, dim3(PL_T), 0, hs, image, n_elems, d, result);
    return done();
}

int launch_delta_pieces(uint32_t w, const uint8_t* scratch, const DeltaPieces& P, uint8_t* dst, const int32_t* result,
                        void* stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    uint64_t longest = 0;
    for (uint32_t i = 0; i < P.n; ++i) longest = longest > P.count[i] ? longest : P.count[i];
    if (P.n == 0 || longest == 0) return FSE_OK;
    const dim3 grid(tiles_for(longest), P.n);
    if (w == 1) hipLaunchKernelGGL(delta_merge_pieces_kernel<1>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    else if (w == 2) hipLaunchKernelGGL(delta_merge_pieces_kernel<2>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    else if (w == 4) hipLaunchKernelGGL(delta_merge_pieces_kernel<4>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    else hipLaunchKernelGGL(delta_merge_pieces_kernel<8>, grid, dim3(PL_T), 0, hs, scratch, P, dst, result);
    return done();
}

}  // namespace fsehip
