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
// side; the bytes change places in registers with v_perm_b32.  Element i of
// a group is the dwords [i * W / 4, (i + 1) * W / 4) of the lane's 4 W.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_planes_host.h"

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

}  // namespace

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

namespace {

uint32_t grid_for(uint64_t items) {
    return (uint32_t)(items < (uint64_t)PL_MAX_WGS * PL_T ? (items + PL_T - 1u) / PL_T : PL_MAX_WGS);
}

int done() { return hipGetLastError() == hipSuccess ? FSE_OK : FSE_ERR_HIP; }

}  // namespace

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

int launch_planes_finish(const uint8_t hdr[16], uint8_t* out, uint64_t* out_len, void* stream) {
    Hdr16 h;
    for (int i = 0; i < 16; ++i) h.b[i] = hdr[i];
    hipLaunchKernelGGL(planes_finish_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), h, out, out_len);
    return done();
}

int launch_planes_check(const uint8_t hdr[16], const uint8_t* in, int32_t* result, int32_t* status,
                        uint64_t n_status, bool zero_count, void* stream) {
    Hdr16 h;
    for (int i = 0; i < 16; ++i) h.b[i] = hdr[i];
    hipLaunchKernelGGL(planes_check_kernel, dim3(status ? grid_for(n_status ? n_status : 1u) : 1u), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), h, in, result, status, n_status, zero_count);
    return done();
}

int launch_planes_range_status(uint32_t w, const int32_t* plane_status, uint32_t n_ranges, int32_t* range_status,
                               int32_t* result, void* stream) {
    if (n_ranges == 0) return FSE_OK;
    hipLaunchKernelGGL(planes_range_status_kernel, dim3(grid_for(n_ranges)), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), w, plane_status, n_ranges, range_status, result);
    return done();
}

}  // namespace fsehip
