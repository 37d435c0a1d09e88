// fse_planes_dev.hpp -- the device pieces the plane transforms (fse_planes.hip,
// fsehip.h section 2d), the delta transforms (fse_delta.hip, section 2e) and
// the image histogram (fse_estimate.hip, section 2g) share: the launch shape,
// the under-aligned access types, the byte transposes on v_perm_b32, and the
// group load and the zigzag delta and diff of the element side.  Element i of a 16-element
// group is the dwords [i * W / 4, (i + 1) * W / 4) of the lane's 4 W.
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
struct __attribute__((packed, aligned(1))) U128b {
    uint32_t x, y, z, w;
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

// ---- the element side of the delta transforms (fse_delta.hip) and of the
// image histogram (fse_estimate.hip)

// the integer the sums run in
template <int W>
struct Acc {
    using type = uint32_t;
};
template <>
struct Acc<8> {
    using type = uint64_t;
};

// element i (a constant after unrolling) of the lane's 4 W dwords
template <int W>
__device__ __forceinline__ typename Acc<W>::type get(const uint32_t (&e)[4 * W], int i) {
    if constexpr (W == 1) return (e[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    else if constexpr (W == 2) return (e[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    else if constexpr (W == 4) return e[i];
    else return (uint64_t)e[2 * i] | ((uint64_t)e[2 * i + 1] << 32);
}

// the low 8 W bits of v into element i; the dwords start out zero for W < 4
template <int W>
__device__ __forceinline__ void put(uint32_t (&e)[4 * W], int i, typename Acc<W>::type v) {
    if constexpr (W == 1) e[i >> 2] |= (v & 0xFFu) << (8 * (i & 3));
    else if constexpr (W == 2) e[i >> 1] |= (v & 0xFFFFu) << (16 * (i & 1));
    else if constexpr (W == 4) e[i] = v;
    else {
        e[2 * i] = (uint32_t)v;
        e[2 * i + 1] = (uint32_t)(v >> 32);
    }
}

// The 16 elements of one group at s (aligned to W).  A whole group is W
// 16-byte loads; of the ragged last one, `rem` < 16 W source bytes, whole
// dwords that hold one are loaded (up to roundup(n_elems * W, 4), never
// more) and the rest is zero.
template <int W>
__device__ __forceinline__ void load_group(const uint8_t* __restrict__ s, bool whole, uint32_t rem,
                                           uint32_t (&e)[4 * W]) {
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
}

// the pad of a ragged group, and whatever its last loaded dword held behind
// the source, to zero
template <int W>
__device__ __forceinline__ void zero_pad(uint32_t (&z)[4 * W], uint32_t rem) {
#pragma unroll
    for (int j = 0; j < 4 * W; ++j) {
        if (4u * j >= rem) z[j] = 0;
        else if (4u * j + 4u > rem) z[j] &= (1u << (8u * (rem - 4u * j))) - 1u;
    }
}

// The zigzag deltas z of the group's elements e; the element before the
// lane's first is read at s - W (a line the neighbouring lane loads anyway)
// and is zero at a restart.
template <int W>
__device__ __forceinline__ void delta_zigzag(const uint8_t* __restrict__ s, bool restart, const uint32_t (&e)[4 * W],
                                             uint32_t (&z)[4 * W]) {
    using A = typename Acc<W>::type;
    A prev = 0;
    if (!restart) {
        if constexpr (W == 1) prev = s[-1];
        else if constexpr (W == 2) prev = *reinterpret_cast<const uint16_t*>(s - 2);
        else if constexpr (W == 4) prev = *reinterpret_cast<const uint32_t*>(s - 4);
        else prev = *reinterpret_cast<const uint64_t*>(s - 8);
    }
#pragma unroll
    for (int j = 0; j < 4 * W; ++j) z[j] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const A x = get<W>(e, i);
        const A d = x - prev;
        prev = x;
        put<W>(z, i, (A)(d << 1) ^ (A)(0 - ((d >> (8 * W - 1)) & 1u)));
    }
}

// The diff frame's transform (fse_diff.hip) and its histogram
// (fse_estimate.hip): z = zigzag(x - b) for the N / W * 4 elements of the N
// dwords x and b (N = 4 W: a group of 16; N = W: a quad of 4).  z may be x.
template <int W, int N>
__device__ __forceinline__ void diff_zigzag(const uint32_t (&x)[N], const uint32_t (&b)[N], uint32_t (&z)[N]) {
    using A = typename Acc<W>::type;
    uint32_t xe[4 * W], be[4 * W], ze[4 * W];
#pragma unroll
    for (int j = 0; j < 4 * W; ++j) {
        xe[j] = j < N ? x[j] : 0u;
        be[j] = j < N ? b[j] : 0u;
        ze[j] = 0;
    }
#pragma unroll
    for (int i = 0; i < 4 * N / W; ++i) {
        const A d = get<W>(xe, i) - get<W>(be, i);
        put<W>(ze, i, (A)(d << 1) ^ (A)(0 - ((d >> (8 * W - 1)) & 1u)));
    }
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = ze[j];
}

// The inverse (the diff merges of fse_diff.hip and fse_vpack.hip): x = b +
// unzigzag(z) for the N / W * 4 elements of the N dwords z and b (N = 4 W: a
// group of 16; N = W: a quad of 4).
template <int W, int N>
__device__ __forceinline__ void diff_unzigzag(const uint32_t (&z)[N], const uint32_t (&b)[N], uint32_t (&x)[N]) {
    using A = typename Acc<W>::type;
    uint32_t ze[4 * W], be[4 * W], xe[4 * W];
#pragma unroll
    for (int j = 0; j < 4 * W; ++j) {
        ze[j] = j < N ? z[j] : 0u;
        be[j] = j < N ? b[j] : 0u;
        xe[j] = 0;
    }
#pragma unroll
    for (int i = 0; i < 4 * N / W; ++i) {
        const A v = get<W>(ze, i);
        put<W>(xe, i, get<W>(be, i) + ((v >> 1) ^ (A)(0 - (v & 1u))));
    }
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = xe[j];
}

// workgroups for `items` lanes' worth of work, capped
inline uint32_t grid_for(uint64_t items) {
    return (uint32_t)(items < (uint64_t)PL_MAX_WGS * PL_T ? (items + PL_T - 1u) / PL_T : PL_MAX_WGS);
}

inline int done() { return hipGetLastError() == hipSuccess ? FSE_OK : FSE_ERR_HIP; }

}  // namespace

}  // namespace fsehip
