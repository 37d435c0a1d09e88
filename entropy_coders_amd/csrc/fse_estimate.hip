// fse_estimate.hip -- the kernels of the size estimate (fsehip.h sections 2g
// and 2i), gfx950.
//
//   image_histogram_kernel<W, DELTA>  raw elements -> the 256-bin counts of
//                                     every block of the plane or delta image,
//                                     without writing the image
//   diff_histogram_kernel<W>          raw elements and the base's -> the same
//                                     of the diff image
//   estimate_blocks_kernel            a block's counts -> the estimated type,
//                                     record bytes, payload bits and table log
//   est_init_kernel                   the containers' fixed bytes
//
// The histogram reads the source once, 16 elements per lane as the transforms
// of fse_planes.hip and fse_delta.hip, and turns them into the lane's 16 bytes
// of each plane in registers.  A workgroup takes a run of whole restart groups
// (tiles of 4,096 elements: no delta crosses a tile, so no workgroup needs
// another's elements, let alone waits for one) and counts each plane in LDS
// sub-histograms of its own.  A plane's counts leave for global memory, one
// atomicAdd per non-zero bin, when the plane's bytes cross into the next image
// block and when the run ends; integer adds commute, so the counts do not
// depend on the order the workgroups arrive in.  A lane's 16 bytes of a plane
// never straddle a block (strides and block sizes are multiples of 16).
// Blocks below one tile (4,096 bytes) would flush several times per tile:
// for them the lanes add to global memory directly, a path for small inputs.
//
// The estimate runs one wave per block: optimal_log2, wave_normalize and
// wave_header_write of fse_device.hpp as the encoder runs them (the header
// only for its length), then the integer cost of fse_estimate_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_device.hpp"
#include "fse_estimate_host.h"
#include "fse_planes_dev.hpp"

namespace fsehip {

namespace {

constexpr uint32_t IH_TILE = PL_T * 16u;  // elements, and bytes of one plane, per tile
static_assert(IH_TILE == FSEHIP_DELTA_RESTART, "a tile is one restart group");

// Sub-histograms per plane: 32 KiB of u32 counters at W >= 2 (4 workgroups
// per CU), the copies of a bin on consecutive banks as in wave_histogram.
template <int W>
constexpr uint32_t ih_copies() {
    return W == 8 ? 4u : W == 4 ? 8u : 16u;
}

// Count a lane's 16 bytes of one plane through add(byte, increment).  Zero
// planes and constant runs put every lane on one bin: 16 equal bytes are one
// add of 16, and (MERGE: every active lane adds to the same histogram) a wave
// whose lanes all hold the same 16 equal bytes adds once.
template <bool MERGE, class Add>
__device__ __forceinline__ void count16(const uint32_t (&q)[4], Add add) {
    const uint32_t b0 = q[0] & 0xFFu;
    const bool same = q[0] == b0 * 0x01010101u && q[1] == q[0] && q[2] == q[0] && q[3] == q[0];
    if constexpr (MERGE) {
        const uint64_t act = __ballot(true);
        const uint32_t bf = __builtin_amdgcn_readfirstlane(b0);
        if (__ballot(same && b0 == bf) == act) {
            if (lane_id() == (uint32_t)__builtin_ctzll(act)) add(bf, 16u * (uint32_t)__popcll(act));
            return;
        }
    }
    if (same) {
        add(b0, 16u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) add((q[j] >> (8 * b)) & 0xFFu, 1u);
    }
}

}  // namespace

// (4 waves per SIMD, 128 VGPRs: 4 workgroups per CU, which the 32 KiB of LDS allow)
template <int W, bool DELTA>
__global__ __launch_bounds__(PL_T) __attribute__((amdgpu_waves_per_eu(4))) void image_histogram_kernel(
    const uint8_t* __restrict__ src, uint64_t n_elems, uint32_t bs, uint32_t tiles_per_wg,
    uint32_t* __restrict__ counts) {
    constexpr uint32_t C = ih_copies<W>();
    __shared__ __attribute__((aligned(16))) uint32_t hist[W * 256u * C];  // [plane][bin][copy]
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t tiles = (groups + PL_T - 1u) / PL_T;
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_wg;
    if (t0 >= tiles) return;
    const uint64_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    const bool direct = bs < IH_TILE;  // several blocks per tile and plane: no LDS
    const uint32_t tid = threadIdx.x;
    uint32_t* const mine = hist + (tid & (C - 1u));

    // plane k's current image block and where it ends, workgroup-uniform
    uint64_t cur[W], bound[W];
    if (!direct) {
        for (uint32_t i = tid; i < W * 256u * C; i += PL_T) hist[i] = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            cur[k] = (k * stride + t0 * IH_TILE) / bs;
            bound[k] = (cur[k] + 1u) * bs;
        }
        __syncthreads();
    }
    // bin `tid` of plane k: its copies summed and cleared, added to block cur[k]
    auto flush = [&](int k) {
        __syncthreads();
        uint32_t* h = hist + (k * 256u + tid) * C;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t c = 0; c < C; c += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(h + c);
            sum += v.x + v.y + v.z + v.w;
            *reinterpret_cast<uint4*>(h + c) = make_uint4(0, 0, 0, 0);
        }
        if (sum) atomicAdd(counts + cur[k] * 256u + tid, sum);
        __syncthreads();
    };

    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t g = tile * PL_T + tid;
        const bool active = g < groups;
        uint32_t p[W][4];
        if (active) {
            const uint8_t* s = src + g * (16u * W);
            const bool whole = (g << 4) + 16u <= n_elems;
            const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
            uint32_t e[4 * W];
            load_group<W>(s, whole, rem, e);
            if constexpr (DELTA) {
                uint32_t z[4 * W];
                delta_zigzag<W>(s, tid == 0u, e, z);  // a tile starts a restart group
                if (!whole) zero_pad<W>(z, rem);
                if constexpr (W == 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[0][j] = z[j];
                } else {
                    deinterleave<W>(z, p);
                }
            } else {
                if (!whole) zero_pad<W>(e, rem);
                if constexpr (W == 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[0][j] = e[j];
                } else {
                    deinterleave<W>(e, p);
                }
            }
        }
        if (direct) {
            if (active) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    uint32_t* c = counts + (k * stride + (g << 4)) / bs * 256u;
                    count16<false>(p[k], [&](uint32_t byte, uint32_t inc) { atomicAdd(c + byte, inc); });
                }
            }
            continue;
        }
        const uint64_t tile_off = tile * IH_TILE;
        const uint64_t tile_len = stride - tile_off < IH_TILE ? stride - tile_off : IH_TILE;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t base = k * stride + tile_off;  // the tile's first byte of plane k in the image
            auto add = [&](uint32_t byte, uint32_t inc) { atomicAdd(mine + (k * 256u + byte) * C, inc); };
            if (base >= bound[k]) {  // the last tile ended on the block's last byte
                flush(k);
                cur[k] += 1u;
                bound[k] += bs;
            }
            // bs >= IH_TILE: the tile's bytes lie in at most two blocks
            const bool first = base + ((uint64_t)tid << 4) < bound[k];
            if (active && first) count16<true>(p[k], add);
            if (base + tile_len > bound[k]) {
                flush(k);
                cur[k] += 1u;
                bound[k] += bs;
                if (active && !first) count16<true>(p[k], add);
            }
        }
    }
    if (!direct) {
#pragma unroll
        for (int k = 0; k < W; ++k) flush(k);
    }
}

// image_histogram_kernel's structure over two sources: the tiles, the
// sub-histograms, the flush and the small-block path are the same, the text is
// its own so that the seven instances above keep their registers.  A lane
// issues the 16-byte loads of its 16 elements and of the base's same 16 before
// it uses either, then takes the diff frame's own zigzag (diff_zigzag of
// fse_planes_dev.hpp, as diff_split_kernel) in place over the source's
// registers.  An element depends on its own base element only: no restart, and
// src and base may overlap in any way (neither is written).  Diff images are
// mostly zero high planes: count16<true> adds such a wave's 1,024 bytes once.
template <int W>
__global__ __launch_bounds__(PL_T) __attribute__((amdgpu_waves_per_eu(4))) void diff_histogram_kernel(
    const uint8_t* src, const uint8_t* base, uint64_t n_elems, uint32_t bs, uint32_t tiles_per_wg,
    uint32_t* __restrict__ counts) {
    constexpr uint32_t C = ih_copies<W>();
    __shared__ __attribute__((aligned(16))) uint32_t hist[W * 256u * C];  // [plane][bin][copy]
    const uint64_t groups = (n_elems + 15u) >> 4, stride = groups << 4;
    const uint64_t tiles = (groups + PL_T - 1u) / PL_T;
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_wg;
    if (t0 >= tiles) return;
    const uint64_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    const bool direct = bs < IH_TILE;
    const uint32_t tid = threadIdx.x;
    uint32_t* const mine = hist + (tid & (C - 1u));

    uint64_t cur[W], bound[W];
    if (!direct) {
        for (uint32_t i = tid; i < W * 256u * C; i += PL_T) hist[i] = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            cur[k] = (k * stride + t0 * IH_TILE) / bs;
            bound[k] = (cur[k] + 1u) * bs;
        }
        __syncthreads();
    }
    auto flush = [&](int k) {
        __syncthreads();
        uint32_t* h = hist + (k * 256u + tid) * C;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t c = 0; c < C; c += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(h + c);
            sum += v.x + v.y + v.z + v.w;
            *reinterpret_cast<uint4*>(h + c) = make_uint4(0, 0, 0, 0);
        }
        if (sum) atomicAdd(counts + cur[k] * 256u + tid, sum);
        __syncthreads();
    };

    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t g = tile * PL_T + tid;
        const bool active = g < groups;
        uint32_t p[W][4];
        if (active) {
            const bool whole = (g << 4) + 16u <= n_elems;
            const uint32_t rem = whole ? 16u * W : (uint32_t)(n_elems - (g << 4)) * W;
            uint32_t x[4 * W], b[4 * W];
            load_group<W>(src + g * (16u * W), whole, rem, x);
            load_group<W>(base + g * (16u * W), whole, rem, b);
            diff_zigzag<W, 4 * W>(x, b, x);
            if (!whole) zero_pad<W>(x, rem);
            if constexpr (W == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) p[0][j] = x[j];
            } else {
                deinterleave<W>(x, p);
            }
        }
        if (direct) {
            if (active) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    uint32_t* c = counts + (k * stride + (g << 4)) / bs * 256u;
                    count16<false>(p[k], [&](uint32_t byte, uint32_t inc) { atomicAdd(c + byte, inc); });
                }
            }
            continue;
        }
        const uint64_t tile_off = tile * IH_TILE;
        const uint64_t tile_len = stride - tile_off < IH_TILE ? stride - tile_off : IH_TILE;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t at = k * stride + tile_off;  // the tile's first byte of plane k in the image
            auto add = [&](uint32_t byte, uint32_t inc) { atomicAdd(mine + (k * 256u + byte) * C, inc); };
            if (at >= bound[k]) {
                flush(k);
                cur[k] += 1u;
                bound[k] += bs;
            }
            const bool first = at + ((uint64_t)tid << 4) < bound[k];
            if (active && first) count16<true>(p[k], add);
            if (at + tile_len > bound[k]) {
                flush(k);
                cur[k] += 1u;
                bound[k] += bs;
                if (active && !first) count16<true>(p[k], add);
            }
        }
    }
    if (!direct) {
#pragma unroll
        for (int k = 0; k < W; ++k) flush(k);
    }
}

// One wave per block.  What the histogram alone decides of the encoder's
// status decides the type: ALL_ZERO_SYMBOL0 is RLE, any other refusal RAW.
__global__ __launch_bounds__(64) void estimate_blocks_kernel(EstBlocks E) {
    __shared__ uint32_t counts[256];
    __shared__ int32_t norm[256];
    __shared__ uint32_t hdrw[HDR_MAX / 4];
    __shared__ int scratch[4];
    const uint32_t lane = lane_id();
    for (uint64_t b = blockIdx.x; b < E.n_blocks; b += gridDim.x) {
        const uint64_t off = b * E.block_size;
        const uint32_t raw = (uint32_t)(E.n_image - off < E.block_size ? E.n_image - off : E.block_size);
        uint32_t tl = 0;
        for (uint32_t s = lane; s < 256u; s += WAVE) {
            const uint32_t c = E.counts[b * 256u + s];
            counts[s] = c;
            if (c) tl = s + 1u;
        }
        tl = wave_max(tl);
        tl = tl == 0u ? 1u : tl;
        wave_sync();
        uint32_t type = 0, L = 0;  // RAW
        uint64_t rec = raw, bits = 0;
        if (raw && counts[0] == raw) {
            type = 1;  // RLE
            rec = 1;
        } else {
            int rc = raw ? FSE_OK : FSE_ERR_EMPTY;
            uint32_t Lreq = E.table_log, slow = 0;
            if (rc == FSE_OK && E.table_log == 0u) rc = optimal_log2(raw, tl, &Lreq);
            if (rc == FSE_OK) rc = wave_normalize(counts, raw, tl, Lreq, norm, &L, &slow, scratch);
            if (rc == FSE_OK && raw < 2u) rc = FSE_ERR_TOO_SHORT;
            if (rc == FSE_OK && L > E.lmax) rc = FSE_ERR_UNSUPPORTED;
            int hl = 0;
            if (rc == FSE_OK) {
                hl = wave_header_write(norm, L, tl, hdrw);
                if (hl < 0) rc = hl;
            }
            if (rc == FSE_OK) {
                uint64_t q = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t s = lane * 4u + k, c = counts[s];
                    if (c) q += (uint64_t)c * cost8(norm[s], L);
                }
                // q < 2^28 * 256 * 15 per lane: the low 20 bits and the rest, summed apart
                const uint64_t Q = ((uint64_t)wave_sum((uint32_t)(q >> 20)) << 20) + wave_sum((uint32_t)q & 0xFFFFFu);
                uint64_t r;
                est_record(Q, L, (uint32_t)hl, raw, E.ckpt_interval, E.nstates, &bits, &r);
                if (r < raw) {
                    type = 2;  // FSE
                    rec = r;
                } else {
                    bits = 0;
                }
            }
            if (type != 2u) L = 0;
        }
        if (lane == 0) {
            if (E.type) E.type[b] = (uint8_t)type;
            if (E.rec) E.rec[b] = (uint32_t)rec;
            if (E.bits) E.bits[b] = (uint32_t)bits;
            if (E.log) E.log[b] = (uint8_t)L;
            atomicAdd(reinterpret_cast<unsigned long long*>(E.total), (unsigned long long)rec);
        }
        wave_sync();  // the next block's counts overwrite this one's
    }
}

__global__ void est_init_kernel(uint64_t* d, uint64_t v0, uint64_t v1, uint64_t v2, uint32_t n) {
    if (threadIdx.x == 0 && n > 0) d[0] = v0;
    if (threadIdx.x == 1 && n > 1) d[1] = v1;
    if (threadIdx.x == 2 && n > 2) d[2] = v2;
}

int launch_est_init(uint64_t* d, const uint64_t v[3], uint32_t n, void* stream) {
    hipLaunchKernelGGL(est_init_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), d, v[0],
                       n > 1 ? v[1] : 0, n > 2 ? v[2] : 0, n);
    return done();
}

int launch_est_blocks(const EstBlocks& E, void* stream) {
    if (E.n_blocks == 0) return FSE_OK;
    const uint32_t grid = E.n_blocks < (1u << 20) ? E.n_blocks : 1u << 20;
    hipLaunchKernelGGL(estimate_blocks_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), E);
    return done();
}

namespace {

template <int W, bool DELTA>
void ih_launch(const uint8_t* src, uint64_t n_elems, uint32_t bs, uint32_t* counts, hipStream_t hs) {
    const uint64_t tiles = (n_elems + IH_TILE - 1u) / IH_TILE;
    const uint32_t grid = (uint32_t)(tiles < PL_MAX_WGS ? tiles : PL_MAX_WGS);
    const uint32_t per = (uint32_t)((tiles + grid - 1u) / grid);
    hipLaunchKernelGGL((image_histogram_kernel<W, DELTA>), dim3(grid), dim3(PL_T), 0, hs, src, n_elems, bs, per,
                       counts);
}

template <int W>
void dh_launch(const uint8_t* src, const uint8_t* base, uint64_t n_elems, uint32_t bs, uint32_t* counts,
               hipStream_t hs) {
    const uint64_t tiles = (n_elems + IH_TILE - 1u) / IH_TILE;
    const uint32_t grid = (uint32_t)(tiles < PL_MAX_WGS ? tiles : PL_MAX_WGS);
    const uint32_t per = (uint32_t)((tiles + grid - 1u) / grid);
    hipLaunchKernelGGL(diff_histogram_kernel<W>, dim3(grid), dim3(PL_T), 0, hs, src, base, n_elems, bs, per, counts);
}

}  // namespace

int launch_diff_histogram(uint32_t w, const void* src, const void* base, uint64_t n_elems, uint32_t block_size,
                          uint32_t* counts, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    const uint8_t* b = static_cast<const uint8_t*>(base);
    if (w == 1) dh_launch<1>(s, b, n_elems, block_size, counts, hs);
    else if (w == 2) dh_launch<2>(s, b, n_elems, block_size, counts, hs);
    else if (w == 4) dh_launch<4>(s, b, n_elems, block_size, counts, hs);
    else dh_launch<8>(s, b, n_elems, block_size, counts, hs);
    return done();
}

int launch_image_histogram(uint32_t w, bool delta, const void* src, uint64_t n_elems, uint32_t block_size,
                           uint32_t* counts, void* stream) {
    if (n_elems == 0) return FSE_OK;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    if (delta) {
        if (w == 1) ih_launch<1, true>(s, n_elems, block_size, counts, hs);
        else if (w == 2) ih_launch<2, true>(s, n_elems, block_size, counts, hs);
        else if (w == 4) ih_launch<4, true>(s, n_elems, block_size, counts, hs);
        else ih_launch<8, true>(s, n_elems, block_size, counts, hs);
    } else {
        if (w == 2) ih_launch<2, false>(s, n_elems, block_size, counts, hs);
        else if (w == 4) ih_launch<4, false>(s, n_elems, block_size, counts, hs);
        else ih_launch<8, false>(s, n_elems, block_size, counts, hs);
    }
    return done();
}

}  // namespace fsehip
