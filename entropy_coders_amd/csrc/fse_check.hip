// fse_check.hip -- the kernels of the check record (fsehip.h section 2f),
// gfx950.
//
//   check_crc_kernel<MODE>      one CRC-32 per check block: to the record's
//                               table (build), into the status array (verify),
//                               or compared with the table (ranges)
//   check_build_finish_kernel   the table combined into content_crc, the header
//   check_verify_finish_kernel  header on the device == the caller's; the
//                               computed CRCs combined against content_crc
//   check_status_kernel         computed CRC -> OK / CHECKSUM per check block
//   check_ranges_begin_kernel   ranges: the header check, statuses set
//
// The CRC kernel.  16, 32 or 64 lanes of a wave take a check block
// (crc::check_lanes_log) and read its aligned 16-byte words interleaved, so
// the lanes' loads are contiguous runs of 256 bytes to 1 KiB.  A lane's words
// lie one stride apart, and its state is carried from one to the next by
// table, not by a multiplication: per word 16 lookups for the word's bytes
// (crc::Tables t[0..15]) and 4 for the state's (the stride's set of four, the
// state moved one stride on) -- 20 ds_read_b32 per 16 bytes, the 20 tables in
// LDS.  At the block's end each lane's state is moved to the block's last
// word by one multiplication with x^(128 k) (crc::Weights), the lanes of the
// block are xored together (the CRC is linear), and one lane adds the init
// value's share (a kernel argument: it depends only on the block's length and
// alignment) and walks the last word's 1..16 bytes bytewise.  That per-block
// work is one set of wave instructions for all the blocks a wave holds: 4 of
// them up to 4 KiB, which is why small blocks take 16 lanes.
//
// Leading bytes of a block's first word that belong to the block before are
// zeroed: ahead of the first content byte the state is 0, and zeros leave it
// there.  Loads are whole aligned 16-byte words that hold a content byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_check_host.h"
#include "fse_crc_dev.hpp"
#include "fse_planes_dev.hpp"

namespace fsehip {

namespace {

constexpr uint32_t CK_T = 256;         // threads per workgroup of the CRC kernel
constexpr uint32_t CK_MAX_WGS = 2048;  // the capped grid: 8 workgroups per CU
constexpr uint32_t CK_TAB = crc::kLdsTables * 256;

__device__ const crc::Tables d_tables = crc::make_tables();
__device__ const crc::Weights d_weights = crc::make_weights();

__device__ __forceinline__ uint4 load_word(uintptr_t a) { return *reinterpret_cast<const uint4*>(a << 4); }

}  // namespace

template <int MODE>
__global__ __launch_bounds__(CK_T) void check_crc_kernel(CheckSpans S, const uint8_t* __restrict__ data,
                                                         uint64_t n_content, uint32_t check_log,
                                                         uint8_t* __restrict__ record, int32_t* __restrict__ status,
                                                         uint32_t r0, int32_t* __restrict__ result) {
    __shared__ uint32_t T[CK_TAB];
    const uint32_t lanes_log = crc::check_lanes_log(check_log);
    // the 16 word tables, then the four of this stride
    for (uint32_t i = threadIdx.x; i < CK_TAB; i += CK_T)
        T[i] = (&d_tables.t[0][0])[i < 16u * 256u ? i : i + (lanes_log - 4u) * 1024u];
    __syncthreads();
    if (MODE == kCheckRanges && result[0] == FSE_ERR_BAD_FRAME) return;

    const uint32_t sp = blockIdx.y;
    const uint64_t nb = S.nb[sp], b_first = S.b0[sp];
    const uint32_t B = 1u << check_log;
    const uint32_t G = 1u << lanes_log, per_wave = 64u >> lanes_log;
    const uint32_t lane = threadIdx.x & 63u, l = lane & (G - 1u);
    const uint64_t wave = (uint64_t)blockIdx.x * (CK_T / 64u) + (threadIdx.x >> 6);
    const uint64_t step = (uint64_t)gridDim.x * (CK_T / 64u) * per_wave;
    const uint64_t last_block = (n_content - 1u) >> check_log;  // nb > 0 implies n_content > 0
    const uint8_t* base = data + S.off[sp];

    for (uint64_t u = wave * per_wave + (lane >> lanes_log); u < nb; u += step) {
        const uint64_t b = b_first + u;
        const uint64_t left = n_content - (b << check_log);
        const uint32_t len = left < B ? (uint32_t)left : B;
        const uintptr_t s = reinterpret_cast<uintptr_t>(base + (u << check_log)), e = s + len;
        const uintptr_t a0 = s >> 4, a1 = (e - 1u) >> 4;  // the first and the last word; [a0, a1) go to the lanes

        uint32_t st = 0;
        uintptr_t a = a0 + l;
        if (a < a1) {
            uint4 w = load_word(a);
            if (l == 0) {
                const uint32_t lead = (uint32_t)(s & 15u);
                w.x = mask_lead(w.x, lead, 0);
                w.y = mask_lead(w.y, lead, 1);
                w.z = mask_lead(w.z, lead, 2);
                w.w = mask_lead(w.w, lead, 3);
            }
            st = word16(T, w);
            uintptr_t mine = a;  // the lane's last word
            a += G;
            while (a + 3u * G < a1) {
                const uint4 w0 = load_word(a), w1 = load_word(a + G), w2 = load_word(a + 2u * G),
                            w3 = load_word(a + 3u * G);
                st = carry(T, st) ^ word16(T, w0);
                st = carry(T, st) ^ word16(T, w1);
                st = carry(T, st) ^ word16(T, w2);
                st = carry(T, st) ^ word16(T, w3);
                mine = a + 3u * G;
                a += 4u * G;
            }
            while (a < a1) {
                const uint4 w0 = load_word(a);
                st = carry(T, st) ^ word16(T, w0);
                mine = a;
                a += G;
            }
            st = crc::mulmod(d_weights.w[a1 - 1u - mine], st);  // to the start of the last word
        }
        for (uint32_t o = 1; o < G; o <<= 1) st ^= __shfl_xor(st, o);

        if (l == 0) {
            // the init value's share, then the last word's bytes one by one
            st ^= b == last_block ? S.k_last[sp] : S.k_full[sp];
            const uint4 w = load_word(a1);
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
            const uint32_t lo = a1 == a0 ? (uint32_t)(s & 15u) : 0u, hi = (uint32_t)(e - (a1 << 4));
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i)
                if (i >= lo && i < hi) st = (st >> 8) ^ T[15 * 256 + ((st ^ (wd[i >> 2] >> (8u * (i & 3u)))) & 0xFFu)];
            const uint32_t crc = ~st;
            if (MODE == kCheckBuild) {
                reinterpret_cast<U32u*>(record + kCheckHeaderBytes + 4u * b)->v = crc;
            } else if (MODE == kCheckVerify) {
                status[b] = (int32_t)crc;
            } else {
                const uint32_t want = reinterpret_cast<const U32u*>(record + kCheckHeaderBytes + 4u * b)->v;
                if (crc != want && atomicExch(&status[r0 + sp], FSE_ERR_CHECKSUM) == FSE_OK) atomicAdd(&result[1], 1);
            }
        }
    }
}

namespace {

struct Hdr32 {
    uint8_t b[32];
};

// Every thread of the kCombineThreads: the combine of `n_cb` CRCs read by
// entry(i), in thread 0.  Threads take runs of P.run entries, aligned to the
// end of the n_cb - 1 full blocks' entries (so each run ends a whole number of
// runs ahead of it; the first threads may have short or empty runs), and walk
// them with a multiplication by x^(8 B) made of four table lookups (M, built
// here); a tree then joins the runs, level d multiplying the left half by
// x^(8 B run 2^d); the last block's entry, of its own length, comes last.
template <class Entry>
__device__ uint32_t combine(const CombinePlan& P, uint32_t n_cb, Entry entry, uint32_t* M, uint32_t* red) {
    const uint32_t t = threadIdx.x;
    M[t] = crc::mulmod((t & 255u) << (8u * (t >> 8)), P.x_block);
    __syncthreads();
    const int64_t full = n_cb ? (int64_t)n_cb - 1 : 0;
    const int64_t hi = full - (int64_t)(kCombineThreads - 1u - t) * P.run;
    uint32_t acc = 0;
    for (int64_t i = hi - P.run < 0 ? 0 : hi - P.run; i < hi; ++i)
        acc = M[acc & 0xFFu] ^ M[256 + ((acc >> 8) & 0xFFu)] ^ M[512 + ((acc >> 16) & 0xFFu)] ^ M[768 + (acc >> 24)] ^
              entry((uint64_t)i);
    red[t] = acc;
    for (uint32_t d = 0; d < kCombineLevels; ++d) {
        __syncthreads();
        const uint32_t stride = 1u << d;
        if ((t & (2u * stride - 1u)) == 0) red[t] = crc::mulmod(red[t], P.level[d]) ^ red[t + stride];
    }
    if (t != 0 || n_cb == 0) return 0;
    return crc::mulmod(red[0], P.x_last) ^ entry(n_cb - 1u);
}

__device__ bool same_header(const Hdr32& hdr, const uint8_t* in) {
    bool same = true;
#pragma unroll
    for (int i = 0; i < 32; ++i) same = same && in[i] == hdr.b[i];
    return same;
}

__global__ __launch_bounds__(kCombineThreads) void check_build_finish_kernel(Hdr32 hdr, CombinePlan P, uint32_t n_cb,
                                                                             uint8_t* __restrict__ record) {
    __shared__ uint32_t M[1024], red[kCombineThreads];
    const uint8_t* table = record + kCheckHeaderBytes;
    const uint32_t content =
        combine(P, n_cb, [table](uint64_t i) { return reinterpret_cast<const U32u*>(table + 4u * i)->v; }, M, red);
    if (threadIdx.x != 0) return;
    // bytes 0..19 and the reserved word come from the host; content_crc and header_crc from here
    for (int i = 0; i < 4; ++i) hdr.b[20 + i] = (uint8_t)(content >> (8 * i));
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < 28; ++i) {
        c ^= hdr.b[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? crc::kPoly : 0u);
    }
    c = ~c;
    for (int i = 0; i < 4; ++i) hdr.b[28 + i] = (uint8_t)(c >> (8 * i));
    for (int i = 0; i < 32; ++i) record[i] = hdr.b[i];
}

__global__ __launch_bounds__(kCombineThreads) void check_verify_finish_kernel(Hdr32 hdr, CombinePlan P, uint32_t n_cb,
                                                                              uint32_t content_crc,
                                                                              const uint8_t* __restrict__ record,
                                                                              int32_t* __restrict__ status,
                                                                              int32_t* __restrict__ result) {
    __shared__ uint32_t M[1024], red[kCombineThreads];
    if (!same_header(hdr, record)) {  // uniform: every thread compares the same bytes
        if (threadIdx.x == 0) {
            result[0] = FSE_ERR_BAD_FRAME;
            result[1] = (int32_t)n_cb;
        }
        for (uint64_t i = threadIdx.x; i < n_cb; i += kCombineThreads) status[i] = FSE_ERR_BAD_FRAME;
        return;
    }
    const uint32_t content = combine(P, n_cb, [status](uint64_t i) { return (uint32_t)status[i]; }, M, red);
    if (threadIdx.x == 0) {
        result[0] = content == content_crc ? FSE_OK : FSE_ERR_CHECKSUM;
        result[1] = 0;
    }
}

__global__ __launch_bounds__(PL_T) void check_status_kernel(const uint8_t* __restrict__ record, uint32_t n_cb,
                                                            int32_t* __restrict__ status,
                                                            int32_t* __restrict__ result) {
    if (result[0] == FSE_ERR_BAD_FRAME) return;
    const uint8_t* table = record + kCheckHeaderBytes;
    uint32_t failed = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * PL_T + threadIdx.x; i < n_cb; i += (uint64_t)gridDim.x * PL_T) {
        const bool ok = (uint32_t)status[i] == reinterpret_cast<const U32u*>(table + 4u * i)->v;
        status[i] = ok ? FSE_OK : FSE_ERR_CHECKSUM;
        failed += ok ? 0u : 1u;
    }
    if (failed) atomicAdd(&result[1], (int32_t)failed);
}

__global__ __launch_bounds__(PL_T) void check_ranges_begin_kernel(Hdr32 hdr, const uint8_t* __restrict__ record,
                                                                  uint32_t n_ranges, int32_t* __restrict__ status,
                                                                  int32_t* __restrict__ result) {
    const bool same = same_header(hdr, record);
    if (threadIdx.x == 0) {
        result[0] = same ? FSE_OK : FSE_ERR_BAD_FRAME;
        result[1] = same ? 0 : (int32_t)n_ranges;
    }
    for (uint32_t r = threadIdx.x; r < n_ranges; r += PL_T) status[r] = same ? FSE_OK : FSE_ERR_BAD_FRAME;
}

Hdr32 hdr32(const uint8_t hdr[32]) {
    Hdr32 h;
    for (int i = 0; i < 32; ++i) h.b[i] = hdr[i];
    return h;
}

}  // namespace

int launch_check_crc(int mode, const CheckSpans& S, const uint8_t* data, uint64_t n_content, uint32_t check_log,
                     uint8_t* record, int32_t* status, uint32_t r0, int32_t* result, void* stream) {
    uint64_t most = 0;
    for (uint32_t i = 0; i < S.n; ++i) most = most > S.nb[i] ? most : S.nb[i];
    if (S.n == 0 || most == 0) return FSE_OK;
    const uint32_t lanes_log = crc::check_lanes_log(check_log);
    const uint64_t waves = (most + (64u >> lanes_log) - 1u) / (64u >> lanes_log);
    const uint64_t wgs = (waves + CK_T / 64u - 1u) / (CK_T / 64u);
    const dim3 grid((uint32_t)(wgs < CK_MAX_WGS ? wgs : CK_MAX_WGS), S.n);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (mode == kCheckBuild)
        hipLaunchKernelGGL(check_crc_kernel<kCheckBuild>, grid, dim3(CK_T), 0, hs, S, data, n_content, check_log, record,
                           status, r0, result);
    else if (mode == kCheckVerify)
        hipLaunchKernelGGL(check_crc_kernel<kCheckVerify>, grid, dim3(CK_T), 0, hs, S, data, n_content, check_log, record,
                           status, r0, result);
    else
        hipLaunchKernelGGL(check_crc_kernel<kCheckRanges>, grid, dim3(CK_T), 0, hs, S, data, n_content, check_log, record,
                           status, r0, result);
    return done();
}

int launch_check_build_finish(const fsehip_check_info* info, const CombinePlan& plan, uint8_t* record, void* stream) {
    uint8_t hdr[32];
    if (fsehip_check_write_header(info, hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    hipLaunchKernelGGL(check_build_finish_kernel, dim3(1), dim3(kCombineThreads), 0, static_cast<hipStream_t>(stream),
                       hdr32(hdr), plan, info->n_cb, record);
    return done();
}

int launch_check_verify_finish(const uint8_t hdr[32], const fsehip_check_info* info, const CombinePlan& plan,
                               const uint8_t* record, int32_t* status, int32_t* result, void* stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(check_verify_finish_kernel, dim3(1), dim3(kCombineThreads), 0, hs, hdr32(hdr), plan, info->n_cb,
                       info->content_crc, record, status, result);
    if (const int rc = done()) return rc;
    if (info->n_cb == 0) return FSE_OK;
    hipLaunchKernelGGL(check_status_kernel, dim3(grid_for(info->n_cb)), dim3(PL_T), 0, hs, record, info->n_cb, status,
                       result);
    return done();
}

int launch_check_ranges_begin(const uint8_t hdr[32], const uint8_t* record, uint32_t n_ranges, int32_t* range_status,
                              int32_t* result, void* stream) {
    hipLaunchKernelGGL(check_ranges_begin_kernel, dim3(1), dim3(PL_T), 0, static_cast<hipStream_t>(stream), hdr32(hdr),
                       record, n_ranges, range_status, result);
    return done();
}

}  // namespace fsehip
