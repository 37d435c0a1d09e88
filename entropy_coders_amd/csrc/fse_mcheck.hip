// fse_mcheck.hip -- the kernels of the member check record (fsehip.h section
// 2l), gfx950.
//
//   mcheck_units_kernel          one CRC-32 per work unit (up to 64 KiB of one
//                                span), all spans of a descriptor list in one
//                                launch
//   mcheck_combine_kernel        the units of every span combined into its CRC
//   mcheck_build_finish_kernel   the header and the table to the record
//   mcheck_verify_finish_kernel  header on the device == the caller's; span
//                                CRCs against the table: statuses, counts, the
//                                gate word
//   mcheck_gate_kernel           the sealed decode's gate: the pack's own
//                                BAD_FRAME joins the failed bases'
//
// The units kernel is the CRC kernel of fse_check.hip at its 64-lane
// geometry -- a wave per unit, the unit's aligned 16-byte words interleaved
// over the lanes, twenty 1 KiB tables in LDS (fse_crc_dev.hpp) -- driven by a
// device descriptor table instead of spans passed by value: a wave finds its
// unit's span by binary search on first_unit, and keeps it while its next
// units fall into the same span.  Everything a wave decides on is uniform.
// Spans sit at element alignment only; loads are whole aligned 16-byte words
// that hold a content byte, never more.
//
// The combine.  crc(A || B) = crc(A) x^(8 |B|) ^ crc(B), and all units but a
// span's last have one size, so x^(8 * 64 KiB) and the tree's level constants
// are compile-time; only the last step's x^(8 |last unit|) comes with the
// descriptor.  Short spans take a thread each, long ones a workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fse_crc_dev.hpp"
#include "fse_mcheck_host.h"
#include "fse_planes_dev.hpp"

namespace fsehip {

namespace {

constexpr uint32_t MC_T = 256;         // threads per workgroup of the units kernel
constexpr uint32_t MC_MAX_WGS = 2048;  // the capped grid: 8 workgroups per CU
constexpr uint32_t MC_TAB = crc::kLdsTables * 256;
constexpr uint32_t MC_LANES_LOG = 6;  // a unit is read by the whole wave
static_assert(crc::check_lanes_log(kMcheckUnitLog) == MC_LANES_LOG, "the 64-lane stride tables");

__device__ const crc::Tables d_mc_tables = crc::make_tables();
__device__ const crc::Weights d_mc_weights = crc::make_weights();

// x^(8 * unit) and the combine tree's constants: level d joins runs of
// kMcheckRun * 2^d units, a chunk is all kMcheckCombineThreads runs
constexpr uint32_t kXUnit = crc::xpow8(kMcheckUnit);
struct Levels {
    uint32_t x[kMcheckCombineLevels + 1];
};
constexpr Levels make_levels() {
    Levels L{};
    uint32_t x = crc::xpow8(kMcheckUnit * kMcheckRun);
    for (uint32_t d = 0; d <= kMcheckCombineLevels; ++d) {
        L.x[d] = x;
        x = crc::mulmod(x, x);
    }
    return L;
}
__device__ const Levels d_mc_levels = make_levels();
static_assert(kMcheckCombineThreads == 1u << kMcheckCombineLevels, "a tree over a chunk's runs");

__device__ __forceinline__ uint4 mc_load_word(uintptr_t a) { return *reinterpret_cast<const uint4*>(a << 4); }

// the last span whose first unit is at or before `unit`: spans without units
// share their first unit with the next one and are never the last
__device__ __forceinline__ uint32_t span_of(const McheckDesc* __restrict__ descs, uint32_t n, uint64_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (descs[mid].first_unit <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Hdr32 {
    uint8_t b[32];
};

__device__ bool same_header(const Hdr32& hdr, const uint8_t* in) {
    bool same = true;
#pragma unroll
    for (int i = 0; i < 32; ++i) same = same && in[i] == hdr.b[i];
    return same;
}

Hdr32 hdr32(const uint8_t hdr[32]) {
    Hdr32 h;
    for (int i = 0; i < 32; ++i) h.b[i] = hdr[i];
    return h;
}

}  // namespace

__global__ __launch_bounds__(MC_T) void mcheck_units_kernel(const McheckDesc* __restrict__ descs, uint32_t n,
                                                            uint64_t units, uint32_t* __restrict__ unit_crc) {
    __shared__ uint32_t T[MC_TAB];
    // the 16 word tables, then the four of the 64-lane stride
    for (uint32_t i = threadIdx.x; i < MC_TAB; i += MC_T)
        T[i] = (&d_mc_tables.t[0][0])[i < 16u * 256u ? i : i + (MC_LANES_LOG - 4u) * 1024u];
    __syncthreads();

    constexpr uint32_t G = 1u << MC_LANES_LOG;
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t step = (uint64_t)gridDim.x * (MC_T / 64u);

    // the span the wave is in: units [lo, hi)
    uint64_t lo = 0, hi = 0, ptr = 0, bytes = 0;
    uint32_t k_full = 0, k_last = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * (MC_T / 64u) + wave_in_wg; u < units; u += step) {
        if (u >= hi) {
            const uint32_t m = span_of(descs, n, u);
            const McheckDesc& D = descs[m];
            lo = D.first_unit;
            ptr = D.ptr;
            bytes = D.bytes;
            k_full = D.k_full;
            k_last = D.k_last;
            hi = lo + mcheck_units_of(bytes);
        }
        const uint64_t off = (u - lo) << kMcheckUnitLog, left = bytes - off;
        const bool is_last = left <= kMcheckUnit;
        const uint32_t len = is_last ? (uint32_t)left : (uint32_t)kMcheckUnit;
        const uintptr_t s = (uintptr_t)(ptr + off), e = s + len;
        const uintptr_t a0 = s >> 4, a1 = (e - 1u) >> 4;  // the first and the last word; [a0, a1) go to the lanes

        uint32_t st = 0;
        uintptr_t a = a0 + l;
        if (a < a1) {
            uint4 w = mc_load_word(a);
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
                const uint4 w0 = mc_load_word(a), w1 = mc_load_word(a + G), w2 = mc_load_word(a + 2u * G),
                            w3 = mc_load_word(a + 3u * G);
                st = carry(T, st) ^ word16(T, w0);
                st = carry(T, st) ^ word16(T, w1);
                st = carry(T, st) ^ word16(T, w2);
                st = carry(T, st) ^ word16(T, w3);
                mine = a + 3u * G;
                a += 4u * G;
            }
            while (a < a1) {
                const uint4 w0 = mc_load_word(a);
                st = carry(T, st) ^ word16(T, w0);
                mine = a;
                a += G;
            }
            st = crc::mulmod(d_mc_weights.w[a1 - 1u - mine], st);  // to the start of the last word
        }
        for (uint32_t o = 1; o < G; o <<= 1) st ^= __shfl_xor(st, o);

        if (l == 0) {
            // the init value's share, then the last word's bytes one by one
            st ^= is_last ? k_last : k_full;
            const uint4 w = mc_load_word(a1);
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
            const uint32_t b0 = a1 == a0 ? (uint32_t)(s & 15u) : 0u, b1 = (uint32_t)(e - (a1 << 4));
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i)
                if (i >= b0 && i < b1) st = (st >> 8) ^ T[15 * 256 + ((st ^ (wd[i >> 2] >> (8u * (i & 3u)))) & 0xFFu)];
            unit_crc[u] = ~st;
        }
    }
}

__global__ __launch_bounds__(kMcheckCombineThreads) void mcheck_combine_kernel(const McheckDesc* __restrict__ descs,
                                                                               uint32_t n,
                                                                               const uint32_t* __restrict__ unit_crc,
                                                                               uint32_t* __restrict__ span_crc) {
    // M: a state times x^(8 * unit), byte by byte
    __shared__ uint32_t M[1024], red[kMcheckCombineThreads];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 1024u; i += kMcheckCombineThreads) M[i] = crc::mulmod((i & 255u) << (8u * (i >> 8)), kXUnit);
    __syncthreads();
    auto step = [&](uint32_t acc) {
        return M[acc & 0xFFu] ^ M[256 + ((acc >> 8) & 0xFFu)] ^ M[512 + ((acc >> 16) & 0xFFu)] ^ M[768 + (acc >> 24)];
    };

    // short spans: a thread each
    for (uint64_t i = (uint64_t)blockIdx.x * kMcheckCombineThreads + t; i < n;
         i += (uint64_t)gridDim.x * kMcheckCombineThreads) {
        const McheckDesc& D = descs[i];
        const uint64_t units = mcheck_units_of(D.bytes);
        if (units > kMcheckSerialUnits) continue;
        uint32_t acc = 0;
        if (units) {
            const uint32_t* c = unit_crc + D.first_unit;
            for (uint32_t k = 0; k + 1u < (uint32_t)units; ++k) acc = step(acc) ^ c[k];
            acc = crc::mulmod(acc, D.x_last) ^ c[units - 1u];
        }
        span_crc[i] = acc;
    }

    // long spans: a workgroup each.  The full units go in chunks of
    // kMcheckCombineThreads runs of kMcheckRun, aligned to the end of the full
    // units (the first threads of the first chunk may have short or empty runs:
    // ahead of the first unit the state is 0); the last unit, of its own length,
    // comes last.
    constexpr int64_t kChunk = (int64_t)kMcheckRun * kMcheckCombineThreads;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const McheckDesc& D = descs[i];
        const uint64_t units = mcheck_units_of(D.bytes);
        if (units <= kMcheckSerialUnits) continue;  // uniform
        const uint32_t* c = unit_crc + D.first_unit;
        const int64_t full = (int64_t)units - 1;
        const int64_t chunks = (full + kChunk - 1) / kChunk;
        uint32_t total = 0;
        for (int64_t ch = 0; ch < chunks; ++ch) {
            const int64_t end = full - (chunks - 1 - ch) * kChunk - (int64_t)(kMcheckCombineThreads - 1u - t) * kMcheckRun;
            uint32_t acc = 0;
            for (int64_t k = end - kMcheckRun < 0 ? 0 : end - kMcheckRun; k < end; ++k) acc = step(acc) ^ c[k];
            red[t] = acc;
#pragma unroll
            for (uint32_t d = 0; d < kMcheckCombineLevels; ++d) {
                __syncthreads();
                const uint32_t stride = 1u << d;
                if ((t & (2u * stride - 1u)) == 0) red[t] = crc::mulmod(red[t], d_mc_levels.x[d]) ^ red[t + stride];
            }
            if (t == 0) total = crc::mulmod(total, d_mc_levels.x[kMcheckCombineLevels]) ^ red[0];
            __syncthreads();
        }
        if (t == 0) span_crc[i] = crc::mulmod(total, D.x_last) ^ c[full];
    }
}

__global__ __launch_bounds__(PL_T) void mcheck_build_finish_kernel(Hdr32 hdr, const uint32_t* __restrict__ span_crc,
                                                                   uint32_t n, uint32_t with_bases,
                                                                   uint8_t* __restrict__ record,
                                                                   uint64_t* __restrict__ out_len, uint64_t add,
                                                                   const int32_t* __restrict__ result) {
    if (blockIdx.x == 0 && threadIdx.x < 32u) record[threadIdx.x] = hdr.b[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_len && (!result || result[0] == FSE_OK)) *out_len += add;
    uint8_t* table = record + kMcheckHeaderBytes;
    for (uint64_t m = (uint64_t)blockIdx.x * PL_T + threadIdx.x; m < n; m += (uint64_t)gridDim.x * PL_T) {
        reinterpret_cast<U32u*>(table + kMcheckEntryBytes * m)->v = span_crc[m];
        reinterpret_cast<U32u*>(table + kMcheckEntryBytes * m + 4u)->v = with_bases ? span_crc[n + m] : 0u;
    }
}

// one workgroup: the counts need no atomics and no cleared word
__global__ __launch_bounds__(1024) void mcheck_verify_finish_kernel(Hdr32 hdr, const uint8_t* __restrict__ record,
                                                                    const McheckDesc* __restrict__ descs, uint32_t n,
                                                                    uint32_t which, uint32_t active,
                                                                    const uint32_t* __restrict__ span_crc,
                                                                    int32_t* __restrict__ status,
                                                                    int32_t* __restrict__ result, int mode,
                                                                    int32_t* __restrict__ gate) {
    __shared__ uint32_t failed_sum;
    if (threadIdx.x == 0) failed_sum = 0;
    __syncthreads();
    const bool same = same_header(hdr, record);  // uniform: every thread compares the same bytes
    const uint8_t* table = record + kMcheckHeaderBytes + 4u * which;
    uint32_t failed = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 1024u) {
        int32_t st = FSE_OK;
        if (!same) {
            st = FSE_ERR_BAD_FRAME;
        } else if (active) {
            const uint32_t want = reinterpret_cast<const U32u*>(table + (uint64_t)kMcheckEntryBytes * descs[i].member)->v;
            if (span_crc[i] != want) st = FSE_ERR_CHECKSUM;
        }
        if (status) status[i] = st;
        failed += st != FSE_OK ? 1u : 0u;
    }
    if (failed) atomicAdd(&failed_sum, failed);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t count = failed_sum;
    const int32_t st = !same ? FSE_ERR_BAD_FRAME : count ? FSE_ERR_CHECKSUM : FSE_OK;
    if (mode == kMcheckAlone) {
        result[0] = st;
        result[1] = (int32_t)count;
    } else if (mode == kMcheckBases) {
        result[0] = st;
        result[1] = 0;
        result[2] = (int32_t)count;
        result[3] = 0;
        gate[0] = st != FSE_OK ? FSE_ERR_BAD_FRAME : FSE_OK;
    } else {
        result[1] = (int32_t)count;
        if (!same) result[0] = FSE_ERR_BAD_FRAME;
        else if (count && result[0] == FSE_OK) result[0] = FSE_ERR_CHECKSUM;
    }
}

__global__ void mcheck_gate_kernel(const int32_t* __restrict__ result, int32_t* __restrict__ gate) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && result[0] == FSE_ERR_BAD_FRAME) gate[0] = FSE_ERR_BAD_FRAME;
}

int launch_mcheck_units(const McheckDesc* d_descs, uint32_t n, uint64_t units, uint32_t* unit_crc, void* stream) {
    if (n == 0 || units == 0) return FSE_OK;
    const uint64_t wgs = (units + MC_T / 64u - 1u) / (MC_T / 64u);
    hipLaunchKernelGGL(mcheck_units_kernel, dim3((uint32_t)(wgs < MC_MAX_WGS ? wgs : MC_MAX_WGS)), dim3(MC_T), 0,
                       static_cast<hipStream_t>(stream), d_descs, n, units, unit_crc);
    return done();
}

int launch_mcheck_combine(const McheckDesc* d_descs, uint32_t n, uint32_t n_long, const uint32_t* unit_crc,
                          uint32_t* span_crc, void* stream) {
    if (n == 0) return FSE_OK;
    uint64_t wgs = ((uint64_t)n + kMcheckCombineThreads - 1u) / kMcheckCombineThreads;
    if (wgs < n_long) wgs = n_long;
    hipLaunchKernelGGL(mcheck_combine_kernel, dim3((uint32_t)(wgs < MC_MAX_WGS ? wgs : MC_MAX_WGS)),
                       dim3(kMcheckCombineThreads), 0, static_cast<hipStream_t>(stream), d_descs, n, unit_crc, span_crc);
    return done();
}

int launch_mcheck_build_finish(const uint8_t hdr[32], const uint32_t* span_crc, uint32_t n, bool with_bases,
                               uint8_t* record, uint64_t* out_len, uint64_t add, const int32_t* result, void* stream) {
    hipLaunchKernelGGL(mcheck_build_finish_kernel, dim3(n ? grid_for(n) : 1u), dim3(PL_T), 0,
                       static_cast<hipStream_t>(stream), hdr32(hdr), span_crc, n, with_bases ? 1u : 0u, record, out_len,
                       add, result);
    return done();
}

int launch_mcheck_verify_finish(const uint8_t hdr[32], const uint8_t* record, const McheckDesc* d_descs, uint32_t n,
                                int which, bool active, const uint32_t* span_crc, int32_t* status, int32_t* result,
                                int mode, int32_t* gate, void* stream) {
    hipLaunchKernelGGL(mcheck_verify_finish_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), hdr32(hdr),
                       record, d_descs, n, (uint32_t)which, active ? 1u : 0u, span_crc, status, result, mode, gate);
    return done();
}

int launch_mcheck_gate(const int32_t* result, int32_t* gate, void* stream) {
    hipLaunchKernelGGL(mcheck_gate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), result, gate);
    return done();
}

}  // namespace fsehip
