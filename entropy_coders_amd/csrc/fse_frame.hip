// fse_frame.hip -- the frame's device side (fsehip.h section 2b): directory,
// record offsets and the copies between the frame and the block codec's slot
// layout.  The frame only wraps the encode / decode kernels; it changes none.
//
//   frame_plan_kernel    encode: the encoder rule per block, the directory
//                        entry, an exclusive scan of the record lengths on
//                        top of the running frame offset; the last chunk
//                        writes the header, the length and the result
//   frame_pack_kernel    encode: one workgroup per block -- checkpoints +
//                        slot bytes (FSE), the source bytes (RAW), one byte
//                        (RLE) -- to the record's place in the frame
//   frame_check_kernel   decode, once: header == the caller's info and the
//                        directory's record lengths end at frame_len
//   frame_scan_kernel    decode: validate each entry, record offsets
//   frame_unpack_kernel  decode: FSE records into slot / comp_len / sidecar
//                        scratch, RAW copied and RLE filled into the output
//   frame_merge_kernel   decode: the frame's own status for RAW / RLE / bad
//                        entries, the decoder's for FSE blocks; failures
//
// A frame may start at any byte address, so directory words and the header
// move bytewise and a copy takes 16-byte accesses only where source and
// destination are congruent mod 16; otherwise aligned destination dwords
// come from two aligned source dwords (v_alignbyte), as in copy_blocks_kernel.
#include "fse_kernels.h"

namespace fsehip {

namespace {

constexpr uint32_t FR_HDR = 32;      // header bytes
constexpr uint32_t FR_SCAN_T = 1024;  // threads of the one-workgroup scans
constexpr uint32_t FR_COPY_T = 256;   // threads of the per-block copies
enum : uint32_t { FR_RAW = 0, FR_RLE = 1, FR_FSE = 2, FR_BAD = 3 };

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void st_u32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

__device__ __forceinline__ uint32_t raw_len_of(const FrameChunk& F, uint64_t b) {
    return (uint32_t)min((uint64_t)F.block_size, F.n_total - b * F.block_size);
}
// fsehip_sidecar_per_block_ns of a block of n bytes
__device__ __forceinline__ uint32_t spb_of(const FrameChunk& F, uint32_t n) {
    if (F.ckpt_interval == 0u) return 0u;
    return F.nstates == 1u ? n / F.ckpt_interval + 2u : n / 2u / F.ckpt_interval + 2u;
}

// Exclusive scan of one u64 per thread over the workgroup's FR_SCAN_T
// threads; *total = their sum.  sh: 16 words of LDS.
__device__ __forceinline__ uint64_t wg_excl_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint64_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63u) sh[wv] = incl;
    __syncthreads();
    uint64_t below = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < FR_SCAN_T / 64u; ++w) {
        below += w < wv ? sh[w] : 0u;
        all += sh[w];
    }
    __syncthreads();
    *total = all;
    return below + incl - v;
}

// len bytes from src to dst, any alignments, by the workgroup's FR_COPY_T
// threads.  Stores: exactly [dst, dst + len).  Loads: exactly [src, src + len)
// on the 16-byte path; on the dword path the aligned dwords that hold a byte
// of the source range.
__device__ __forceinline__ void copy_span(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len) {
    const uint32_t t = threadIdx.x;
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
    if (((da ^ sa) & 15u) == 0u) {
        const uint32_t head = min(len, (uint32_t)((16u - (da & 15u)) & 15u));
        if (t < head) dst[t] = src[t];
        const uint32_t nv = (len - head) >> 4;
        const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
        uint4* d4 = reinterpret_cast<uint4*>(dst + head);
        for (uint32_t i = t; i < nv; i += FR_COPY_T) d4[i] = s4[i];
        for (uint32_t i = head + (nv << 4) + t; i < len; i += FR_COPY_T) dst[i] = src[i];
    } else {
        const uint32_t head = min(len, (uint32_t)((4u - (da & 3u)) & 3u));
        if (t < head) dst[t] = src[t];
        const uint32_t nd = (len - head) >> 2;  // whole destination dwords
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
        const uint32_t sh = (uint32_t)((sa + head) & 3u);
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(src + head - sh);
        for (uint32_t i = t; i < nd; i += FR_COPY_T) {
            const uint32_t lo = sw[i];
            // the word above is read only when it carries bytes of this range
            const uint32_t hi = sh ? sw[i + 1u] : 0u;
            dw[i] = __builtin_amdgcn_alignbyte(hi, lo, sh);
        }
        for (uint32_t i = head + (nd << 2) + t; i < len; i += FR_COPY_T) dst[i] = src[i];
    }
}

// len copies of `v` at dst: 16-byte stores with bytewise ends, never past len
__device__ __forceinline__ void fill_span(uint8_t* dst, uint32_t v, uint32_t len) {
    const uint32_t t = threadIdx.x;
    const uint32_t head = min(len, (uint32_t)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
    if (t < head) dst[t] = (uint8_t)v;
    const uint32_t nv = (len - head) >> 4;
    const uint32_t w = v * 0x01010101u;
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (uint32_t i = t; i < nv; i += FR_COPY_T) d4[i] = make_uint4(w, w, w, w);
    for (uint32_t i = head + (nv << 4) + t; i < len; i += FR_COPY_T) dst[i] = (uint8_t)v;
}

}  // namespace

// ------------------------------------------------------------------------
// Encode
// ------------------------------------------------------------------------
__global__ __launch_bounds__(FR_SCAN_T) void frame_plan_kernel(FrameChunk F, FrameHdr hdr, int first, int last,
                                                               uint64_t* frame_len, int32_t* result) {
    __shared__ uint64_t sh[FR_SCAN_T / 64u];
    __shared__ uint64_t carry;
    __shared__ uint32_t not_fse;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        carry = first ? FR_HDR + 4ull * F.n_blocks : *F.base;
        not_fse = 0;
    }
    __syncthreads();
    for (uint32_t tile = 0; tile < F.cb; tile += FR_SCAN_T) {
        const uint32_t i = tile + t;
        uint64_t v = 0;
        if (i < F.cb) {
            const uint64_t b = (uint64_t)F.c0 + i;
            const uint32_t raw = raw_len_of(F, b);
            const uint32_t clen = F.comp_len[i];
            const int32_t st = F.status[i];
            const uint64_t rec = (uint64_t)clen + 8ull * spb_of(F, raw);
            uint32_t type = FR_RAW, stored = raw;
            v = raw;
            if (st == FSE_ERR_ALL_ZERO_SYMBOL0) {
                type = FR_RLE;
                stored = 1u;
                v = 1u;
            } else if (st == FSE_OK && rec < (uint64_t)raw) {
                type = FR_FSE;
                stored = clen;
                v = rec;
            }
            F.kind[i] = type;
            st_u32(F.frame + FR_HDR + 4ull * b, (type << 30) | stored);
            if (type != FR_FSE) atomicAdd(&not_fse, 1u);
        }
        uint64_t total;
        const uint64_t excl = wg_excl_scan(v, sh, &total);
        if (i < F.cb) F.off[i] = carry + excl;
        __syncthreads();
        if (t == 0) carry += total;
        __syncthreads();
    }
    if (t == 0) {
        *F.base = carry;
        result[1] = (first ? 0 : result[1]) + (int32_t)not_fse;
        if (last) {
            *frame_len = carry;
            result[0] = FSE_OK;
        }
    }
    if (last && t < 8u) st_u32(F.frame + 4u * t, hdr.w[t]);
}

__global__ __launch_bounds__(FR_COPY_T) void frame_pack_kernel(FrameChunk F) {
    const uint32_t i = blockIdx.x;
    if (i >= F.cb) return;
    const uint64_t b = (uint64_t)F.c0 + i;
    const uint32_t raw = raw_len_of(F, b);
    const uint32_t type = F.kind[i];
    uint8_t* dst = F.frame + F.off[i];
    if (type == FR_FSE) {
        const uint32_t nck = F.sidecar ? 8u * spb_of(F, raw) : 0u;
        if (nck) copy_span(dst, reinterpret_cast<const uint8_t*>(F.sidecar + (uint64_t)i * F.spb), nck);
        copy_span(dst + nck, F.slots + (uint64_t)i * F.slot_bytes, F.comp_len[i]);
    } else if (type == FR_RAW) {
        copy_span(dst, F.raw + b * F.block_size, raw);
    } else if (threadIdx.x == 0) {
        dst[0] = 0;  // RLE: the encoder stores all-zero blocks only
    }
}

// ------------------------------------------------------------------------
// Decode
// ------------------------------------------------------------------------
// The bytes of entry e's record: stored_len, plus the checkpoints of a type-2
// entry -- whether or not the entry is valid, so that offsets stay defined
// and only a bad entry's own block is lost.
__device__ __forceinline__ uint64_t record_bytes(const FrameChunk& F, uint32_t e, uint32_t raw) {
    const uint32_t type = e >> 30, len = e & 0x3FFFFFFFu;
    return (uint64_t)len + (type == FR_FSE ? 8ull * spb_of(F, raw) : 0ull);
}

__global__ __launch_bounds__(FR_SCAN_T) void frame_check_kernel(FrameChunk F, FrameHdr hdr, int32_t* result) {
    __shared__ uint64_t sh[FR_SCAN_T / 64u];
    __shared__ uint32_t bad;
    const uint32_t t = threadIdx.x;
    const uint64_t rec_off = FR_HDR + 4ull * F.n_blocks;
    if (t == 0) bad = F.frame_len < rec_off ? 1u : 0u;
    __syncthreads();
    // nothing of the frame is read unless header and directory lie inside it
    if (!bad && t < 8u && ld_u32(F.frame + 4u * t) != hdr.w[t]) atomicOr(&bad, 1u);
    uint64_t sum = 0;
    if (F.frame_len >= rec_off)
        for (uint64_t b = t; b < F.n_blocks; b += FR_SCAN_T)
            sum += record_bytes(F, ld_u32(F.frame + FR_HDR + 4ull * b), raw_len_of(F, b));
    uint64_t total;
    (void)wg_excl_scan(sum, sh, &total);  // syncs: `bad` is complete after it
    if (t == 0) {
        const bool ok = !bad && rec_off + total == F.frame_len;
        *F.base = ok ? rec_off : 0ull;
        result[0] = ok ? FSE_OK : FSE_ERR_BAD_FRAME;
        result[1] = 0;
    }
}

__global__ __launch_bounds__(FR_SCAN_T) void frame_scan_kernel(FrameChunk F) {
    __shared__ uint64_t sh[FR_SCAN_T / 64u];
    __shared__ uint64_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = *F.base;
    __syncthreads();
    const bool ok = carry != 0ull;  // 0: the frame failed frame_check_kernel
    for (uint32_t tile = 0; tile < F.cb; tile += FR_SCAN_T) {
        const uint32_t i = tile + t;
        uint64_t v = 0;
        if (i < F.cb) {
            uint32_t kind = FR_BAD, clen = 0;
            if (ok) {
                const uint64_t b = (uint64_t)F.c0 + i;
                const uint32_t raw = raw_len_of(F, b);
                const uint32_t e = ld_u32(F.frame + FR_HDR + 4ull * b);
                const uint32_t type = e >> 30, len = e & 0x3FFFFFFFu;
                v = record_bytes(F, e, raw);
                const bool valid = type == FR_RAW   ? len == raw
                                   : type == FR_RLE ? len == 1u
                                   : type == FR_FSE ? len >= 1u && (uint64_t)len <= F.slot_bytes
                                                    : false;
                if (valid) kind = type;
                if (kind == FR_FSE) clen = len;
            }
            F.kind[i] = kind;
            F.comp_len[i] = clen;  // 0: the table build fails the block and no decode kernel touches its output
        }
        uint64_t total;
        const uint64_t excl = wg_excl_scan(v, sh, &total);
        if (i < F.cb) F.off[i] = carry + excl;
        __syncthreads();
        if (t == 0) carry += total;
        __syncthreads();
    }
    if (t == 0) *F.base = ok ? carry : 0ull;
}

__global__ __launch_bounds__(FR_COPY_T) void frame_unpack_kernel(FrameChunk F) {
    const uint32_t i = blockIdx.x;
    if (i >= F.cb) return;
    const uint32_t kind = F.kind[i];
    if (kind == FR_BAD) return;
    const uint64_t b = (uint64_t)F.c0 + i;
    const uint32_t raw = raw_len_of(F, b);
    // frame_check_kernel proved every record inside [0, frame_len)
    const uint8_t* src = F.frame + F.off[i];
    if (kind == FR_FSE) {
        const uint32_t nck = F.sidecar ? 8u * spb_of(F, raw) : 0u;
        if (nck) copy_span(reinterpret_cast<uint8_t*>(F.sidecar + (uint64_t)i * F.spb), src, nck);
        copy_span(F.slots + (uint64_t)i * F.slot_bytes, src + nck, F.comp_len[i]);
    } else if (kind == FR_RAW) {
        copy_span(F.raw + b * F.block_size, src, raw);
    } else {
        fill_span(F.raw + b * F.block_size, src[0], raw);
    }
}

__global__ __launch_bounds__(256) void frame_merge_kernel(FrameChunk F, int32_t* block_status, int32_t* result) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= F.cb) return;
    const uint32_t kind = F.kind[i];
    const int32_t st = kind == FR_FSE ? F.status[i] : kind == FR_BAD ? FSE_ERR_BAD_FRAME : FSE_OK;
    if (block_status) block_status[(uint64_t)F.c0 + i] = st;
    if (st != FSE_OK) atomicAdd(&result[1], 1);
}

// ------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------
hipError_t launch_frame_plan(const FrameChunk& F, const FrameHdr& hdr, bool first, bool last, uint64_t* frame_len,
                             int32_t* result, hipStream_t hs) {
    hipLaunchKernelGGL(frame_plan_kernel, dim3(1), dim3(FR_SCAN_T), 0, hs, F, hdr, first ? 1 : 0, last ? 1 : 0, frame_len,
                       result);
    return hipGetLastError();
}
hipError_t launch_frame_pack(const FrameChunk& F, hipStream_t hs) {
    if (F.cb == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_pack_kernel, dim3(F.cb), dim3(FR_COPY_T), 0, hs, F);
    return hipGetLastError();
}
hipError_t launch_frame_check(const FrameChunk& F, const FrameHdr& hdr, int32_t* result, hipStream_t hs) {
    hipLaunchKernelGGL(frame_check_kernel, dim3(1), dim3(FR_SCAN_T), 0, hs, F, hdr, result);
    return hipGetLastError();
}
hipError_t launch_frame_scan(const FrameChunk& F, hipStream_t hs) {
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(FR_SCAN_T), 0, hs, F);
    return hipGetLastError();
}
hipError_t launch_frame_unpack(const FrameChunk& F, hipStream_t hs) {
    if (F.cb == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_unpack_kernel, dim3(F.cb), dim3(FR_COPY_T), 0, hs, F);
    return hipGetLastError();
}
hipError_t launch_frame_merge(const FrameChunk& F, int32_t* block_status, int32_t* result, hipStream_t hs) {
    if (F.cb == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_merge_kernel, dim3((F.cb + 255u) / 256u), dim3(256), 0, hs, F, block_status, result);
    return hipGetLastError();
}

}  // namespace fsehip
