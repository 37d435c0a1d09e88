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
//   ranges (fsehip_frame_decompress_ranges; blocks listed by the host planner)
//   frame_seek_kernel    record offset, type and length of the listed blocks
//   frame_gather_kernel  frame_unpack_kernel over a list: FSE records only
//   frame_gather_merge_kernel  the listed blocks' statuses
//   frame_pieces_kernel  each piece of a range to its destination: from the
//                        record (RAW, RLE) or the decoded bounce block (FSE)
//   frame_seed_kernel    a direct run's first record offset for frame_scan_kernel
//   frame_range_status_kernel  range statuses from block statuses
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
constexpr uint32_t FR_SEEK_E = 4;      // directory entries per thread and tile of frame_seek_kernel
constexpr uint32_t FR_PIECE_SUB = 8192;  // bytes of a piece per workgroup (frame_pieces_kernel)
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
// Ranges: decode of listed blocks only (fsehip_frame_decompress_ranges)
// ------------------------------------------------------------------------
// One pass over the directory up to the last listed block: the scan of
// frame_scan_kernel over the whole frame instead of a chunk, with the same
// per-entry validation, keeping only the listed blocks' results (a binary
// search in the ascending list finds a block's slot).
__global__ __launch_bounds__(FR_SCAN_T) void frame_seek_kernel(FrameChunk F, FrameRanges R) {
    __shared__ uint64_t sh[FR_SCAN_T / 64u];
    __shared__ uint64_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = *F.base;
    __syncthreads();
    if (carry == 0ull) {  // the frame failed frame_check_kernel: nothing of it is read
        for (uint32_t s = t; s < R.n_listed; s += FR_SCAN_T) {
            R.off[s] = 0ull;
            R.kind[s] = FR_BAD;
            R.clen[s] = 0u;
        }
        return;
    }
    const uint64_t first = R.blocks[0], last = R.blocks[R.n_listed - 1u];
    // one contiguous span (a single range, the whole frame): slots without a search
    const bool span = last - first + 1u == (uint64_t)R.n_listed;
    // FR_SEEK_E consecutive entries per thread: their loads overlap, and a
    // tile's scan and barriers are paid once per FR_SEEK_E * FR_SCAN_T blocks
    for (uint64_t tile = 0; tile <= last; tile += (uint64_t)FR_SEEK_E * FR_SCAN_T) {
        const uint64_t b0 = tile + (uint64_t)FR_SEEK_E * t;
        uint64_t v[FR_SEEK_E], sum = 0;
        uint32_t e[FR_SEEK_E], raw[FR_SEEK_E];
#pragma unroll
        for (uint32_t j = 0; j < FR_SEEK_E; ++j) {
            v[j] = 0;
            e[j] = raw[j] = 0;
            if (b0 + j <= last) {
                raw[j] = raw_len_of(F, b0 + j);
                e[j] = ld_u32(F.frame + FR_HDR + 4ull * (b0 + j));
                v[j] = record_bytes(F, e[j], raw[j]);
            }
            sum += v[j];
        }
        uint64_t total;
        uint64_t at = carry + wg_excl_scan(sum, sh, &total);
#pragma unroll
        for (uint32_t j = 0; j < FR_SEEK_E; ++j) {
            const uint64_t b = b0 + j;
            if (b <= last) {
                uint32_t lo = 0, hi = R.n_listed;
                if (span) lo = hi = b < first ? R.n_listed : (uint32_t)(b - first);
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((uint64_t)R.blocks[mid] < b) lo = mid + 1u; else hi = mid;
                }
                if (lo < R.n_listed && (uint64_t)R.blocks[lo] == b) {
                    const uint32_t type = e[j] >> 30, len = e[j] & 0x3FFFFFFFu;
                    const bool valid = type == FR_RAW   ? len == raw[j]
                                       : type == FR_RLE ? len == 1u
                                       : type == FR_FSE ? len >= 1u && (uint64_t)len <= F.slot_bytes
                                                        : false;
                    R.off[lo] = at;
                    R.kind[lo] = valid ? type : (uint32_t)FR_BAD;
                    R.clen[lo] = valid && type == FR_FSE ? len : 0u;
                }
            }
            at += v[j];
        }
        __syncthreads();
        if (t == 0) carry += total;
        __syncthreads();
    }
}

// The gather form of frame_unpack_kernel: workgroup i takes listed block
// bounce[j0 + i].  Only FSE records move here; RAW and RLE pieces go from the
// record straight to their destinations in frame_pieces_kernel.
__global__ __launch_bounds__(FR_COPY_T) void frame_gather_kernel(FrameChunk F, FrameRanges R, uint32_t j0) {
    const uint32_t i = blockIdx.x;
    if (i >= F.cb) return;
    const uint32_t slot = R.bounce[j0 + i];
    const uint32_t kind = R.kind[slot];
    const uint32_t clen = kind == FR_FSE ? R.clen[slot] : 0u;
    const bool lead = blockIdx.y == 0;
    if (lead && threadIdx.x == 0) F.comp_len[i] = clen;  // 0: the table build fails the block and no decode kernel touches its output
    if (kind != FR_FSE) return;
    const uint32_t raw = raw_len_of(F, R.blocks[slot]);
    const uint8_t* src = F.frame + R.off[slot];
    const uint32_t nck = F.sidecar ? 8u * spb_of(F, raw) : 0u;
    if (lead && nck) copy_span(reinterpret_cast<uint8_t*>(F.sidecar + (uint64_t)i * F.spb), src, nck);
    // the record's bytes in shares of FR_PIECE_SUB, so that a few blocks still fill the chip
    const uint32_t lo = blockIdx.y * FR_PIECE_SUB;
    if (lo < clen) copy_span(F.slots + (uint64_t)i * F.slot_bytes + lo, src + nck + lo, min(FR_PIECE_SUB, clen - lo));
}

__global__ __launch_bounds__(256) void frame_gather_merge_kernel(FrameChunk F, FrameRanges R, uint32_t j0) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= F.cb) return;
    const uint32_t slot = R.bounce[j0 + i];
    const uint32_t kind = R.kind[slot];
    R.status[slot] = kind == FR_FSE ? F.status[i] : kind == FR_BAD ? FSE_ERR_BAD_FRAME : FSE_OK;
}

// Workgroup (x, y) copies bytes [y * FR_PIECE_SUB, (y + 1) * FR_PIECE_SUB) of
// piece p0 + x of the chunk at j0, so that a few long pieces still fill the
// chip.  Stores: exactly the piece's bytes, or none when its block failed.
__global__ __launch_bounds__(FR_COPY_T) void frame_pieces_kernel(FrameChunk F, FrameRanges R, uint32_t j0, uint64_t p0) {
    const FramePiece pc = R.pieces[p0 + blockIdx.x];
    const uint32_t lo = blockIdx.y * FR_PIECE_SUB;
    if (lo >= pc.len) return;
    const uint32_t n = min(FR_PIECE_SUB, pc.len - lo);
    const uint32_t slot = R.bounce[pc.bounce];
    const uint32_t kind = R.kind[slot];
    uint8_t* dst = R.out + pc.dst_off + lo;
    if (kind == FR_RAW) {
        copy_span(dst, F.frame + R.off[slot] + pc.in_off + lo, n);
    } else if (kind == FR_RLE) {
        fill_span(dst, F.frame[R.off[slot]], n);
    } else if (kind == FR_FSE && R.status[slot] == FSE_OK) {
        copy_span(dst, R.raw_bounce + (uint64_t)(pc.bounce - j0) * F.block_size + pc.in_off + lo, n);
    }
}

__global__ void frame_seed_kernel(FrameChunk F, FrameRanges R, uint32_t slot) { *F.base = R.off[slot]; }

// The range-level counterpart of frame_merge_kernel, one workgroup per range
// (a range may span every block of the frame): a range's blocks are
// consecutive slots; the lowest failed one decides.
__global__ __launch_bounds__(256) void frame_range_status_kernel(FrameRanges R, uint32_t n_ranges, int32_t* range_status,
                                                                  int32_t* result) {
    __shared__ uint32_t first_bad;
    const uint32_t none = 0xFFFFFFFFu;
    const int32_t frame_st = result[0];  // BAD_FRAME: every range, the empty ones included
    for (uint32_t r = blockIdx.x; r < n_ranges; r += gridDim.x) {
        if (threadIdx.x == 0) first_bad = none;
        __syncthreads();
        const uint2 s = R.range_slots[r];
        if (frame_st == FSE_OK) {
            uint32_t mine = none;
            for (uint32_t k = threadIdx.x; k < s.y && mine == none; k += 256u)
                if (R.status[s.x + k] != FSE_OK) mine = k;
            if (mine != none) atomicMin(&first_bad, mine);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int32_t st = frame_st != FSE_OK ? frame_st : first_bad != none ? R.status[s.x + first_bad] : FSE_OK;
            if (range_status) range_status[r] = st;
            if (st != FSE_OK) atomicAdd(&result[1], 1);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------
hipError_t launch_frame_seek(const FrameChunk& F, const FrameRanges& R, hipStream_t hs) {
    if (R.n_listed == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_seek_kernel, dim3(1), dim3(FR_SCAN_T), 0, hs, F, R);
    return hipGetLastError();
}
hipError_t launch_frame_gather(const FrameChunk& F, const FrameRanges& R, uint32_t j0, hipStream_t hs) {
    if (F.cb == 0) return hipSuccess;
    const uint32_t ny = (uint32_t)((F.slot_bytes + FR_PIECE_SUB - 1u) / FR_PIECE_SUB);  // comp_len <= slot_bytes
    hipLaunchKernelGGL(frame_gather_kernel, dim3(F.cb, ny), dim3(FR_COPY_T), 0, hs, F, R, j0);
    return hipGetLastError();
}
hipError_t launch_frame_gather_merge(const FrameChunk& F, const FrameRanges& R, uint32_t j0, hipStream_t hs) {
    if (F.cb == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_gather_merge_kernel, dim3((F.cb + 255u) / 256u), dim3(256), 0, hs, F, R, j0);
    return hipGetLastError();
}
hipError_t launch_frame_pieces(const FrameChunk& F, const FrameRanges& R, uint32_t j0, uint64_t p0, uint32_t np,
                               uint32_t max_len, hipStream_t hs) {
    if (np == 0 || max_len == 0) return hipSuccess;
    const uint32_t ny = (max_len + FR_PIECE_SUB - 1u) / FR_PIECE_SUB;  // <= 2^28 / 8192
    hipLaunchKernelGGL(frame_pieces_kernel, dim3(np, ny), dim3(FR_COPY_T), 0, hs, F, R, j0, p0);
    return hipGetLastError();
}
hipError_t launch_frame_seed(const FrameChunk& F, const FrameRanges& R, uint32_t slot, hipStream_t hs) {
    hipLaunchKernelGGL(frame_seed_kernel, dim3(1), dim3(1), 0, hs, F, R, slot);
    return hipGetLastError();
}
hipError_t launch_frame_range_status(const FrameRanges& R, uint32_t n_ranges, int32_t* range_status, int32_t* result,
                                     hipStream_t hs) {
    if (n_ranges == 0) return hipSuccess;
    hipLaunchKernelGGL(frame_range_status_kernel, dim3(min(n_ranges, 1u << 16)), dim3(256), 0, hs, R, n_ranges,
                       range_status, result);
    return hipGetLastError();
}
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
