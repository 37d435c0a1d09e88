// fse_check_host.h -- what the check record's translation units share
// (fsehip.h section 2f): the CRC-32 arithmetic, from which the host functions
// of fse_check.cpp, the kernels' tables and every x^(8n) constant are
// generated; the range planner; and the launchers of fse_check.hip, called by
// fse_capi_check.cpp.  Plain C++ with no HIP include (a stream travels as
// void*), so that fse_check.cpp builds with g++ alone.  Not part of the
// public ABI.
#pragma once
#include <stdint.h>

#include "../../include/fsehip.h"

namespace fsehip {
namespace crc {

// CRC-32 as zlib computes it: the reflected polynomial, so bit 31 of a word
// is the coefficient of x^0 and a state's low byte meets the next input byte.
constexpr uint32_t kPoly = 0xEDB88320u;

// a * b mod P
constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
    }
    return p;
}

// x^(8 n) mod P by square and multiply: what n zero bytes do to a state
constexpr uint32_t xpow8(uint64_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1u) r = mulmod(r, sq);
        sq = mulmod(sq, sq);
    }
    return r;
}

// the state one byte leaves behind it, from state 0
constexpr uint32_t byte_state(uint32_t b) {
    for (int i = 0; i < 8; ++i) b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
    return b;
}

// The kernels' tables.  A check block is read by 16, 32 or 64 lanes of a
// wave (lanes_log), each lane taking every (1 << lanes_log)-th 16-byte word,
// so a lane's words lie 256, 512 or 1024 bytes apart:
//   t[j][b],  j < 16:         the state byte b at place j of a word leaves at
//                             the word's end (b, then 15 - j zero bytes);
//   t[16 + 4 s + k][b], k < 4: the state byte k of a lane's state leaves one
//                             stride on, stride = 256 << s (b at place k, then
//                             stride - 1 - k zeros).
// t[15] is the bytewise table.  A kernel holds t[0..15] and the one stride set
// it uses in LDS: kLdsTables tables.
constexpr uint32_t kLanes = 64, kStrides = 3, kTables = 16 + 4 * kStrides, kLdsTables = 20;
struct Tables {
    uint32_t t[kTables][256];
};
constexpr Tables make_tables() {
    Tables T{};
    for (uint32_t b = 0; b < 256; ++b) T.t[15][b] = byte_state(b);
    for (int j = 14; j >= 0; --j)
        for (uint32_t b = 0; b < 256; ++b) T.t[j][b] = (T.t[j + 1][b] >> 8) ^ T.t[15][T.t[j + 1][b] & 0xFFu];
    for (uint32_t s = 0; s < kStrides; ++s) {
        const uint32_t far = xpow8((256u << s) - 4u), base = 16 + 4 * s;
        for (uint32_t b = 0; b < 256; ++b) T.t[base + 3][b] = mulmod(T.t[15][b], far);
        for (int k = 2; k >= 0; --k)
            for (uint32_t b = 0; b < 256; ++b)
                T.t[base + k][b] = (T.t[base + k + 1][b] >> 8) ^ T.t[15][T.t[base + k + 1][b] & 0xFFu];
    }
    return T;
}
// log2 of the lanes that share a check block: 16 up to 4 KiB blocks (so a
// wave holds 4 blocks and its per-block work is shared by 4), 32 at 8 KiB, 64
// above; a lane has at most 16 words below 16 KiB
constexpr uint32_t check_lanes_log(uint32_t check_log) { return check_log <= 12 ? 4u : check_log == 13 ? 5u : 6u; }

// w[k] = x^(128 k): k words between a lane's last word and the block's last (k < lanes)
struct Weights {
    uint32_t w[kLanes];
};
constexpr Weights make_weights() {
    Weights W{};
    W.w[0] = 0x80000000u;
    for (uint32_t k = 1; k < kLanes; ++k) W.w[k] = mulmod(W.w[k - 1], xpow8(16));
    return W;
}

// 0xFFFFFFFF * x^(8 a): a = the bytes of a block of `len` bytes that starts
// `alpha` bytes into a 16-byte word and lie ahead of its last word -- the init
// value's share of the block's CRC
inline uint32_t init_share(uint32_t alpha, uint64_t len) {
    if (!len) return 0xFFFFFFFFu;
    const uint64_t last_word = (alpha + len - 1u) >> 4;
    return mulmod(0xFFFFFFFFu, xpow8(last_word ? 16u * last_word - alpha : 0u));
}

}  // namespace crc

constexpr uint32_t kCheckHeaderBytes = 32;
constexpr uint32_t kCheckLogMin = 8, kCheckLogMax = 16;

// FSE_OK when `info` is what fsehip_check_read_header gives, BAD_ARG otherwise
int check_info_ok(const fsehip_check_info* info);

// The check blocks [*b0, *b0 + *nb) that lie wholly inside the content bytes
// [src_off, src_off + len); the content's last block counts as whole when the
// range ends at n_content.  The caller has checked src_off + len <= n_content.
inline void check_plan_range(uint64_t n_content, uint32_t check_log, uint64_t src_off, uint64_t len, uint64_t* b0,
                             uint64_t* nb) {
    const uint64_t mask = (1ull << check_log) - 1u, end = src_off + len;
    const uint64_t first = (src_off >> check_log) + ((src_off & mask) ? 1u : 0u);
    const uint64_t last = len && end == n_content ? (n_content >> check_log) + ((n_content & mask) ? 1u : 0u)
                                                  : end >> check_log;
    *b0 = first;
    *nb = last > first ? last - first : 0u;
}

// The range rules of fsehip_check_verify_ranges for a destination of out_cap
// bytes, those of fsehip_frame_decompress_ranges: BAD_ARG, DST_TOO_SMALL or
// FSE_OK.
int check_ranges_ok(const fsehip_check_info* info, uint64_t out_cap, const fsehip_frame_range* ranges,
                    uint32_t n_ranges);

// One launch of the CRC kernel: up to kCheckSpans runs of check blocks, passed
// by value as a kernel argument.  Span i: blocks [b0, b0 + nb) of the content,
// the first at data + off[i].  k_full / k_last: 0xFFFFFFFF * x^(8 a), a = the
// bytes of a full block (of the content's last block) ahead of its last
// 16-byte word at that address -- the init value's share of the block's CRC.
constexpr uint32_t kCheckSpans = 32;
struct CheckSpans {
    uint64_t off[kCheckSpans];
    uint32_t b0[kCheckSpans];
    uint32_t nb[kCheckSpans];
    uint32_t k_full[kCheckSpans];
    uint32_t k_last[kCheckSpans];
    uint32_t n;
};
// fills span i of S for nb blocks from b0 whose first byte is data + off
void check_span(CheckSpans* S, uint32_t i, const void* data, uint64_t off, uint64_t b0, uint64_t nb,
                uint64_t n_content, uint32_t check_log);

// What the finish kernels need to combine n_cb block CRCs in a tree: with R =
// run (entries per thread), x^(8 B R 2^d) for each level d, and x^(8 len) of
// the content's last block.
constexpr uint32_t kCombineThreads = 1024, kCombineLevels = 10;
struct CombinePlan {
    uint32_t run;
    uint32_t x_block;  // x^(8 B)
    uint32_t x_last;   // x^(8 * bytes of the last block)
    uint32_t level[kCombineLevels];
};
CombinePlan check_combine_plan(uint64_t n_content, uint32_t check_log, uint32_t n_cb);

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t.
enum CheckMode { kCheckBuild = 0, kCheckVerify = 1, kCheckRanges = 2 };
// build: CRCs to the record's table; verify: computed CRCs into status[];
// ranges: compared with the table, range_status[r0 + i] and result[1] updated
int launch_check_crc(int mode, const CheckSpans& S, const uint8_t* data, uint64_t n_content, uint32_t check_log,
                     uint8_t* record, int32_t* status, uint32_t r0, int32_t* result, void* stream);
// build: content_crc from the table, then the 32 header bytes
int launch_check_build_finish(const fsehip_check_info* info, const CombinePlan& plan, uint8_t* record, void* stream);
// verify: the header on the device against hdr, content_crc against the
// combine of the computed CRCs in status[], then status[] -> OK / CHECKSUM
int launch_check_verify_finish(const uint8_t hdr[32], const fsehip_check_info* info, const CombinePlan& plan,
                               const uint8_t* record, int32_t* status, int32_t* result, void* stream);
// ranges, first: the header against hdr, range statuses and result set
int launch_check_ranges_begin(const uint8_t hdr[32], const uint8_t* record, uint32_t n_ranges, int32_t* range_status,
                              int32_t* result, void* stream);

}  // namespace fsehip
