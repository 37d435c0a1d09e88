// fse_check.cpp -- the check record's header, sizes, CRC-32 and range planner,
// host side (fsehip.h section 2f).
//
// Plain C++ with no HIP include, as fse_elem.cpp: the same source builds
// into libfsehip.so and, with g++ alone, into the sanitizer fuzz of
// tests/native/check_fuzz.cpp.  The kernels are fse_check.hip, the device
// calls fse_capi_check.cpp; their tables and constants come from
// fse_check_host.h, as the functions here do.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/fsehip.h"
#include "fse_check_host.h"

namespace {

using namespace fsehip;

constexpr crc::Tables kTab = crc::make_tables();

uint32_t get32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
void put32(uint8_t* p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// n_cb = ceil(n_content / check_block), false when it does not fit a u32
bool blocks_of(uint64_t n_content, uint32_t check_log, uint32_t* n_cb) {
    const uint64_t n = (n_content >> check_log) + ((n_content & ((1ull << check_log) - 1u)) ? 1u : 0u);
    if (n > 0xFFFFFFFFull) return false;
    *n_cb = (uint32_t)n;
    return true;
}

bool fields_ok(const fsehip_check_info& f) {
    uint32_t n_cb;
    return f.version == 1u && f.algorithm == FSEHIP_CHECK_CRC32 && f.check_log >= kCheckLogMin &&
           f.check_log <= kCheckLogMax && f.reserved == 0u && blocks_of(f.n_content, f.check_log, &n_cb) &&
           n_cb == f.n_cb && (f.n_content || f.content_crc == 0u);
}

void header_bytes(const fsehip_check_info& f, uint8_t hdr[32]) {
    hdr[0] = 'F';
    hdr[1] = 'S';
    hdr[2] = 'E';
    hdr[3] = 'K';
    hdr[4] = (uint8_t)f.version;
    hdr[5] = (uint8_t)f.algorithm;
    hdr[6] = (uint8_t)f.check_log;
    hdr[7] = 0;
    for (int i = 0; i < 8; ++i) hdr[8 + i] = (uint8_t)(f.n_content >> (8 * i));
    put32(hdr + 16, f.n_cb);
    put32(hdr + 20, f.content_crc);
    put32(hdr + 24, 0);
    put32(hdr + 28, fsehip_crc32(0, hdr, 28));
}

}  // namespace

extern "C" {

uint32_t fsehip_crc32(uint32_t crc, const uint8_t* buf, size_t n) {
    if (!buf) return 0;  // zlib's convention: the initial value
    uint32_t c = ~crc;
    for (size_t i = 0; i < n; ++i) c = (c >> 8) ^ kTab.t[15][(c ^ buf[i]) & 0xFFu];
    return ~c;
}

uint32_t fsehip_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
    return crc::mulmod(crc::xpow8(len2), crc1) ^ crc2;
}

uint64_t fsehip_check_bytes(uint64_t n_content, uint32_t check_log) {
    if (check_log == 0) check_log = kCheckLogMax;
    uint32_t n_cb;
    if (check_log < kCheckLogMin || check_log > kCheckLogMax || !blocks_of(n_content, check_log, &n_cb)) return 0;
    return kCheckHeaderBytes + 4ull * n_cb;
}

int fsehip_check_read_header(const uint8_t* hdr, size_t len, fsehip_check_info* out) {
    if (!out || (!hdr && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (len < kCheckHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (hdr[0] != 'F' || hdr[1] != 'S' || hdr[2] != 'E' || hdr[3] != 'K') return FSE_ERR_BAD_FRAME;
    fsehip_check_info f;
    memset(&f, 0, sizeof(f));
    f.version = hdr[4];
    f.algorithm = hdr[5];
    f.check_log = hdr[6];
    f.reserved = (uint32_t)hdr[7] | get32(hdr + 24);  // the spare byte and the reserved word: both zero
    for (int i = 7; i >= 0; --i) f.n_content = (f.n_content << 8) | hdr[8 + i];
    f.n_cb = get32(hdr + 16);
    f.content_crc = get32(hdr + 20);
    f.header_crc = get32(hdr + 28);
    if (!fields_ok(f) || f.header_crc != fsehip_crc32(0, hdr, 28)) return FSE_ERR_BAD_FRAME;
    *out = f;
    return FSE_OK;
}

int fsehip_check_write_header(const fsehip_check_info* info, uint8_t hdr[32]) {
    if (!info || !hdr || !fields_ok(*info)) return FSE_ERR_BAD_ARG;
    header_bytes(*info, hdr);
    return FSE_OK;
}

int fsehip_sealed_read_header(const uint8_t* buf, size_t len, fsehip_check_info* info, uint32_t* kind,
                              uint64_t* inner_off) {
    if (!info || !kind || !inner_off || (!buf && len)) return FSE_ERR_BAD_ARG;
    *kind = 0;
    *inner_off = 0;
    fsehip_check_info f;
    const int rc = fsehip_check_read_header(buf, len, &f);
    memset(info, 0, sizeof(*info));
    if (rc != FSE_OK) return rc;
    const uint64_t off = kCheckHeaderBytes + 4ull * f.n_cb;
    if (len < off || len - off < 4u) return FSE_ERR_BAD_FRAME;
    const uint8_t* in = buf + off;
    const size_t left = len - (size_t)off;
    if (in[0] != 'F' || in[1] != 'S' || in[2] != 'E') return FSE_ERR_BAD_FRAME;
    // Only the container's magic and content length are read here (this file
    // stands alone); its own reader validates the rest of its header.
    uint64_t content = 0;
    uint32_t k = 0;
    if (in[3] == 'F') {
        if (left < 32u) return FSE_ERR_BAD_FRAME;
        k = FSEHIP_SEALED_FRAME;
        for (int i = 7; i >= 0; --i) content = (content << 8) | in[16 + i];  // n_total
    } else if (in[3] == 'P' || in[3] == 'D' || in[3] == 'B') {
        if (left < 48u) return FSE_ERR_BAD_FRAME;
        k = in[3] == 'P' ? FSEHIP_SEALED_PLANES : in[3] == 'D' ? FSEHIP_SEALED_DELTA : FSEHIP_SEALED_DIFF;
        const uint64_t w = in[5];
        uint64_t n_elems = 0;
        for (int i = 7; i >= 0; --i) n_elems = (n_elems << 8) | in[8 + i];
        if (w == 0 || w > 8u || n_elems > UINT64_MAX / w) return FSE_ERR_BAD_FRAME;
        content = n_elems * w;
    } else {
        return FSE_ERR_BAD_FRAME;
    }
    if (content != f.n_content) return FSE_ERR_BAD_FRAME;
    *info = f;
    *kind = k;
    *inner_off = off;
    return FSE_OK;
}

int fsehip_check_ranges_verified_bytes(const fsehip_check_info* info, const fsehip_frame_range* ranges,
                                       uint32_t n_ranges, uint64_t* bytes) {
    if (!bytes) return FSE_ERR_BAD_ARG;
    *bytes = 0;
    if (check_info_ok(info) != FSE_OK || (n_ranges && !ranges)) return FSE_ERR_BAD_ARG;
    const uint64_t n = info->n_content, B = 1ull << info->check_log;
    uint64_t sum = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_frame_range& g = ranges[r];
        if (g.src_off + g.len < g.src_off || g.src_off + g.len > n) return FSE_ERR_BAD_ARG;
        uint64_t b0, nb;
        check_plan_range(n, info->check_log, g.src_off, g.len, &b0, &nb);
        if (!nb) continue;
        const uint64_t covered = std::min(n, (b0 + nb) * B) - b0 * B;  // at most len: no overflow
        if (covered > UINT64_MAX - sum) return FSE_ERR_BAD_ARG;
        sum += covered;
    }
    *bytes = sum;
    return FSE_OK;
}

}  // extern "C"

namespace fsehip {

int check_info_ok(const fsehip_check_info* info) {
    if (!info || !fields_ok(*info)) return FSE_ERR_BAD_ARG;
    uint8_t hdr[32];
    header_bytes(*info, hdr);
    return get32(hdr + 28) == info->header_crc ? FSE_OK : FSE_ERR_BAD_ARG;
}

int check_ranges_ok(const fsehip_check_info* info, uint64_t out_cap, const fsehip_frame_range* ranges,
                    uint32_t n_ranges) {
    if (!info || (n_ranges && !ranges)) return FSE_ERR_BAD_ARG;
    std::vector<std::pair<uint64_t, uint64_t>> dst;  // non-empty destinations [lo, hi)
    dst.reserve(n_ranges);
    uint64_t dst_end = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_frame_range& g = ranges[r];
        if (g.src_off + g.len < g.src_off || g.src_off + g.len > info->n_content) return FSE_ERR_BAD_ARG;
        if (g.dst_off + g.len < g.dst_off) return FSE_ERR_BAD_ARG;
        if (g.len) dst.emplace_back(g.dst_off, g.dst_off + g.len);
        dst_end = std::max(dst_end, g.dst_off + g.len);
    }
    if (!std::is_sorted(dst.begin(), dst.end())) std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); ++i)
        if (dst[i].first < dst[i - 1].second) return FSE_ERR_BAD_ARG;
    if (dst_end > out_cap) return FSE_ERR_DST_TOO_SMALL;  // an empty range's place counts too
    return FSE_OK;
}

void check_span(CheckSpans* S, uint32_t i, const void* data, uint64_t off, uint64_t b0, uint64_t nb,
                uint64_t n_content, uint32_t check_log) {
    const uint64_t B = 1ull << check_log;
    const uint32_t alpha = (uint32_t)((reinterpret_cast<uintptr_t>(data) + off) & 15u);
    const uint64_t tail = n_content & (B - 1u);
    S->off[i] = off;
    S->b0[i] = (uint32_t)b0;
    S->nb[i] = (uint32_t)nb;
    S->k_full[i] = crc::init_share(alpha, B);
    S->k_last[i] = crc::init_share(alpha, tail ? tail : B);
}

CombinePlan check_combine_plan(uint64_t n_content, uint32_t check_log, uint32_t n_cb) {
    CombinePlan P{};
    const uint64_t B = 1ull << check_log, full = n_cb ? n_cb - 1u : 0u;  // the entries ahead of the last
    P.run = (uint32_t)((full + kCombineThreads - 1u) / kCombineThreads);
    if (!P.run) P.run = 1;
    P.x_block = crc::xpow8(B);
    P.x_last = crc::xpow8(n_cb ? n_content - full * B : 0u);
    uint32_t x = crc::xpow8(B * P.run);
    for (uint32_t d = 0; d < kCombineLevels; ++d) {
        P.level[d] = x;
        x = crc::mulmod(x, x);
    }
    return P;
}

}  // namespace fsehip
