// fse_elem.cpp -- the header, sizes and range checks of the element frames,
// host side: the plane frame (fsehip.h section 2d), the delta frame (section
// 2e) and the diff frame (section 2h) are the same 16 header bytes over one
// frame of section 2b and differ in what an ElemKind says.
//
// Plain C++ with no HIP include, as fse_frame.cpp: the same source builds
// into libfsehip.so and, with g++ alone, into the sanitizer fuzzes of
// tests/native/planes_fuzz.cpp, delta_fuzz.cpp and diff_fuzz.cpp.  The kernels
// are fse_planes.hip, fse_delta.hip and fse_diff.hip, the device calls
// fse_capi_elem.cpp.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/fsehip.h"
#include "fse_elem_host.h"

namespace fsehip {

namespace {

constexpr uint32_t kHeaderBytes = 16;
constexpr uint32_t kInnerHeaderBytes = 32;

// stride = roundup(n_elems, 16) and w * stride, false on overflow
bool image_geom(uint64_t n_elems, uint32_t w, uint64_t* stride, uint64_t* bytes) {
    if (n_elems > UINT64_MAX - 15u) return false;
    const uint64_t s = (n_elems + 15u) & ~15ull;
    if (s > UINT64_MAX / w) return false;
    *stride = s;
    *bytes = s * w;
    return true;
}

bool fields_ok(const ElemKind& K, const fsehip_planes_info& f, uint64_t* stride, uint64_t* bytes) {
    return f.version == 1u && width_ok(K, f.elem_bytes) && f.reserved == 0u &&
           image_geom(f.n_elems, f.elem_bytes, stride, bytes);
}

}  // namespace

uint64_t elem_scratch_bytes(const ElemKind& K, uint64_t n_elems, uint32_t elem_bytes) {
    uint64_t stride, bytes;
    if (!width_ok(K, elem_bytes) || !image_geom(n_elems, elem_bytes, &stride, &bytes)) return 0;
    return bytes;
}

uint64_t elem_bound(const ElemKind& K, uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size) {
    uint64_t stride, bytes;
    if (!width_ok(K, elem_bytes) || !image_geom(n_elems, elem_bytes, &stride, &bytes)) return 0;
    const uint64_t inner = fsehip_frame_bound(bytes, block_size);
    if (inner < bytes || inner > UINT64_MAX - kHeaderBytes) return 0;  // the frame bound wrapped
    return kHeaderBytes + inner;
}

int elem_read_header(const ElemKind& K, const uint8_t* hdr, size_t len, fsehip_planes_info* out,
                     fsehip_frame_info* inner) {
    if (!out || !inner || (!hdr && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    memset(inner, 0, sizeof(*inner));
    if (len < kHeaderBytes + kInnerHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (hdr[0] != 'F' || hdr[1] != 'S' || hdr[2] != 'E' || hdr[3] != K.magic3) return FSE_ERR_BAD_FRAME;
    fsehip_planes_info f;
    memset(&f, 0, sizeof(f));
    f.version = hdr[4];
    f.elem_bytes = hdr[5];
    f.reserved = (uint32_t)hdr[6] | ((uint32_t)hdr[7] << 8);
    for (int i = 7; i >= 0; --i) f.n_elems = (f.n_elems << 8) | hdr[8 + i];
    uint64_t bytes;
    if (!fields_ok(K, f, &f.stride, &bytes)) return FSE_ERR_BAD_FRAME;
    fsehip_frame_info in;
    if (fsehip_frame_read_header(hdr + kHeaderBytes, len - kHeaderBytes, &in) != FSE_OK) return FSE_ERR_BAD_FRAME;
    if (in.n_total != bytes) return FSE_ERR_BAD_FRAME;
    *out = f;
    *inner = in;
    return FSE_OK;
}

int elem_write_header(const ElemKind& K, const fsehip_planes_info* info, uint8_t hdr[16]) {
    uint64_t stride, bytes;
    if (!info || !hdr || !fields_ok(K, *info, &stride, &bytes)) return FSE_ERR_BAD_ARG;
    hdr[0] = 'F';
    hdr[1] = 'S';
    hdr[2] = 'E';
    hdr[3] = K.magic3;
    hdr[4] = (uint8_t)info->version;
    hdr[5] = (uint8_t)info->elem_bytes;
    hdr[6] = 0;
    hdr[7] = 0;
    for (int i = 0; i < 8; ++i) hdr[8 + i] = (uint8_t)(info->n_elems >> (8 * i));
    return FSE_OK;
}

// Per range w plane pieces, 16-byte aligned for the merge's loads, then the
// w * n_ranges statuses of the frame call.  A plane range's pieces hold
// n_elems bytes each, back to back, and so do a diff range's.  A delta range is decoded from its restart
// group's first element e0, so its pieces hold (elem_off - e0) + n_elems bytes
// each, every one 16-byte aligned.
uint64_t elem_ranges_scratch_bytes(const ElemKind& K, uint32_t elem_bytes, const fsehip_planes_range* ranges,
                                   uint32_t n_ranges) {
    if (!width_ok(K, elem_bytes) || (n_ranges && !ranges)) return 0;
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const uint64_t n = ranges[r].n_elems;
        uint64_t piece;
        if (K.restart) {
            const uint64_t skip = ranges[r].elem_off & (FSEHIP_DELTA_RESTART - 1u);
            if (n > UINT64_MAX - 15u - skip || (skip + n + 15u) / 16u > UINT64_MAX / 16u / elem_bytes) return 0;
            piece = ((skip + n + 15u) & ~15ull) * elem_bytes;
        } else {
            if (n > (UINT64_MAX - 15u) / elem_bytes) return 0;
            piece = (n * elem_bytes + 15u) & ~15ull;
        }
        if (piece > UINT64_MAX - at) return 0;
        at += piece;
    }
    const uint64_t status = ((4ull * elem_bytes * n_ranges) + 15u) & ~15ull;
    if (status > UINT64_MAX - at) return 0;
    return at + status;
}

int elem_check(const ElemKind& K, const fsehip_planes_info* info, const fsehip_frame_info* inner) {
    uint64_t stride, bytes;
    uint8_t hb[32];
    if (!info || !inner || !fields_ok(K, *info, &stride, &bytes)) return FSE_ERR_BAD_ARG;
    if (fsehip_frame_write_header(inner, hb) != FSE_OK || inner->n_total != bytes) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

int check_elem_ranges(uint64_t n_elems, uint64_t w, uint64_t out_cap, const fsehip_planes_range* ranges,
                      uint32_t n_ranges) {
    if (n_ranges && !ranges) return FSE_ERR_BAD_ARG;
    std::vector<std::pair<uint64_t, uint64_t>> dst;  // non-empty destinations [lo, hi), in elements
    dst.reserve(n_ranges);
    uint64_t dst_end = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_planes_range& g = ranges[r];
        if (g.elem_off + g.n_elems < g.elem_off || g.elem_off + g.n_elems > n_elems) return FSE_ERR_BAD_ARG;
        if (g.dst_elem_off + g.n_elems < g.dst_elem_off) return FSE_ERR_BAD_ARG;
        if (g.n_elems) dst.emplace_back(g.dst_elem_off, g.dst_elem_off + g.n_elems);
        dst_end = std::max(dst_end, g.dst_elem_off + g.n_elems);
    }
    if (!std::is_sorted(dst.begin(), dst.end())) std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); ++i)
        if (dst[i].first < dst[i - 1].second) return FSE_ERR_BAD_ARG;
    if (dst_end > out_cap / w) return FSE_ERR_DST_TOO_SMALL;  // an empty range's place counts too
    return FSE_OK;
}

int elem_check_ranges(const ElemKind& K, const fsehip_planes_info* info, uint64_t out_cap,
                      const fsehip_planes_range* ranges, uint32_t n_ranges) {
    if (!info || !width_ok(K, info->elem_bytes)) return FSE_ERR_BAD_ARG;
    return check_elem_ranges(info->n_elems, info->elem_bytes, out_cap, ranges, n_ranges);
}

}  // namespace fsehip

using namespace fsehip;

extern "C" {

uint64_t fsehip_planes_scratch_bytes(uint64_t n, uint32_t w) { return elem_scratch_bytes(kPlanes, n, w); }
uint64_t fsehip_delta_scratch_bytes(uint64_t n, uint32_t w) { return elem_scratch_bytes(kDelta, n, w); }
uint64_t fsehip_planes_bound(uint64_t n, uint32_t w, uint32_t bs) { return elem_bound(kPlanes, n, w, bs); }
uint64_t fsehip_delta_bound(uint64_t n, uint32_t w, uint32_t bs) { return elem_bound(kDelta, n, w, bs); }
int fsehip_planes_read_header(const uint8_t* hdr, size_t len, fsehip_planes_info* out, fsehip_frame_info* inner) {
    return elem_read_header(kPlanes, hdr, len, out, inner);
}
int fsehip_delta_read_header(const uint8_t* hdr, size_t len, fsehip_delta_info* out, fsehip_frame_info* inner) {
    return elem_read_header(kDelta, hdr, len, out, inner);
}
int fsehip_planes_write_header(const fsehip_planes_info* info, uint8_t hdr[16]) {
    return elem_write_header(kPlanes, info, hdr);
}
int fsehip_delta_write_header(const fsehip_delta_info* info, uint8_t hdr[16]) {
    return elem_write_header(kDelta, info, hdr);
}
uint64_t fsehip_planes_ranges_scratch_bytes(uint32_t w, const fsehip_planes_range* ranges, uint32_t n_ranges) {
    return elem_ranges_scratch_bytes(kPlanes, w, ranges, n_ranges);
}
uint64_t fsehip_delta_ranges_scratch_bytes(uint32_t w, const fsehip_planes_range* ranges, uint32_t n_ranges) {
    return elem_ranges_scratch_bytes(kDelta, w, ranges, n_ranges);
}

uint64_t fsehip_diff_scratch_bytes(uint64_t n, uint32_t w) { return elem_scratch_bytes(kDiff, n, w); }
uint64_t fsehip_diff_bound(uint64_t n, uint32_t w, uint32_t bs) { return elem_bound(kDiff, n, w, bs); }
int fsehip_diff_read_header(const uint8_t* hdr, size_t len, fsehip_diff_info* out, fsehip_frame_info* inner) {
    return elem_read_header(kDiff, hdr, len, out, inner);
}
int fsehip_diff_write_header(const fsehip_diff_info* info, uint8_t hdr[16]) {
    return elem_write_header(kDiff, info, hdr);
}
uint64_t fsehip_diff_ranges_scratch_bytes(uint32_t w, const fsehip_planes_range* ranges, uint32_t n_ranges) {
    return elem_ranges_scratch_bytes(kDiff, w, ranges, n_ranges);
}

}  // extern "C"
