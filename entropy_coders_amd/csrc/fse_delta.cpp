// fse_delta.cpp -- the delta frame's header, sizes and range checks, host
// side (fsehip.h section 2e).
//
// Plain C++ with no HIP include, as fse_planes.cpp: the same source builds
// into libfsehip.so and, with g++ alone, into the sanitizer fuzz of
// tests/native/delta_fuzz.cpp.  The kernels are fse_delta.hip, the device
// calls fse_capi_delta.cpp.
#include <string.h>

#include "../../include/fsehip.h"
#include "fse_delta_host.h"
#include "fse_planes_host.h"

namespace {

constexpr uint32_t kHeaderBytes = 16;
constexpr uint32_t kInnerHeaderBytes = 32;

bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }

// stride = roundup(n_elems, 16) and w * stride, false on overflow
bool image_geom(uint64_t n_elems, uint32_t w, uint64_t* stride, uint64_t* bytes) {
    if (n_elems > UINT64_MAX - 15u) return false;
    const uint64_t s = (n_elems + 15u) & ~15ull;
    if (s > UINT64_MAX / w) return false;
    *stride = s;
    *bytes = s * w;
    return true;
}

bool fields_ok(const fsehip_delta_info& f, uint64_t* stride, uint64_t* bytes) {
    return f.version == 1u && width_ok(f.elem_bytes) && f.reserved == 0u &&
           image_geom(f.n_elems, f.elem_bytes, stride, bytes);
}

}  // namespace

extern "C" {

uint64_t fsehip_delta_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes) {
    uint64_t stride, bytes;
    if (!width_ok(elem_bytes) || !image_geom(n_elems, elem_bytes, &stride, &bytes)) return 0;
    return bytes;
}

uint64_t fsehip_delta_bound(uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size) {
    uint64_t stride, bytes;
    if (!width_ok(elem_bytes) || !image_geom(n_elems, elem_bytes, &stride, &bytes)) return 0;
    const uint64_t inner = fsehip_frame_bound(bytes, block_size);
    if (inner < bytes || inner > UINT64_MAX - kHeaderBytes) return 0;  // the frame bound wrapped
    return kHeaderBytes + inner;
}

int fsehip_delta_read_header(const uint8_t* hdr, size_t len, fsehip_delta_info* out, fsehip_frame_info* inner) {
    if (!out || !inner || (!hdr && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    memset(inner, 0, sizeof(*inner));
    if (len < kHeaderBytes + kInnerHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (hdr[0] != 'F' || hdr[1] != 'S' || hdr[2] != 'E' || hdr[3] != 'D') return FSE_ERR_BAD_FRAME;
    fsehip_delta_info f;
    memset(&f, 0, sizeof(f));
    f.version = hdr[4];
    f.elem_bytes = hdr[5];
    f.reserved = (uint32_t)hdr[6] | ((uint32_t)hdr[7] << 8);
    for (int i = 7; i >= 0; --i) f.n_elems = (f.n_elems << 8) | hdr[8 + i];
    uint64_t bytes;
    if (!fields_ok(f, &f.stride, &bytes)) return FSE_ERR_BAD_FRAME;
    fsehip_frame_info in;
    if (fsehip_frame_read_header(hdr + kHeaderBytes, len - kHeaderBytes, &in) != FSE_OK) return FSE_ERR_BAD_FRAME;
    if (in.n_total != bytes) return FSE_ERR_BAD_FRAME;
    *out = f;
    *inner = in;
    return FSE_OK;
}

int fsehip_delta_write_header(const fsehip_delta_info* info, uint8_t hdr[16]) {
    uint64_t stride, bytes;
    if (!info || !hdr || !fields_ok(*info, &stride, &bytes)) return FSE_ERR_BAD_ARG;
    hdr[0] = 'F';
    hdr[1] = 'S';
    hdr[2] = 'E';
    hdr[3] = 'D';
    hdr[4] = (uint8_t)info->version;
    hdr[5] = (uint8_t)info->elem_bytes;
    hdr[6] = 0;
    hdr[7] = 0;
    for (int i = 0; i < 8; ++i) hdr[8 + i] = (uint8_t)(info->n_elems >> (8 * i));
    return FSE_OK;
}

// A range is decoded from its restart group's first element, so its plane
// pieces hold (elem_off - e0) + n_elems bytes each, every plane piece 16-byte
// aligned for the merge's loads.
uint64_t fsehip_delta_ranges_scratch_bytes(uint32_t elem_bytes, const fsehip_planes_range* ranges,
                                           uint32_t n_ranges) {
    if (!width_ok(elem_bytes) || (n_ranges && !ranges)) return 0;
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const uint64_t skip = ranges[r].elem_off & (FSEHIP_DELTA_RESTART - 1u);
        const uint64_t n = ranges[r].n_elems;
        if (n > UINT64_MAX - 15u - skip || (skip + n + 15u) / 16u > UINT64_MAX / 16u / elem_bytes) return 0;
        const uint64_t piece = ((skip + n + 15u) & ~15ull) * elem_bytes;
        if (piece > UINT64_MAX - at) return 0;
        at += piece;
    }
    if (at > UINT64_MAX - 15u - 4ull * elem_bytes * n_ranges) return 0;
    return at + (((4ull * elem_bytes * n_ranges) + 15u) & ~15ull);
}

}  // extern "C"

namespace fsehip {

int delta_check(const fsehip_delta_info* info, const fsehip_frame_info* inner) {
    uint64_t stride, bytes;
    uint8_t hb[32];
    if (!info || !inner || !fields_ok(*info, &stride, &bytes)) return FSE_ERR_BAD_ARG;
    if (fsehip_frame_write_header(inner, hb) != FSE_OK || inner->n_total != bytes) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

int delta_check_ranges(const fsehip_delta_info* info, uint64_t out_cap, const fsehip_planes_range* ranges,
                       uint32_t n_ranges) {
    if (!info || !width_ok(info->elem_bytes)) return FSE_ERR_BAD_ARG;
    return check_elem_ranges(info->n_elems, info->elem_bytes, out_cap, ranges, n_ranges);
}

}  // namespace fsehip
