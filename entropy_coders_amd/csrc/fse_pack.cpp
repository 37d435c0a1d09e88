// fse_pack.cpp -- the header, member table, sizes and planner of the pack
// frame, host side (fsehip.h section 2j): 32 header bytes, 16 bytes per
// member and one frame of section 2b over an image that holds every member's
// byte planes, plane-major from the top byte.
//
// Plain C++ with no HIP include, as fse_elem.cpp: the same source builds into
// libfsehip.so and, with g++ alone, into the sanitizer fuzz of
// tests/native/pack_fuzz.cpp.  The kernels are fse_pack.hip, the device calls
// fse_capi_pack.cpp.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/fsehip.h"
#include "fse_pack_host.h"

namespace fsehip {

namespace {

bool kind_ok(uint32_t kind) { return kind == FSEHIP_KIND_PLANES || kind == FSEHIP_KIND_DELTA; }
bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }

// stride = roundup(n_elems, 16); false when it or w * stride overflows
bool stride_of(uint64_t n_elems, uint32_t w, uint64_t* stride) {
    if (n_elems > UINT64_MAX - 15u) return false;
    *stride = (n_elems + 15u) & ~15ull;
    return *stride <= UINT64_MAX / w;
}

uint64_t get_u64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}
void put_u64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// image offsets of the eight segments' starts: seg[j] = bytes of segments 0 .. j - 1
void segment_starts(const fsehip_pack_member* members, uint64_t n, uint64_t seg[9]) {
    uint64_t by_width[9] = {};  // strides summed per width
    for (uint64_t m = 0; m < n; ++m) by_width[members[m].elem_bytes] += (members[m].n_elems + 15u) & ~15ull;
    seg[0] = 0;
    for (uint32_t j = 0; j < 8; ++j) {
        uint64_t bytes = 0;
        for (uint32_t w = j + 1; w <= 8; ++w) bytes += by_width[w];
        seg[j + 1] = seg[j] + bytes;
    }
}

uint64_t tiles_of(uint64_t n_elems) { return n_elems / FSEHIP_DELTA_RESTART + (n_elems % FSEHIP_DELTA_RESTART != 0); }

void fill_desc(const fsehip_pack_member& mb, uint64_t first_tile, PackDesc* d) {
    memset(d, 0, sizeof(*d));
    d->ptr = (uint64_t)(uintptr_t)mb.d_ptr;
    d->n_elems = mb.n_elems;
    d->first_tile = first_tile;
    d->w = mb.elem_bytes;
    d->kind = mb.kind;
}

}  // namespace

int pack_geom(const fsehip_pack_member* members, uint64_t n, uint64_t* image_bytes, uint64_t* content_bytes) {
    if (n > FSEHIP_PACK_MAX_MEMBERS || (n && !members)) return FSE_ERR_UNSUPPORTED;
    uint64_t image = 0, content = 0;
    for (uint64_t m = 0; m < n; ++m) {
        const uint32_t w = members[m].elem_bytes;
        uint64_t stride;
        if (!kind_ok(members[m].kind) || !width_ok(w) || !stride_of(members[m].n_elems, w, &stride))
            return FSE_ERR_UNSUPPORTED;
        if (stride * w > UINT64_MAX - image) return FSE_ERR_UNSUPPORTED;
        image += stride * w;
        content += members[m].n_elems * w;  // below the image's sum
    }
    if (image_bytes) *image_bytes = image;
    if (content_bytes) *content_bytes = content;
    return FSE_OK;
}

uint64_t pack_plan(const fsehip_pack_member* members, uint32_t n, PackDesc* out) {
    uint64_t at[9];
    segment_starts(members, n, at);  // at[j]: where segment j's next plane goes
    uint64_t tile = 0;
    for (uint32_t m = 0; m < n; ++m) {
        const fsehip_pack_member& mb = members[m];
        fill_desc(mb, tile, &out[m]);
        const uint64_t stride = (mb.n_elems + 15u) & ~15ull;
        for (uint32_t j = 0; j < mb.elem_bytes; ++j) {
            out[m].plane[mb.elem_bytes - 1u - j] = at[j];
            at[j] += stride;
        }
        tile += tiles_of(mb.n_elems);
    }
    return tile;
}

int pack_plan_selected(const fsehip_pack_member* members, uint32_t n, const uint32_t* sel, uint32_t n_sel,
                       std::vector<PackDesc>* descs, std::vector<fsehip_frame_range>* ranges, uint64_t* planes_bytes,
                       uint64_t* tiles) {
    if (n_sel && !sel) return FSE_ERR_BAD_ARG;
    std::vector<uint32_t> order(sel, sel + n_sel);
    std::sort(order.begin(), order.end());
    for (uint32_t s = 0; s < n_sel; ++s)
        if (order[s] >= n || (s && order[s] == order[s - 1u])) return FSE_ERR_BAD_ARG;
    // the selected members' plane offsets in the image: the whole list's plan,
    // kept only where asked for
    uint64_t at[9];
    segment_starts(members, n, at);
    std::vector<uint64_t> plane0((size_t)n_sel * 8u);
    {
        std::vector<uint32_t> slot(n, UINT32_MAX);
        for (uint32_t s = 0; s < n_sel; ++s) slot[sel[s]] = s;
        for (uint32_t m = 0; m < n; ++m) {
            const uint64_t stride = (members[m].n_elems + 15u) & ~15ull;
            for (uint32_t j = 0; j < members[m].elem_bytes; ++j) {
                if (slot[m] != UINT32_MAX) plane0[(size_t)slot[m] * 8u + members[m].elem_bytes - 1u - j] = at[j];
                at[j] += stride;
            }
        }
    }
    descs->assign(n_sel, PackDesc{});
    ranges->clear();
    uint64_t tile = 0, scratch = 0;
    for (uint32_t s = 0; s < n_sel; ++s) {
        const fsehip_pack_member& mb = members[sel[s]];
        PackDesc& d = (*descs)[s];
        fill_desc(mb, tile, &d);
        d.status0 = (uint32_t)ranges->size();
        const uint64_t stride = (mb.n_elems + 15u) & ~15ull;
        for (uint32_t k = 0; k < mb.elem_bytes; ++k) {
            d.plane[k] = scratch;
            if (stride) ranges->push_back(fsehip_frame_range{plane0[(size_t)s * 8u + k], stride, scratch});
            scratch += stride;
        }
        tile += tiles_of(mb.n_elems);
    }
    *planes_bytes = scratch;
    *tiles = tile;
    return FSE_OK;
}

}  // namespace fsehip

using namespace fsehip;

extern "C" {

uint64_t fsehip_pack_image_bytes(const fsehip_pack_member* members, uint32_t n_members) {
    uint64_t image;
    return pack_geom(members, n_members, &image, nullptr) == FSE_OK ? image : 0;
}

uint64_t fsehip_pack_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size) {
    uint64_t image;
    if (pack_geom(members, n_members, &image, nullptr) != FSE_OK) return 0;
    const uint64_t inner = fsehip_frame_bound(image, block_size), head = pack_head_bytes(n_members);
    if (inner < image || inner > UINT64_MAX - head) return 0;  // the frame bound wrapped
    return head + inner;
}

// the image | the descriptors | the head bytes
uint64_t fsehip_pack_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members) {
    uint64_t image;
    if (pack_geom(members, n_members, &image, nullptr) != FSE_OK) return 0;
    const uint64_t tail = (sizeof(PackDesc) * (uint64_t)n_members + pack_head_bytes(n_members) + 15u) & ~15ull;
    return image > UINT64_MAX - tail ? 0 : image + tail;
}

// the selected planes | their statuses | the descriptors | the head bytes
uint64_t fsehip_pack_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, const uint32_t* sel,
                                           uint32_t n_sel) {
    if (pack_geom(members, n_members, nullptr, nullptr) != FSE_OK || (n_sel && !sel)) return 0;
    uint64_t planes = 0, n_planes = 0;
    for (uint32_t s = 0; s < n_sel; ++s) {
        if (sel[s] >= n_members) return 0;
        const fsehip_pack_member& mb = members[sel[s]];
        const uint64_t bytes = ((mb.n_elems + 15u) & ~15ull) * mb.elem_bytes;
        if (bytes > UINT64_MAX - planes) return 0;
        planes += bytes;
        n_planes += mb.elem_bytes;
    }
    const uint64_t tail = ((4u * n_planes + 15u) & ~15ull) +
                          ((sizeof(PackDesc) * (uint64_t)n_sel + pack_head_bytes(n_members) + 15u) & ~15ull);
    return planes > UINT64_MAX - tail ? 0 : planes + tail;
}

uint64_t fsehip_pack_plane_offset(const fsehip_pack_member* members, uint32_t n_members, uint32_t m, uint32_t k) {
    if (pack_geom(members, n_members, nullptr, nullptr) != FSE_OK || m >= n_members || k >= members[m].elem_bytes)
        return UINT64_MAX;
    const uint32_t j = members[m].elem_bytes - 1u - k;  // the segment
    uint64_t seg[9];
    segment_starts(members, n_members, seg);
    uint64_t off = seg[j];
    for (uint32_t i = 0; i < m; ++i)
        if (members[i].elem_bytes > j) off += (members[i].n_elems + 15u) & ~15ull;
    return off;
}

int fsehip_pack_read_header(const uint8_t* buf, size_t len, fsehip_pack_info* out) {
    if (!out || (!buf && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (len < kPackHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (buf[0] != 'F' || buf[1] != 'S' || buf[2] != 'E' || buf[3] != 'M' || buf[4] != 1u) return FSE_ERR_BAD_FRAME;
    for (int i = 5; i < 8; ++i)
        if (buf[i]) return FSE_ERR_BAD_FRAME;
    for (int i = 12; i < 16; ++i)
        if (buf[i]) return FSE_ERR_BAD_FRAME;
    const uint32_t n = (uint32_t)buf[8] | (uint32_t)buf[9] << 8 | (uint32_t)buf[10] << 16 | (uint32_t)buf[11] << 24;
    if (n > FSEHIP_PACK_MAX_MEMBERS) return FSE_ERR_BAD_FRAME;
    const uint64_t image = get_u64(buf + 16), content = get_u64(buf + 24);
    if (content > image || (image & 15u)) return FSE_ERR_BAD_FRAME;  // no member list sums to these
    out->version = 1;
    out->n_members = n;
    out->image_bytes = image;
    out->content_bytes = content;
    return FSE_OK;
}

int fsehip_pack_read_members(const uint8_t* buf, size_t len, fsehip_pack_member* members, uint32_t members_cap,
                             fsehip_pack_info* out, fsehip_frame_info* inner) {
    if (!out || !inner || (!buf && len)) return FSE_ERR_BAD_ARG;
    memset(inner, 0, sizeof(*inner));
    fsehip_pack_info f;
    const int rc = fsehip_pack_read_header(buf, len, &f);
    memset(out, 0, sizeof(*out));
    if (rc != FSE_OK) return rc;
    const uint64_t head = pack_head_bytes(f.n_members);
    if (len < head || len - head < 32u) return FSE_ERR_BAD_FRAME;
    if (f.n_members > members_cap || (f.n_members && !members)) return FSE_ERR_DST_TOO_SMALL;
    for (uint32_t m = 0; m < f.n_members; ++m) {
        const uint8_t* e = buf + kPackHeaderBytes + (size_t)kPackEntryBytes * m;
        for (int i = 2; i < 8; ++i)
            if (e[i]) return FSE_ERR_BAD_FRAME;
        members[m].d_ptr = nullptr;
        members[m].kind = e[0];
        members[m].elem_bytes = e[1];
        members[m].n_elems = get_u64(e + 8);
    }
    uint64_t image, content;
    if (pack_geom(members, f.n_members, &image, &content) != FSE_OK) return FSE_ERR_BAD_FRAME;
    if (image != f.image_bytes || content != f.content_bytes) return FSE_ERR_BAD_FRAME;
    fsehip_frame_info in;
    if (fsehip_frame_read_header(buf + head, len - head, &in) != FSE_OK || in.n_total != image) return FSE_ERR_BAD_FRAME;
    *out = f;
    *inner = in;
    return FSE_OK;
}

int fsehip_pack_write_header(const fsehip_pack_member* members, uint32_t n_members, uint8_t* out) {
    uint64_t image, content;
    if (!out || pack_geom(members, n_members, &image, &content) != FSE_OK) return FSE_ERR_BAD_ARG;
    memset(out, 0, kPackHeaderBytes);
    memcpy(out, "FSEM", 4);
    out[4] = 1;
    for (int i = 0; i < 4; ++i) out[8 + i] = (uint8_t)(n_members >> (8 * i));
    put_u64(out + 16, image);
    put_u64(out + 24, content);
    for (uint32_t m = 0; m < n_members; ++m) {
        uint8_t* e = out + kPackHeaderBytes + (size_t)kPackEntryBytes * m;
        memset(e, 0, kPackEntryBytes);
        e[0] = (uint8_t)members[m].kind;
        e[1] = (uint8_t)members[m].elem_bytes;
        put_u64(e + 8, members[m].n_elems);
    }
    return FSE_OK;
}

}  // extern "C"
