// fse_pack.cpp -- the header, member table, sizes and planner of the pack
// frame and of the versioned pack, host side (fsehip.h sections 2j and 2k): 32
// header bytes, 16 bytes per member and one frame of section 2b over an image
// that holds every member's byte planes, plane-major from the top byte.  The
// two containers are flavours of one implementation: a magic, the member
// kinds it allows, and whether base pointers travel with the descriptors; the
// fsehip_pack_* and fsehip_vpack_* entry points are thin fronts of it.
//
// Plain C++ with no HIP include, as fse_elem.cpp: the same source builds into
// libfsehip.so and, with g++ alone, into the sanitizer fuzzes of
// tests/native/pack_fuzz.cpp and vpack_fuzz.cpp.  The kernels are fse_pack.hip
// and fse_vpack.hip, the device calls fse_capi_pack.cpp.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/fsehip.h"
#include "fse_pack_host.h"

namespace fsehip {

namespace {

const char* magic_of(PackFlavour f) { return f == kFlavourVpack ? "FSEV" : "FSEM"; }
bool kind_ok(PackFlavour f, uint32_t kind) {
    return kind == FSEHIP_KIND_PLANES || kind == FSEHIP_KIND_DELTA || (f == kFlavourVpack && kind == FSEHIP_KIND_DIFF);
}
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

int pack_geom(const fsehip_pack_member* members, uint64_t n, uint64_t* image_bytes, uint64_t* content_bytes,
              PackFlavour f) {
    if (n > FSEHIP_PACK_MAX_MEMBERS || (n && !members)) return FSE_ERR_UNSUPPORTED;
    uint64_t image = 0, content = 0;
    for (uint64_t m = 0; m < n; ++m) {
        const uint32_t w = members[m].elem_bytes;
        uint64_t stride;
        if (!kind_ok(f, members[m].kind) || !width_ok(w) || !stride_of(members[m].n_elems, w, &stride))
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

bool pack_needs_base(const fsehip_pack_member& mb) { return mb.kind == FSEHIP_KIND_DIFF && mb.n_elems != 0; }

bool pack_bases_ok(const fsehip_pack_member* members, const void* const* bases, const uint32_t* idx, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = idx ? idx[i] : i;
        if (!pack_needs_base(members[m])) continue;
        if (!bases || !bases[m] || ((uintptr_t)bases[m] & (members[m].elem_bytes - 1u))) return false;
    }
    return true;
}

// Sorted destination spans are checked against their neighbours; every base
// span is then looked up among them by binary search: the one destination it
// may meet is its own member's, byte for byte.
bool pack_decode_spans_ok(const fsehip_pack_member* members, const void* const* bases, const uint32_t* idx,
                          uint32_t n) {
    struct Span {
        uintptr_t lo, hi;
        uint32_t m;
        bool operator<(const Span& o) const { return lo < o.lo; }
    };
    std::vector<Span> dst;
    dst.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = idx ? idx[i] : i;
        const fsehip_pack_member& mb = members[m];
        const uintptr_t lo = reinterpret_cast<uintptr_t>(mb.d_ptr);
        if (mb.n_elems) dst.push_back(Span{lo, lo + mb.n_elems * mb.elem_bytes, m});
    }
    std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); ++i)
        if (dst[i].lo < dst[i - 1].hi) return false;
    if (!bases) return true;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = idx ? idx[i] : i;
        if (!pack_needs_base(members[m])) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(bases[m]), hi = lo + members[m].n_elems * members[m].elem_bytes;
        // the first destination that ends behind the base's start: the only
        // candidate's predecessors end at or before it, the spans being disjoint
        auto it = std::upper_bound(dst.begin(), dst.end(), lo,
                                   [](uintptr_t v, const Span& s) { return v < s.hi; });
        if (it == dst.end() || it->lo >= hi) continue;
        if (it->m != m || it->lo != lo) return false;  // its own destination has its length: no other can meet it
    }
    return true;
}

uint64_t pack_image_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members) {
    uint64_t image;
    return pack_geom(members, n_members, &image, nullptr, f) == FSE_OK ? image : 0;
}

uint64_t pack_bound(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size) {
    uint64_t image;
    if (pack_geom(members, n_members, &image, nullptr, f) != FSE_OK) return 0;
    const uint64_t inner = fsehip_frame_bound(image, block_size), head = pack_head_bytes(n_members);
    if (inner < image || inner > UINT64_MAX - head) return 0;  // the frame bound wrapped
    return head + inner;
}

// the image | the descriptors | the base pointers (the versioned pack) | the head bytes
uint64_t pack_scratch_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members) {
    uint64_t image;
    if (pack_geom(members, n_members, &image, nullptr, f) != FSE_OK) return 0;
    const uint64_t tail = (pack_desc_bytes(f) * (uint64_t)n_members + pack_head_bytes(n_members) + 15u) & ~15ull;
    return image > UINT64_MAX - tail ? 0 : image + tail;
}

// the selected planes | their statuses | the descriptors | the base pointers | the head bytes
uint64_t pack_members_scratch_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members,
                                    const uint32_t* sel, uint32_t n_sel) {
    if (pack_geom(members, n_members, nullptr, nullptr, f) != FSE_OK || (n_sel && !sel)) return 0;
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
                          ((pack_desc_bytes(f) * (uint64_t)n_sel + pack_head_bytes(n_members) + 15u) & ~15ull);
    return planes > UINT64_MAX - tail ? 0 : planes + tail;
}

uint64_t pack_plane_offset(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint32_t m,
                           uint32_t k) {
    if (pack_geom(members, n_members, nullptr, nullptr, f) != FSE_OK || m >= n_members || k >= members[m].elem_bytes)
        return UINT64_MAX;
    const uint32_t j = members[m].elem_bytes - 1u - k;  // the segment
    uint64_t seg[9];
    segment_starts(members, n_members, seg);
    uint64_t off = seg[j];
    for (uint32_t i = 0; i < m; ++i)
        if (members[i].elem_bytes > j) off += (members[i].n_elems + 15u) & ~15ull;
    return off;
}

int pack_read_header(PackFlavour f, const uint8_t* buf, size_t len, fsehip_pack_info* out) {
    if (!out || (!buf && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (len < kPackHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (memcmp(buf, magic_of(f), 4) != 0 || buf[4] != 1u) return FSE_ERR_BAD_FRAME;
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

int pack_read_members(PackFlavour f, const uint8_t* buf, size_t len, fsehip_pack_member* members,
                      uint32_t members_cap, fsehip_pack_info* out, fsehip_frame_info* inner) {
    if (!out || !inner || (!buf && len)) return FSE_ERR_BAD_ARG;
    memset(inner, 0, sizeof(*inner));
    fsehip_pack_info h;
    const int rc = pack_read_header(f, buf, len, &h);
    memset(out, 0, sizeof(*out));
    if (rc != FSE_OK) return rc;
    const uint64_t head = pack_head_bytes(h.n_members);
    if (len < head || len - head < 32u) return FSE_ERR_BAD_FRAME;
    if (h.n_members > members_cap || (h.n_members && !members)) return FSE_ERR_DST_TOO_SMALL;
    for (uint32_t m = 0; m < h.n_members; ++m) {
        const uint8_t* e = buf + kPackHeaderBytes + (size_t)kPackEntryBytes * m;
        for (int i = 2; i < 8; ++i)
            if (e[i]) return FSE_ERR_BAD_FRAME;
        members[m].d_ptr = nullptr;
        members[m].kind = e[0];
        members[m].elem_bytes = e[1];
        members[m].n_elems = get_u64(e + 8);
    }
    uint64_t image, content;
    if (pack_geom(members, h.n_members, &image, &content, f) != FSE_OK) return FSE_ERR_BAD_FRAME;
    if (image != h.image_bytes || content != h.content_bytes) return FSE_ERR_BAD_FRAME;
    fsehip_frame_info in;
    if (fsehip_frame_read_header(buf + head, len - head, &in) != FSE_OK || in.n_total != image) return FSE_ERR_BAD_FRAME;
    *out = h;
    *inner = in;
    return FSE_OK;
}

int pack_write_header(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint8_t* out) {
    uint64_t image, content;
    if (!out || pack_geom(members, n_members, &image, &content, f) != FSE_OK) return FSE_ERR_BAD_ARG;
    memset(out, 0, kPackHeaderBytes);
    memcpy(out, magic_of(f), 4);
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

}  // namespace fsehip

using namespace fsehip;

// the host calls of both containers: FRONTS(pack, kFlavourPack) are section
// 2j's, FRONTS(vpack, kFlavourVpack) section 2k's
#define FSEHIP_PACK_FRONTS(NAME, F)                                                                                 \
    uint64_t fsehip_##NAME##_image_bytes(const fsehip_pack_member* members, uint32_t n_members) {                   \
        return pack_image_bytes(F, members, n_members);                                                             \
    }                                                                                                               \
    uint64_t fsehip_##NAME##_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size) {    \
        return pack_bound(F, members, n_members, block_size);                                                       \
    }                                                                                                               \
    uint64_t fsehip_##NAME##_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members) {                 \
        return pack_scratch_bytes(F, members, n_members);                                                           \
    }                                                                                                               \
    uint64_t fsehip_##NAME##_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members,           \
                                                   const uint32_t* sel, uint32_t n_sel) {                           \
        return pack_members_scratch_bytes(F, members, n_members, sel, n_sel);                                       \
    }                                                                                                               \
    uint64_t fsehip_##NAME##_plane_offset(const fsehip_pack_member* members, uint32_t n_members, uint32_t m,        \
                                          uint32_t k) {                                                             \
        return pack_plane_offset(F, members, n_members, m, k);                                                      \
    }                                                                                                               \
    int fsehip_##NAME##_read_header(const uint8_t* buf, size_t len, fsehip_pack_info* out) {                        \
        return pack_read_header(F, buf, len, out);                                                                  \
    }                                                                                                               \
    int fsehip_##NAME##_read_members(const uint8_t* buf, size_t len, fsehip_pack_member* members,                   \
                                     uint32_t members_cap, fsehip_pack_info* out, fsehip_frame_info* inner) {       \
        return pack_read_members(F, buf, len, members, members_cap, out, inner);                                    \
    }                                                                                                               \
    int fsehip_##NAME##_write_header(const fsehip_pack_member* members, uint32_t n_members, uint8_t* out) {         \
        return pack_write_header(F, members, n_members, out);                                                       \
    }

extern "C" {

FSEHIP_PACK_FRONTS(pack, kFlavourPack)
FSEHIP_PACK_FRONTS(vpack, kFlavourVpack)

}  // extern "C"
