// fse_capi_elem.cpp -- the plane-frame, delta-frame and diff-frame calls of
// the C ABI (fsehip.h sections 2d, 2e and 2h): header and range checks in
// fse_elem.cpp, kernels in fse_planes.hip, fse_delta.hip and fse_diff.hip.
// Every call is a transform (split / merge, or their delta or diff forms)
// around one frame call of section 2b on the caller's scratch; the frames
// share every rule but what a Kind says.  Only the diff frame reads a base
// tensor: d_base is null and ignored for the other two.  The frame calls take
// the stream's workspace themselves, so nothing here holds it; what the
// kernels need beyond the scratch (header bytes, the pieces of a range list)
// travels as kernel arguments.
#include <vector>

#include "fse_capi_common.h"
#include "fse_elem_host.h"

using namespace fsehip::capi;

namespace {

struct Kind {
    const fsehip::ElemKind& host;
    bool based;  // the transforms read a base tensor (the diff frame)
    int (*split)(uint32_t, const void* src, const void* base, uint64_t, uint8_t*, void*);
    int (*merge)(uint32_t, const uint8_t*, const void* base, uint64_t, void*, const int32_t*, void*);
};
const Kind kPlanes{fsehip::kPlanes, false,
                   [](uint32_t w, const void* src, const void*, uint64_t n, uint8_t* image, void* stream) {
                       return fsehip::launch_planes_split(w, src, n, image, stream);
                   },
                   [](uint32_t w, const uint8_t* image, const void*, uint64_t n, void* dst, const int32_t* result,
                      void* stream) { return fsehip::launch_planes_merge(w, image, n, dst, result, stream); }};
const Kind kDelta{fsehip::kDelta, false,
                  [](uint32_t w, const void* src, const void*, uint64_t n, uint8_t* image, void* stream) {
                      return fsehip::launch_delta_split(w, src, n, image, stream);
                  },
                  [](uint32_t w, const uint8_t* image, const void*, uint64_t n, void* dst, const int32_t* result,
                     void* stream) { return fsehip::launch_delta_merge(w, image, n, dst, result, stream); }};
const Kind kDiff{fsehip::kDiff, true, fsehip::launch_diff_split, fsehip::launch_diff_merge};
static_assert(fsehip::kPlanePieces == fsehip::kDeltaPieces, "one loop fills either pieces struct");

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

// the base of n elements of w bytes: there and aligned to w (a kind without one: anything goes)
bool base_ok(const Kind& K, const void* d_base, uint64_t n, uint32_t w) {
    return !K.based || n == 0 || (d_base && aligned(d_base, w));
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

// a decode's destination against its base: the base itself (in place) or clear of it
bool dst_ok(const Kind& K, const void* d_out, const void* d_base, uint64_t bytes) {
    return !K.based || d_out == d_base || !overlap(d_out, bytes, d_base, bytes);
}

// BAD_ARG / UNSUPPORTED of a bare transform of n_elems > 0 elements
int transform_args(const Kind& K, uint32_t w, const void* elems, const void* d_base, const void* image,
                   uint64_t n_elems, uintptr_t elem_align) {
    if (!width_ok(K.host, w) || (n_elems && !elem_scratch_bytes(K.host, n_elems, w))) return FSE_ERR_UNSUPPORTED;
    if (n_elems == 0) return FSE_OK;
    if (!elems || !image || !aligned(elems, elem_align) || !aligned(image, 16)) return FSE_ERR_BAD_ARG;
    if (!base_ok(K, d_base, n_elems, w)) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

int split(const Kind& K, uint32_t w, const void* d_src, const void* d_base, uint64_t n_elems, uint8_t* d_dst,
          void* stream) {
    if (const int rc = transform_args(K, w, d_src, d_base, d_dst, n_elems, w)) return rc;
    if (n_elems == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return K.split(w, d_src, d_base, n_elems, d_dst, stream);
}

int merge(const Kind& K, uint32_t w, const uint8_t* d_src, const void* d_base, uint64_t n_elems, void* d_dst,
          void* stream) {
    if (const int rc = transform_args(K, w, d_dst, d_base, d_src, n_elems, 16)) return rc;
    if (n_elems == 0) return FSE_OK;
    if (!dst_ok(K, d_dst, d_base, n_elems * w)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return K.merge(w, d_src, d_base, n_elems, d_dst, nullptr, stream);
}

int compress(const Kind& K, const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, const void* d_base,
             uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
             uint64_t* d_out_len, int32_t* d_result, void* stream) {
    if (!p || !d_out || !d_out_len || !d_result || (n_elems && (!d_src || !d_scratch))) return FSE_ERR_BAD_ARG;
    if (!width_ok(K.host, elem_bytes)) return FSE_ERR_UNSUPPORTED;
    const uint64_t image = elem_scratch_bytes(K.host, n_elems, elem_bytes);
    if (n_elems && !image) return FSE_ERR_UNSUPPORTED;
    // the frame call's own rules, ahead of the split launch
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, image, false);
    (void)n_blocks;
    if (geom_rc != FSE_OK) return geom_rc;
    if (p->nstates > 2 || !aligned(d_src, elem_bytes) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (!base_ok(K, d_base, n_elems, elem_bytes)) return FSE_ERR_BAD_ARG;
    if (p->ckpt_interval && !ckpt_interval_ok(p->nstates == 1 ? 1u : 2u, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    const uint64_t bound = elem_bound(K.host, n_elems, elem_bytes, bs);
    if (!bound) return FSE_ERR_UNSUPPORTED;
    if (scratch_cap < image || out_cap < bound) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    fsehip_planes_info info{};
    info.version = 1;
    info.elem_bytes = elem_bytes;
    info.n_elems = n_elems;
    uint8_t hdr[16];
    if (elem_write_header(K.host, &info, hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    if (const int rc = K.split(elem_bytes, d_src, d_base, n_elems, d_scratch, stream)) return rc;
    if (const int rc = fsehip_frame_compress(p, d_scratch, image, d_out + 16, out_cap - 16u, d_out_len, d_result, stream))
        return rc;
    return fsehip::launch_elem_finish(hdr, d_out, d_out_len, stream);
}

// the decode calls' common checks: the info pair and the 16 header bytes
int decode_args(const Kind& K, const fsehip_planes_info* info, const fsehip_frame_info* inner, const uint8_t* d_in,
                uint64_t in_len, const int32_t* d_result, uint8_t hdr[16]) {
    if (!info || !inner || !d_in || !d_result || in_len < 48u) return FSE_ERR_BAD_ARG;
    if (elem_check(K.host, info, inner) != FSE_OK || elem_write_header(K.host, info, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    return FSE_OK;  // a block above the limit is no valid inner header: BAD_ARG above
}

int decompress(const Kind& K, const fsehip_planes_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
               const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap, void* d_out,
               const void* d_base, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result, void* stream) {
    uint8_t hdr[16];
    if (const int rc = decode_args(K, info, inner, d_in, in_len, d_result, hdr)) return rc;
    const uint64_t n = info->n_elems, w = info->elem_bytes;
    if (n && (!d_out || !d_scratch)) return FSE_ERR_BAD_ARG;
    if (!aligned(d_out, 16) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (!base_ok(K, d_base, n, (uint32_t)w) || !dst_ok(K, d_out, d_base, n * w)) return FSE_ERR_BAD_ARG;
    if (scratch_cap < inner->n_total || out_cap / w < n) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    if (const int rc = fsehip_frame_decompress(inner, chunk_blocks, d_in + 16, in_len - 16u, d_scratch, scratch_cap,
                                               d_block_status, d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_elem_check(hdr, d_in, d_result, d_block_status, inner->n_blocks, false, stream))
        return rc;
    return K.merge(info->elem_bytes, d_scratch, d_base, n, d_out, d_result, stream);
}

// Scratch: range r's w plane pieces from a 16-byte aligned offset on, `pitch`
// bytes apart; then the w * n_ranges statuses of the frame call.  A plane
// range's pieces are its n_elems bytes of each plane, back to back (so the
// frame call's direct route engages for a long range); a diff range's are the
// same, and its base elements are base[elem_off .. elem_off + n_elems), which
// no destination byte may overlap.  A delta range's run
// from the restart group's first element e0 on and lie roundup(elem_off +
// n_elems - e0, 16) bytes apart; an empty one decodes nothing.
int decompress_ranges(const Kind& K, const fsehip_planes_info* info, const fsehip_frame_info* inner,
                      uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len, const fsehip_planes_range* ranges,
                      uint32_t n_ranges, uint8_t* d_scratch, uint64_t scratch_cap, void* d_out, const void* d_base,
                      uint64_t out_cap, int32_t* d_range_status, int32_t* d_result, void* stream) {
    uint8_t hdr[16];
    if (const int rc = decode_args(K, info, inner, d_in, in_len, d_result, hdr)) return rc;
    if (n_ranges && !ranges) return FSE_ERR_BAD_ARG;
    const uint32_t w = info->elem_bytes;
    bool any = false;
    for (uint32_t r = 0; r < n_ranges; ++r) any = any || ranges[r].n_elems;
    if ((any && !d_out) || (n_ranges && !d_scratch) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (!base_ok(K, d_base, any ? info->n_elems : 0u, w)) return FSE_ERR_BAD_ARG;
    if (const int rc = elem_check_ranges(K.host, info, out_cap, ranges, n_ranges)) return rc;
    if (K.based) {  // the destinations' extent (inside out_cap, by the check above) against the whole base
        uint64_t dst_end = 0;
        for (uint32_t r = 0; r < n_ranges; ++r)
            if (ranges[r].n_elems) dst_end = std::max(dst_end, ranges[r].dst_elem_off + ranges[r].n_elems);
        if (overlap(d_out, dst_end * w, d_base, info->n_elems * w)) return FSE_ERR_BAD_ARG;
    }
    if ((uint64_t)n_ranges * w > 0xFFFFFFFFull) return FSE_ERR_UNSUPPORTED;
    const uint64_t need = elem_ranges_scratch_bytes(K.host, w, ranges, n_ranges);
    if ((n_ranges && !need) || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;

    std::vector<fsehip_frame_range> fr((size_t)n_ranges * w);
    std::vector<uint64_t> off(n_ranges);
    std::vector<uint32_t> skips(n_ranges);  // elements of the restart group ahead of a non-empty delta range
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_planes_range& g = ranges[r];
        uint64_t from = g.elem_off, count = g.n_elems, pitch = g.n_elems;
        if (K.host.restart) {
            const uint32_t skip = (uint32_t)(g.elem_off & (FSEHIP_DELTA_RESTART - 1u));
            pitch = round_up(skip + g.n_elems, 16);
            if (g.n_elems) skips[r] = skip, from -= skip, count += skip;
        }
        off[r] = at;
        for (uint32_t k = 0; k < w; ++k)
            fr[(size_t)r * w + k] = fsehip_frame_range{k * info->stride + from, count, at + k * pitch};
        at += K.host.restart ? pitch * w : round_up(g.n_elems * w, 16);
    }
    int32_t* plane_status = reinterpret_cast<int32_t*>(d_scratch + at);
    if (const int rc = fsehip_frame_decompress_ranges(inner, chunk_blocks, d_in + 16, in_len - 16u, fr.data(),
                                                      n_ranges * w, d_scratch, at, n_ranges ? plane_status : nullptr,
                                                      d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_elem_check(hdr, d_in, d_result, nullptr, 0, true, stream)) return rc;
    if (const int rc = fsehip::launch_elem_range_status(w, plane_status, n_ranges, d_range_status, d_result, stream))
        return rc;
    uint32_t r0 = 0;
    const auto fill = [&](auto& P) {  // the pieces of ranges r0 .. r0 + P.n
        P.n = std::min(fsehip::kPlanePieces, n_ranges - r0);
        for (uint32_t i = 0; i < P.n; ++i) {
            P.off[i] = off[r0 + i];
            P.count[i] = fr[(size_t)(r0 + i) * w].len;
            P.dst[i] = ranges[r0 + i].dst_elem_off;
        }
    };
    for (; r0 < n_ranges; r0 += fsehip::kPlanePieces) {
        int rc;
        if (K.host.restart) {
            fsehip::DeltaPieces P{};
            fill(P);
            for (uint32_t i = 0; i < P.n; ++i) P.skip[i] = skips[r0 + i];
            rc = fsehip::launch_delta_pieces(w, d_scratch, P, static_cast<uint8_t*>(d_out), d_result, stream);
        } else if (K.based) {
            fsehip::DiffPieces P{};
            fill(P);
            for (uint32_t i = 0; i < P.n; ++i) P.src[i] = ranges[r0 + i].elem_off;
            rc = fsehip::launch_diff_pieces(w, d_scratch, P, d_base, static_cast<uint8_t*>(d_out), d_result, stream);
        } else {
            fsehip::PlanePieces P{};
            fill(P);
            rc = fsehip::launch_planes_pieces(w, d_scratch, P, static_cast<uint8_t*>(d_out), d_result, stream);
        }
        if (rc) return rc;
    }
    return FSE_OK;
}

}  // namespace

extern "C" {

int fsehip_planes_split(uint32_t elem_bytes, const void* d_src, uint64_t n_elems, uint8_t* d_dst,
                        fsehip_stream_t stream) {
    return split(kPlanes, elem_bytes, d_src, nullptr, n_elems, d_dst, stream);
}
int fsehip_delta_encode(uint32_t elem_bytes, const void* d_src, uint64_t n_elems, uint8_t* d_dst,
                        fsehip_stream_t stream) {
    return split(kDelta, elem_bytes, d_src, nullptr, n_elems, d_dst, stream);
}
int fsehip_planes_merge(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst,
                        fsehip_stream_t stream) {
    return merge(kPlanes, elem_bytes, d_src, nullptr, n_elems, d_dst, stream);
}
int fsehip_delta_decode(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst,
                        fsehip_stream_t stream) {
    return merge(kDelta, elem_bytes, d_src, nullptr, n_elems, d_dst, stream);
}

int fsehip_planes_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                           uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    return compress(kPlanes, p, elem_bytes, d_src, nullptr, n_elems, d_scratch, scratch_cap, d_out, out_cap, d_out_len,
                    d_result, stream);
}
int fsehip_delta_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                          uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    return compress(kDelta, p, elem_bytes, d_src, nullptr, n_elems, d_scratch, scratch_cap, d_out, out_cap, d_out_len,
                    d_result, stream);
}

int fsehip_planes_decompress(const fsehip_planes_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                             const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                             void* d_out, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result,
                             fsehip_stream_t stream) {
    return decompress(kPlanes, info, inner, chunk_blocks, d_in, in_len, d_scratch, scratch_cap, d_out, nullptr, out_cap,
                      d_block_status, d_result, stream);
}
int fsehip_delta_decompress(const fsehip_delta_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                            const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                            void* d_out, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result,
                            fsehip_stream_t stream) {
    return decompress(kDelta, info, inner, chunk_blocks, d_in, in_len, d_scratch, scratch_cap, d_out, nullptr, out_cap,
                      d_block_status, d_result, stream);
}

int fsehip_planes_decompress_ranges(const fsehip_planes_info* info, const fsehip_frame_info* inner,
                                    uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                                    const fsehip_planes_range* ranges, uint32_t n_ranges, uint8_t* d_scratch,
                                    uint64_t scratch_cap, void* d_out, uint64_t out_cap, int32_t* d_range_status,
                                    int32_t* d_result, fsehip_stream_t stream) {
    return decompress_ranges(kPlanes, info, inner, chunk_blocks, d_in, in_len, ranges, n_ranges, d_scratch,
                             scratch_cap, d_out, nullptr, out_cap, d_range_status, d_result, stream);
}
int fsehip_delta_decompress_ranges(const fsehip_delta_info* info, const fsehip_frame_info* inner,
                                   uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                                   const fsehip_planes_range* ranges, uint32_t n_ranges, uint8_t* d_scratch,
                                   uint64_t scratch_cap, void* d_out, uint64_t out_cap, int32_t* d_range_status,
                                   int32_t* d_result, fsehip_stream_t stream) {
    return decompress_ranges(kDelta, info, inner, chunk_blocks, d_in, in_len, ranges, n_ranges, d_scratch, scratch_cap,
                             d_out, nullptr, out_cap, d_range_status, d_result, stream);
}

int fsehip_diff_encode(uint32_t elem_bytes, const void* d_src, const void* d_base, uint64_t n_elems, uint8_t* d_dst,
                       fsehip_stream_t stream) {
    return split(kDiff, elem_bytes, d_src, d_base, n_elems, d_dst, stream);
}
int fsehip_diff_decode(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst, const void* d_base,
                       fsehip_stream_t stream) {
    return merge(kDiff, elem_bytes, d_src, d_base, n_elems, d_dst, stream);
}
int fsehip_diff_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, const void* d_base,
                         uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                         uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    return compress(kDiff, p, elem_bytes, d_src, d_base, n_elems, d_scratch, scratch_cap, d_out, out_cap, d_out_len,
                    d_result, stream);
}
int fsehip_diff_decompress(const fsehip_diff_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                           const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                           void* d_out, const void* d_base, uint64_t out_cap, int32_t* d_block_status,
                           int32_t* d_result, fsehip_stream_t stream) {
    return decompress(kDiff, info, inner, chunk_blocks, d_in, in_len, d_scratch, scratch_cap, d_out, d_base, out_cap,
                      d_block_status, d_result, stream);
}
int fsehip_diff_decompress_ranges(const fsehip_diff_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                                  const uint8_t* d_in, uint64_t in_len, const fsehip_planes_range* ranges,
                                  uint32_t n_ranges, uint8_t* d_scratch, uint64_t scratch_cap, void* d_out,
                                  const void* d_base, uint64_t out_cap, int32_t* d_range_status, int32_t* d_result,
                                  fsehip_stream_t stream) {
    return decompress_ranges(kDiff, info, inner, chunk_blocks, d_in, in_len, ranges, n_ranges, d_scratch, scratch_cap,
                             d_out, d_base, out_cap, d_range_status, d_result, stream);
}

}  // extern "C"
