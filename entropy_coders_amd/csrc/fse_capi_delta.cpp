// fse_capi_delta.cpp -- the delta-frame calls of the C ABI (fsehip.h section
// 2e): header and range checks in fse_delta.cpp, kernels in fse_delta.hip.
// Every call is a delta transform around one frame call of section 2b on the
// caller's scratch, as fse_capi_planes.cpp; the header finish, the header
// check and the range status are the plane frame's launchers, which take the
// 16 header bytes and w as arguments.
#include <vector>

#include "fse_capi_common.h"
#include "fse_delta_host.h"
#include "fse_planes_host.h"

using namespace fsehip::capi;

namespace {

bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

// BAD_ARG / UNSUPPORTED of a bare transform of n_elems > 0 elements
int transform_args(uint32_t w, const void* elems, const void* image, uint64_t n_elems, uintptr_t elem_align) {
    if (!width_ok(w) || (n_elems && !fsehip_delta_scratch_bytes(n_elems, w))) return FSE_ERR_UNSUPPORTED;
    if (n_elems == 0) return FSE_OK;
    if (!elems || !image || !aligned(elems, elem_align) || !aligned(image, 16)) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

// the decode calls' common checks: the info pair and the 16 header bytes
int decode_args(const fsehip_delta_info* info, const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len,
                const int32_t* d_result, uint8_t hdr[16]) {
    if (!info || !inner || !d_in || !d_result || in_len < 48u) return FSE_ERR_BAD_ARG;
    if (fsehip::delta_check(info, inner) != FSE_OK || fsehip_delta_write_header(info, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

}  // namespace

extern "C" {

int fsehip_delta_encode(uint32_t elem_bytes, const void* d_src, uint64_t n_elems, uint8_t* d_dst,
                        fsehip_stream_t stream) {
    if (const int rc = transform_args(elem_bytes, d_src, d_dst, n_elems, elem_bytes)) return rc;
    if (n_elems == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return fsehip::launch_delta_split(elem_bytes, d_src, n_elems, d_dst, stream);
}

int fsehip_delta_decode(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst,
                        fsehip_stream_t stream) {
    if (const int rc = transform_args(elem_bytes, d_dst, d_src, n_elems, 16)) return rc;
    if (n_elems == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return fsehip::launch_delta_merge(elem_bytes, d_src, n_elems, d_dst, nullptr, stream);
}

int fsehip_delta_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                          uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    if (!p || !d_out || !d_out_len || !d_result || (n_elems && (!d_src || !d_scratch))) return FSE_ERR_BAD_ARG;
    if (!width_ok(elem_bytes)) return FSE_ERR_UNSUPPORTED;
    const uint64_t image = fsehip_delta_scratch_bytes(n_elems, elem_bytes);
    if (n_elems && !image) return FSE_ERR_UNSUPPORTED;
    // the frame call's own rules, ahead of the split launch
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, image, false);
    (void)n_blocks;
    if (geom_rc != FSE_OK) return geom_rc;
    if (p->nstates > 2 || !aligned(d_src, elem_bytes) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (p->ckpt_interval && !ckpt_interval_ok(p->nstates == 1 ? 1u : 2u, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    const uint64_t bound = fsehip_delta_bound(n_elems, elem_bytes, bs);
    if (!bound) return FSE_ERR_UNSUPPORTED;
    if (scratch_cap < image || out_cap < bound) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    fsehip_delta_info info{};
    info.version = 1;
    info.elem_bytes = elem_bytes;
    info.n_elems = n_elems;
    uint8_t hdr[16];
    if (fsehip_delta_write_header(&info, hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    if (const int rc = fsehip::launch_delta_split(elem_bytes, d_src, n_elems, d_scratch, stream)) return rc;
    if (const int rc = fsehip_frame_compress(p, d_scratch, image, d_out + 16, out_cap - 16u, d_out_len, d_result, stream))
        return rc;
    return fsehip::launch_planes_finish(hdr, d_out, d_out_len, stream);
}

int fsehip_delta_decompress(const fsehip_delta_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                            const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                            void* d_out, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result,
                            fsehip_stream_t stream) {
    uint8_t hdr[16];
    if (const int rc = decode_args(info, inner, d_in, in_len, d_result, hdr)) return rc;
    const uint64_t n = info->n_elems, w = info->elem_bytes;
    if (n && (!d_out || !d_scratch)) return FSE_ERR_BAD_ARG;
    if (!aligned(d_out, 16) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (scratch_cap < inner->n_total || out_cap / w < n) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    if (const int rc = fsehip_frame_decompress(inner, chunk_blocks, d_in + 16, in_len - 16u, d_scratch, scratch_cap,
                                               d_block_status, d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_planes_check(hdr, d_in, d_result, d_block_status, inner->n_blocks, false, stream))
        return rc;
    return fsehip::launch_delta_merge(info->elem_bytes, d_scratch, n, d_out, d_result, stream);
}

// Scratch: range r's plane pieces at a 16-byte aligned offset, each from the
// restart group's first element e0 on and roundup(elem_off + n_elems - e0, 16)
// bytes apart; then the w * n_ranges statuses of the frame call.  An empty
// range decodes nothing.
int fsehip_delta_decompress_ranges(const fsehip_delta_info* info, const fsehip_frame_info* inner,
                                   uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                                   const fsehip_planes_range* ranges, uint32_t n_ranges, uint8_t* d_scratch,
                                   uint64_t scratch_cap, void* d_out, uint64_t out_cap, int32_t* d_range_status,
                                   int32_t* d_result, fsehip_stream_t stream) {
    uint8_t hdr[16];
    if (const int rc = decode_args(info, inner, d_in, in_len, d_result, hdr)) return rc;
    if (n_ranges && !ranges) return FSE_ERR_BAD_ARG;
    const uint32_t w = info->elem_bytes;
    bool any = false;
    for (uint32_t r = 0; r < n_ranges; ++r) any = any || ranges[r].n_elems;
    if ((any && !d_out) || (n_ranges && !d_scratch) || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (const int rc = fsehip::delta_check_ranges(info, out_cap, ranges, n_ranges)) return rc;
    if ((uint64_t)n_ranges * w > 0xFFFFFFFFull) return FSE_ERR_UNSUPPORTED;
    const uint64_t need = fsehip_delta_ranges_scratch_bytes(w, ranges, n_ranges);
    if ((n_ranges && !need) || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;

    std::vector<fsehip_frame_range> fr((size_t)n_ranges * w);
    std::vector<uint64_t> off(n_ranges);
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_planes_range& g = ranges[r];
        const uint64_t skip = g.elem_off & (FSEHIP_DELTA_RESTART - 1u);
        const uint64_t pitch = round_up(skip + g.n_elems, 16);
        const uint64_t from = g.n_elems ? g.elem_off - skip : g.elem_off, count = g.n_elems ? skip + g.n_elems : 0;
        off[r] = at;
        for (uint32_t k = 0; k < w; ++k)
            fr[(size_t)r * w + k] = fsehip_frame_range{k * info->stride + from, count, at + k * pitch};
        at += pitch * w;
    }
    int32_t* plane_status = reinterpret_cast<int32_t*>(d_scratch + at);
    if (const int rc = fsehip_frame_decompress_ranges(inner, chunk_blocks, d_in + 16, in_len - 16u, fr.data(),
                                                      n_ranges * w, d_scratch, at, n_ranges ? plane_status : nullptr,
                                                      d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_planes_check(hdr, d_in, d_result, nullptr, 0, true, stream)) return rc;
    if (const int rc = fsehip::launch_planes_range_status(w, plane_status, n_ranges, d_range_status, d_result, stream))
        return rc;
    for (uint32_t r0 = 0; r0 < n_ranges; r0 += fsehip::kDeltaPieces) {
        fsehip::DeltaPieces P{};
        P.n = std::min(fsehip::kDeltaPieces, n_ranges - r0);
        for (uint32_t i = 0; i < P.n; ++i) {
            const fsehip_planes_range& g = ranges[r0 + i];
            P.off[i] = off[r0 + i];
            P.skip[i] = g.n_elems ? (uint32_t)(g.elem_off & (FSEHIP_DELTA_RESTART - 1u)) : 0u;
            P.count[i] = g.n_elems ? P.skip[i] + g.n_elems : 0u;
            P.dst[i] = g.dst_elem_off;
        }
        if (const int rc = fsehip::launch_delta_pieces(w, d_scratch, P, static_cast<uint8_t*>(d_out), d_result, stream))
            return rc;
    }
    return FSE_OK;
}

}  // extern "C"
