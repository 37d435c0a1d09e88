// fse_planes_host.h -- what the plane frame's translation units share
// (fsehip.h section 2d): the host checks of fse_planes.cpp and the launchers
// of fse_planes.hip, called by fse_capi_planes.cpp.  Plain C++ with no HIP
// include (a stream travels as void*), so that fse_planes.cpp builds with g++
// alone.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/fsehip.h"

namespace fsehip {

// The range rules the element-range calls share (fsehip_planes_decompress_ranges,
// fsehip_delta_decompress_ranges) for a tensor of n_elems elements of w bytes
// and a destination of out_cap bytes: BAD_ARG, DST_TOO_SMALL or FSE_OK.
// Inline, so that each host-only translation unit builds on its own.
inline int check_elem_ranges(uint64_t n_elems, uint64_t w, uint64_t out_cap, const fsehip_planes_range* ranges,
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

// FSE_OK when `info` and `inner` are a pair fsehip_planes_read_header gives
// (each valid, inner->n_total = w * stride), BAD_ARG otherwise.
int planes_check(const fsehip_planes_info* info, const fsehip_frame_info* inner);
// The range rules of fsehip_planes_decompress_ranges for a destination of
// out_cap bytes: BAD_ARG, DST_TOO_SMALL or FSE_OK.
int planes_check_ranges(const fsehip_planes_info* info, uint64_t out_cap, const fsehip_planes_range* ranges,
                        uint32_t n_ranges);

// One launch of the pieces kernel: up to kPlanePieces element ranges, passed
// by value as a kernel argument (so the list reaches the device with the
// launch, in stream order).  Range i: plane k's `count` bytes lie at scratch +
// off[i] + k * count[i] and go to element dst[i] of the destination.
constexpr uint32_t kPlanePieces = 32;
struct PlanePieces {
    uint64_t off[kPlanePieces];
    uint64_t count[kPlanePieces];
    uint64_t dst[kPlanePieces];
    uint32_t n;
};

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t.
int launch_planes_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream);
// `result`: the frame-status word (nullptr: none); BAD_FRAME there stores nothing
int launch_planes_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                        void* stream);
int launch_planes_pieces(uint32_t w, const uint8_t* scratch, const PlanePieces& P, uint8_t* dst,
                         const int32_t* result, void* stream);
// encode: *out_len += 16 and the 16 header bytes at `out`
int launch_planes_finish(const uint8_t hdr[16], uint8_t* out, uint64_t* out_len, void* stream);
// decode, after the frame call: the 16 bytes at `in` against `hdr`; on a
// difference result[0] = BAD_FRAME, result[1] = n_status and every status
// (nullptr: none) BAD_FRAME.  zero_count (the ranges call): result[1] = 0
// either way, for the range-status launch to count into.
int launch_planes_check(const uint8_t hdr[16], const uint8_t* in, int32_t* result, int32_t* status,
                        uint64_t n_status, bool zero_count, void* stream);
// ranges: range_status[r] = the first failing status of plane_status[w * r ..
// w * r + w) (BAD_FRAME for all when result[0] says so), result[1] += ranges
// with one.
int launch_planes_range_status(uint32_t w, const int32_t* plane_status, uint32_t n_ranges, int32_t* range_status,
                               int32_t* result, void* stream);

}  // namespace fsehip
