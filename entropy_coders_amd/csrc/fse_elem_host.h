// fse_elem_host.h -- what the element frames' translation units share: the
// plane frame (fsehip.h section 2d), the delta frame (section 2e) and the diff
// frame (section 2h) are one container, 16 header bytes and one frame of
// section 2b over a byte-plane image, told apart by an ElemKind.  The host
// checks of fse_elem.cpp and the launchers of fse_planes.hip, fse_delta.hip
// and fse_diff.hip, called by fse_capi_elem.cpp.
// Plain C++ with no HIP include (a stream travels as void*), so that
// fse_elem.cpp builds with g++ alone.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../include/fsehip.h"

namespace fsehip {

struct ElemKind {
    uint8_t magic3;   // the fourth magic byte after "FSE"
    uint32_t widths;  // bit w set: elements of w bytes are taken
    bool restart;     // elements are deltas, restarting every FSEHIP_DELTA_RESTART
};
constexpr ElemKind kPlanes{'P', 1u << 2 | 1u << 4 | 1u << 8, false};
constexpr ElemKind kDelta{'D', 1u << 1 | 1u << 2 | 1u << 4 | 1u << 8, true};
constexpr ElemKind kDiff{'B', 1u << 1 | 1u << 2 | 1u << 4 | 1u << 8, false};  // 'B': against a base

inline bool width_ok(const ElemKind& K, uint32_t w) { return w <= 8u && (K.widths >> w & 1u); }

// The exported host calls of sections 2d, 2e and 2h, by kind.
uint64_t elem_scratch_bytes(const ElemKind& K, uint64_t n_elems, uint32_t elem_bytes);
uint64_t elem_bound(const ElemKind& K, uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size);
int elem_read_header(const ElemKind& K, const uint8_t* hdr, size_t len, fsehip_planes_info* out,
                     fsehip_frame_info* inner);
int elem_write_header(const ElemKind& K, const fsehip_planes_info* info, uint8_t hdr[16]);
uint64_t elem_ranges_scratch_bytes(const ElemKind& K, uint32_t elem_bytes, const fsehip_planes_range* ranges,
                                   uint32_t n_ranges);

// FSE_OK when `info` and `inner` are a pair elem_read_header gives (each
// valid, inner->n_total = w * stride), BAD_ARG otherwise.
int elem_check(const ElemKind& K, const fsehip_planes_info* info, const fsehip_frame_info* inner);
// The range rules of the element-range calls for a tensor of n_elems elements
// of w bytes and a destination of out_cap bytes: BAD_ARG, DST_TOO_SMALL or FSE_OK.
int check_elem_ranges(uint64_t n_elems, uint64_t w, uint64_t out_cap, const fsehip_planes_range* ranges,
                      uint32_t n_ranges);
// The same for a frame's `info`, whose width must be one of the kind's.
int elem_check_ranges(const ElemKind& K, const fsehip_planes_info* info, uint64_t out_cap,
                      const fsehip_planes_range* ranges, uint32_t n_ranges);

// the delta frame's two, by the names tests/native/delta_fuzz.cpp calls
inline int delta_check(const fsehip_delta_info* info, const fsehip_frame_info* inner) {
    return elem_check(kDelta, info, inner);
}
inline int delta_check_ranges(const fsehip_delta_info* info, uint64_t out_cap, const fsehip_planes_range* ranges,
                              uint32_t n_ranges) {
    return elem_check_ranges(kDelta, info, out_cap, ranges, n_ranges);
}

// One launch of a pieces kernel: up to kPlanePieces element ranges, passed
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
// The delta frame's: range i was decoded from its restart group's first
// element on: plane k's `count` bytes (skip + the range's elements) lie at
// scratch + off[i] + k * roundup(count[i], 16); the elements from `skip` on
// go to element dst[i] of the destination.
constexpr uint32_t kDeltaPieces = 32;
struct DeltaPieces {
    uint64_t off[kDeltaPieces];
    uint64_t count[kDeltaPieces];
    uint64_t dst[kDeltaPieces];
    uint32_t skip[kDeltaPieces];  // < FSEHIP_DELTA_RESTART
    uint32_t n;
};

// The diff frame's: PlanePieces, and range i's first element in the base.
struct DiffPieces {
    uint64_t off[kPlanePieces];
    uint64_t count[kPlanePieces];
    uint64_t dst[kPlanePieces];
    uint64_t src[kPlanePieces];
    uint32_t n;
};

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t.  w is one of the kind's widths.
int launch_planes_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream);
int launch_delta_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream);
// `result`: the frame-status word (nullptr: none); BAD_FRAME there stores nothing
int launch_planes_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                        void* stream);
int launch_delta_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                       void* stream);
int launch_planes_pieces(uint32_t w, const uint8_t* scratch, const PlanePieces& P, uint8_t* dst,
                         const int32_t* result, void* stream);
int launch_delta_pieces(uint32_t w, const uint8_t* scratch, const DeltaPieces& P, uint8_t* dst,
                        const int32_t* result, void* stream);
// The diff frame's take the base tensor, n_elems elements aligned to w; the
// merge's dst may be the base itself (fse_diff.hip).  Range i of the pieces
// reads the base from element P.src[i] on.
int launch_diff_split(uint32_t w, const void* src, const void* base, uint64_t n_elems, uint8_t* image, void* stream);
int launch_diff_merge(uint32_t w, const uint8_t* image, const void* base, uint64_t n_elems, void* dst,
                      const int32_t* result, void* stream);
int launch_diff_pieces(uint32_t w, const uint8_t* scratch, const DiffPieces& P, const void* base, uint8_t* dst,
                       const int32_t* result, void* stream);
// The three below serve every kind (fse_planes.hip).
// encode: *out_len += 16 and the 16 header bytes at `out`
int launch_elem_finish(const uint8_t hdr[16], uint8_t* out, uint64_t* out_len, void* stream);
// decode, after the frame call: the 16 bytes at `in` against `hdr`; on a
// difference result[0] = BAD_FRAME, result[1] = n_status and every status
// (nullptr: none) BAD_FRAME.  zero_count (the ranges call): result[1] = 0
// either way, for the range-status launch to count into.
int launch_elem_check(const uint8_t hdr[16], const uint8_t* in, int32_t* result, int32_t* status, uint64_t n_status,
                      bool zero_count, void* stream);
// ranges: range_status[r] = the first failing status of plane_status[w * r ..
// w * r + w) (BAD_FRAME for all when result[0] says so), result[1] += ranges
// with one.
int launch_elem_range_status(uint32_t w, const int32_t* plane_status, uint32_t n_ranges, int32_t* range_status,
                             int32_t* result, void* stream);

}  // namespace fsehip
