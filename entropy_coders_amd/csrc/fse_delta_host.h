// fse_delta_host.h -- what the delta frame's translation units share
// (fsehip.h section 2e): the host checks of fse_delta.cpp and the launchers
// of fse_delta.hip, called by fse_capi_delta.cpp.  Plain C++ with no HIP
// include (a stream travels as void*), as fse_planes_host.h, whose header
// finish, header check and range status launchers the delta calls use as they
// are.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../include/fsehip.h"

namespace fsehip {

// FSE_OK when `info` and `inner` are a pair fsehip_delta_read_header gives
// (each valid, inner->n_total = w * stride), BAD_ARG otherwise.
int delta_check(const fsehip_delta_info* info, const fsehip_frame_info* inner);
// The range rules of fsehip_delta_decompress_ranges for a destination of
// out_cap bytes: BAD_ARG, DST_TOO_SMALL or FSE_OK.
int delta_check_ranges(const fsehip_delta_info* info, uint64_t out_cap, const fsehip_planes_range* ranges,
                       uint32_t n_ranges);

// One launch of the pieces kernel: up to kDeltaPieces element ranges, passed
// by value as a kernel argument.  Range i was decoded from its restart group's
// first element on: plane k's `count` bytes (skip + the range's elements) lie
// at scratch + off[i] + k * roundup(count[i], 16); the elements from `skip`
// on go to element dst[i] of the destination.
constexpr uint32_t kDeltaPieces = 32;
struct DeltaPieces {
    uint64_t off[kDeltaPieces];
    uint64_t count[kDeltaPieces];
    uint64_t dst[kDeltaPieces];
    uint32_t skip[kDeltaPieces];  // < FSEHIP_DELTA_RESTART
    uint32_t n;
};

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t.  w is 1, 2, 4 or 8.
int launch_delta_split(uint32_t w, const void* src, uint64_t n_elems, uint8_t* image, void* stream);
// `result`: the frame-status word (nullptr: none); BAD_FRAME there stores nothing
int launch_delta_merge(uint32_t w, const uint8_t* image, uint64_t n_elems, void* dst, const int32_t* result,
                       void* stream);
int launch_delta_pieces(uint32_t w, const uint8_t* scratch, const DeltaPieces& P, uint8_t* dst,
                        const int32_t* result, void* stream);

}  // namespace fsehip
