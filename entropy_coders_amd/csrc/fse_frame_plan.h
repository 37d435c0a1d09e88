// fse_frame_plan.h -- the host planner of fsehip_frame_decompress_ranges
// (fsehip.h section 2b; defined in fse_frame.cpp).  Plain C++ with no HIP
// include: fse_capi_frame.cpp uses it, and tests/native/frame_ranges_fuzz.cpp
// builds it with g++ alone.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/fsehip.h"

namespace fsehip {

// A direct run (below) is taken from this many whole blocks on: a run costs
// a scan / unpack / table / decode / merge sequence of its own, while the
// bounce route batches the blocks of all ranges into shared chunks, so short
// runs are cheaper bounced.  Reasoned, not tuned.
constexpr uint32_t kDirectMinBlocks = 4;

// The part of one range that lies in one block and goes the bounce route.
struct RangePiece {
    uint32_t range;    // index into the caller's ranges
    uint32_t slot;     // index into RangePlan::blocks
    uint32_t in_off;   // first byte within the block
    uint32_t len;      // > 0, in_off + len <= the block's raw length
    uint64_t dst_off;  // from d_out
    uint32_t bounce;   // index into RangePlan::bounce
};
// Whole blocks [first_block, first_block + n_blocks) of one range, decoded in
// place: block first_block lands at d_out + dst_off, 16-byte aligned.  At
// most one per range.
struct RangeRun {
    uint32_t range, first_block, n_blocks;
    uint32_t slot;  // of first_block; the run's slots are consecutive
    uint64_t dst_off;
};
// Every byte of every range is served by exactly one piece or by its range's run.
struct RangePlan {
    std::vector<uint32_t> blocks;        // every covered block once, ascending
    std::vector<uint32_t> range_slot;    // per range: the slot of its first block (0 for an empty range) ...
    std::vector<uint32_t> range_blocks;  // ... and how many blocks (consecutive slots) it touches
    std::vector<RangeRun> runs;          // the direct route
    std::vector<RangePiece> pieces;      // the bounce route: range by range, each in block order
    std::vector<uint64_t> piece_start;   // n_ranges + 1: range r owns pieces [piece_start[r], piece_start[r + 1])
    std::vector<uint32_t> bounce;        // slots with a piece, ascending
    std::vector<uint64_t> bounce_piece;  // indices of the pieces, ordered by (bounce index, range)
    // Bounce chunk c is bounce[chunk_start[c] .. chunk_start[c + 1]) with the
    // pieces bounce_piece[chunk_piece[c] .. chunk_piece[c + 1]); at most
    // cb_cap blocks each, so the frame's short last block, being the highest,
    // is the last block of its chunk.
    std::vector<uint32_t> chunk_start;
    std::vector<uint64_t> chunk_piece;
};

// Validate `ranges` against the frame `info` and the destination of out_cap
// bytes at address out_addr (only its low four bits matter), and build the
// work list for chunks of cb_cap >= 1 blocks.  FSE_OK, or as
// fsehip_frame_decompress_ranges: BAD_ARG (null pointer, an info
// fsehip_frame_read_header would reject, src_off + len overflowing or past
// n_total, dst_off + len overflowing, two non-empty destinations
// overlapping), DST_TOO_SMALL (dst_off + len > out_cap).  `plan` may be
// nullptr to validate only.
int frame_plan_ranges(const fsehip_frame_info* info, uint32_t cb_cap, uint64_t out_addr, uint64_t out_cap,
                      const fsehip_frame_range* ranges, uint32_t n_ranges, RangePlan* plan);

}  // namespace fsehip
