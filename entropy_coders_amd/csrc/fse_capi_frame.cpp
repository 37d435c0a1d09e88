// fse_capi_frame.cpp -- the frame calls of the C ABI (fsehip.h section 2b):
// header in fse_frame.cpp, kernels in fse_frame.hip.  Every call holds the
// stream's workspace for all its chunks and lays the chunk scratch out as
//   META  [cb_cap x spb] u64 checkpoints | comp_len | status | record type
//   SCAN  [cb_cap] u64 record offsets | u64 running frame offset
#include <string.h>

#include "fse_capi_common.h"
#include "fse_frame_plan.h"

using namespace fsehip::capi;

namespace {

// info -> the header words (the rules of fsehip_frame_read_header: nstates,
// ckpt_interval, n_blocks = ceil(n_total / block_size), ...)
int frame_hdr(const fsehip_frame_info* info, fsehip::FrameHdr* hdr) {
    uint8_t hb[32];
    if (fsehip_frame_write_header(info, hb) != FSE_OK) return FSE_ERR_BAD_ARG;
    memcpy(hdr->w, hb, sizeof(hb));
    return FSE_OK;
}

// blocks per chunk: the caller's (0 = 4096), at most n_blocks, and few enough
// that the chunk's slots stay within 1 GiB
uint32_t frame_chunk_blocks(uint32_t chunk_blocks, uint64_t n_blocks, uint64_t slot_bytes) {
    uint64_t cb = chunk_blocks ? chunk_blocks : 4096u;
    cb = std::min(cb, std::max<uint64_t>((1ull << 30) / slot_bytes, 1u));
    return (uint32_t)std::max<uint64_t>(std::min(cb, n_blocks), 1u);
}

// One frame call: the chunk the kernels work on (F) and the parameters of the
// block coder under it (bp), on the stream's workspace.
struct FrameCall {
    fsehip::FrameChunk F{};
    fsehip_params bp;
    Lease& lease;
    fsehip_stream_t stream;
    hipStream_t hs;

    // the call-constant fields (`raw`: encode: the source; decode: the output)
    FrameCall(Lease& l, fsehip_stream_t s, const fsehip_frame_info& info, uint32_t table_log, const uint8_t* frame,
              uint64_t frame_len, const uint8_t* raw)
        : bp{info.block_size, table_log, info.ckpt_interval, info.max_table_log, info.nstates},
          lease(l), stream(s), hs(static_cast<hipStream_t>(s)) {
        F.frame = const_cast<uint8_t*>(frame);
        F.frame_len = frame_len;
        F.n_total = info.n_total;
        F.block_size = info.block_size;
        F.ckpt_interval = info.ckpt_interval;
        F.nstates = info.nstates;
        F.n_blocks = info.n_blocks;
        F.raw = const_cast<uint8_t*>(raw);
        F.slot_bytes = fsehip_slot_bytes(info.block_size, info.max_table_log);
        F.spb = fsehip_sidecar_per_block_ns(info.block_size, info.ckpt_interval, info.nstates);
    }

    // the chunk scratch for chunks of up to cb_cap blocks
    bool scratch(uint32_t cb_cap, bool slots) {
        uint8_t* meta = static_cast<uint8_t*>(lease.get(SCRATCH_FRAME_META, (12ull + 8ull * F.spb) * cb_cap));
        uint64_t* scan = static_cast<uint64_t*>(lease.get(SCRATCH_FRAME_SCAN, 8ull * cb_cap + 8u));
        F.slots = slots ? static_cast<uint8_t*>(lease.get(SCRATCH_FRAME_SLOTS, (uint64_t)cb_cap * F.slot_bytes)) : nullptr;
        if (!meta || !scan || (slots && !F.slots)) return false;
        F.sidecar = F.spb ? reinterpret_cast<uint64_t*>(meta) : nullptr;
        uint8_t* words = meta + 8ull * F.spb * cb_cap;
        F.comp_len = reinterpret_cast<uint32_t*>(words);
        F.status = reinterpret_cast<int32_t*>(words + 4ull * cb_cap);
        F.kind = reinterpret_cast<uint32_t*>(words + 8ull * cb_cap);
        F.off = scan;
        F.base = scan + cb_cap;
        return true;
    }

    // the chunk's unpacked slots decoded to `out`
    int decode_chunk(uint8_t* out, uint64_t chunk_total) {
        // non-FSE blocks have comp_len 0: their table build fails and no decode kernel touches their output
        return with_dtables_lease(&bp, F.slots, F.slot_bytes, F.comp_len, F.cb, stream, lease,
                                  [&](const uint32_t* dt, const int32_t* dti, Lease& l) {
                                      return decompress_impl(&bp, F.slots, F.slot_bytes, F.comp_len, F.sidecar, out,
                                                             chunk_total, nullptr, F.status, nullptr, 0, stream, dt,
                                                             dti, &l);
                                  });
    }

    // scan -> unpack -> decode -> merge over the blocks [first_block,
    // first_block + n_blocks) in chunks; block b lands at F.raw + b *
    // block_size and its status at status_by_block[b] (both may point below
    // their buffers: addresses, not pointer arithmetic)
    int decode_run(uint64_t first_block, uint64_t n_blocks, uint64_t blocks_per_chunk, int32_t* status_by_block,
                   int32_t* result) {
        const uint64_t bs = F.block_size, end = first_block + n_blocks;
        for (uint64_t c0 = first_block; c0 < end; c0 += blocks_per_chunk) {
            F.c0 = (uint32_t)c0;
            F.cb = (uint32_t)std::min<uint64_t>(blocks_per_chunk, end - c0);
            const uint64_t chunk_total = std::min<uint64_t>((uint64_t)F.cb * bs, F.n_total - c0 * bs);
            if (fsehip::launch_frame_scan(F, hs) != hipSuccess || fsehip::launch_frame_unpack(F, hs) != hipSuccess)
                return FSE_ERR_HIP;
            uint8_t* out = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(F.raw) + c0 * bs);
            if (const int rc = decode_chunk(out, chunk_total)) return rc;
            if (fsehip::launch_frame_merge(F, status_by_block, result, hs) != hipSuccess) return FSE_ERR_HIP;
        }
        return FSE_OK;
    }
};

}  // namespace

extern "C" {

int fsehip_frame_compress(const fsehip_frame_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_frame,
                          uint64_t frame_cap, uint64_t* d_frame_len, int32_t* d_result, fsehip_stream_t stream) {
    if (!p || !d_frame || !d_frame_len || !d_result || (n_total && !d_src)) return FSE_ERR_BAD_ARG;
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, n_total, false);
    if (geom_rc != FSE_OK) return geom_rc;
    if (p->nstates > 2 || (reinterpret_cast<uintptr_t>(d_src) & 15u)) return FSE_ERR_BAD_ARG;
    const uint32_t ns = p->nstates == 1 ? 1u : 2u;
    if (p->ckpt_interval && !ckpt_interval_ok(ns, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    if (frame_cap < fsehip_frame_bound(n_total, bs)) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const fsehip_params lp{bs, p->table_log, p->ckpt_interval, p->max_table_log, ns};
    fsehip_frame_info info{};
    info.version = 1;
    info.nstates = ns;
    info.max_table_log = kern_lmax(lmax_for(&lp));
    info.flags = p->ckpt_interval ? 1u : 0u;
    info.block_size = bs;
    info.ckpt_interval = p->ckpt_interval;
    info.n_blocks = (uint32_t)n_blocks;
    info.n_total = n_total;
    fsehip::FrameHdr hdr;
    if (frame_hdr(&info, &hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    Lease lease(stream);
    FrameCall C(lease, stream, info, p->table_log, d_frame, 0, d_src);
    const uint32_t cb_cap = frame_chunk_blocks(p->chunk_blocks, n_blocks, C.F.slot_bytes);
    if (!C.scratch(cb_cap, n_blocks != 0)) return FSE_ERR_HIP;
    fsehip::FrameChunk& F = C.F;
    if (n_blocks == 0)  // the header alone
        return rc_of(fsehip::launch_frame_plan(F, hdr, true, true, d_frame_len, d_result, C.hs));
    for (uint64_t c0 = 0; c0 < n_blocks; c0 += cb_cap) {
        F.c0 = (uint32_t)c0;
        F.cb = (uint32_t)std::min<uint64_t>(cb_cap, n_blocks - c0);
        const uint64_t chunk_total = std::min<uint64_t>((uint64_t)F.cb * bs, n_total - c0 * bs);
        // entries the encoder leaves unwritten are stored as zero
        if (F.spb && hipMemsetAsync(F.sidecar, 0, 8ull * F.spb * F.cb, C.hs) != hipSuccess) return FSE_ERR_HIP;
        const int rc = compress_blocks_impl(&C.bp, d_src + c0 * bs, chunk_total, F.slots, F.slot_bytes, F.comp_len,
                                            nullptr, F.sidecar, F.status, stream, &lease);
        if (rc != FSE_OK) return rc;
        if (fsehip::launch_frame_plan(F, hdr, c0 == 0, c0 + F.cb == n_blocks, d_frame_len, d_result, C.hs) !=
                hipSuccess ||
            fsehip::launch_frame_pack(F, C.hs) != hipSuccess)
            return FSE_ERR_HIP;
    }
    return FSE_OK;
}

int fsehip_frame_decompress(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                            uint64_t frame_len, uint8_t* d_out, uint64_t out_cap, int32_t* d_block_status,
                            int32_t* d_result, fsehip_stream_t stream) {
    if (!info || !d_frame || !d_result || (info->n_total && !d_out)) return FSE_ERR_BAD_ARG;
    if (info->block_size > kMaxBlock) return FSE_ERR_UNSUPPORTED;
    fsehip::FrameHdr hdr;
    if (frame_hdr(info, &hdr) != FSE_OK || (reinterpret_cast<uintptr_t>(d_out) & 15u)) return FSE_ERR_BAD_ARG;
    if (out_cap < info->n_total) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    Lease lease(stream);
    FrameCall C(lease, stream, *info, 0, d_frame, frame_len, d_out);
    const uint32_t cb_cap = frame_chunk_blocks(chunk_blocks, info->n_blocks, C.F.slot_bytes);
    if (!C.scratch(cb_cap, info->n_blocks != 0)) return FSE_ERR_HIP;
    if (fsehip::launch_frame_check(C.F, hdr, d_result, C.hs) != hipSuccess) return FSE_ERR_HIP;
    return C.decode_run(0, info->n_blocks, cb_cap, d_block_status, d_result);
}

// Ranges.  The planner (fse_frame.cpp) turns the ranges into listed blocks,
// direct runs and bounce chunks; its lists go to the device through pinned
// staging in one copy.  LIST scratch, uploaded part first:
//   pieces | range slots | listed blocks | bounce slots || record offsets |
//   record type | comp_len | block status | a result pair the direct runs' merge counts into
int fsehip_frame_decompress_ranges(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                                   uint64_t frame_len, const fsehip_frame_range* ranges, uint32_t n_ranges,
                                   uint8_t* d_out, uint64_t out_cap, int32_t* d_range_status, int32_t* d_result,
                                   fsehip_stream_t stream) {
    if (!info || !d_frame || !d_result || (n_ranges && !ranges)) return FSE_ERR_BAD_ARG;
    if (info->block_size > kMaxBlock) return FSE_ERR_UNSUPPORTED;
    fsehip::FrameHdr hdr;
    if (frame_hdr(info, &hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    bool any = false;
    for (uint32_t r = 0; r < n_ranges; ++r) any = any || ranges[r].len;
    if (any && !d_out) return FSE_ERR_BAD_ARG;
    const uint32_t bs = info->block_size;
    const uint32_t cb_cap = frame_chunk_blocks(chunk_blocks, info->n_blocks, fsehip_slot_bytes(bs, info->max_table_log));
    const uint64_t out_addr = reinterpret_cast<uintptr_t>(d_out);
    // validation and planning are host work: both come before any device use
    fsehip::RangePlan plan;
    int rc = fsehip::frame_plan_ranges(info, cb_cap, out_addr, out_cap, ranges, n_ranges, &plan);
    if (rc != FSE_OK) return rc;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    // the chunk scratch holds the largest chunk this call runs, not chunk_blocks
    uint64_t cb_use = std::min<uint64_t>(cb_cap, plan.bounce.size());
    for (const fsehip::RangeRun& run : plan.runs) cb_use = std::max(cb_use, std::min<uint64_t>(cb_cap, run.n_blocks));
    cb_use = std::max<uint64_t>(cb_use, 1u);
    Lease lease(stream);
    FrameCall C(lease, stream, *info, 0, d_frame, frame_len, d_out);
    if (!C.scratch((uint32_t)cb_use, !plan.blocks.empty())) return FSE_ERR_HIP;
    fsehip::FrameChunk& F = C.F;
    const hipStream_t hs = C.hs;
    if (fsehip::launch_frame_check(F, hdr, d_result, hs) != hipSuccess) return FSE_ERR_HIP;

    fsehip::FrameRanges R{};
    const uint64_t n_u = plan.blocks.size(), n_b = plan.bounce.size(), n_p = plan.bounce_piece.size();
    if (n_u > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;
    R.n_listed = (uint32_t)n_u;
    R.out = d_out;
    const uint64_t up_bytes = round_up(sizeof(fsehip::FramePiece) * n_p + 8ull * n_ranges + 4ull * n_u + 4ull * n_b, 8);
    int32_t* run_result = nullptr;
    if (n_ranges) {
        uint8_t* list = static_cast<uint8_t*>(lease.get(SCRATCH_FRAME_LIST, up_bytes + 20ull * n_u + 8u));
        PinBuf* pin = lease.pin_get(up_bytes);
        if (!list || !pin) return FSE_ERR_HIP;
        uint8_t* h = static_cast<uint8_t*>(pin->p);
        fsehip::FramePiece* hp = reinterpret_cast<fsehip::FramePiece*>(h);
        for (uint64_t k = 0; k < n_p; ++k) {
            const fsehip::RangePiece& pc = plan.pieces[plan.bounce_piece[k]];
            hp[k] = fsehip::FramePiece{pc.bounce, pc.in_off, pc.len, 0u, pc.dst_off};
        }
        uint32_t* hr = reinterpret_cast<uint32_t*>(hp + n_p);
        for (uint32_t r = 0; r < n_ranges; ++r) {
            hr[2u * r] = plan.range_slot[r];
            hr[2u * r + 1u] = plan.range_blocks[r];
        }
        uint32_t* hbk = hr + 2ull * n_ranges;
        if (n_u) memcpy(hbk, plan.blocks.data(), 4ull * n_u);
        if (n_b) memcpy(hbk + n_u, plan.bounce.data(), 4ull * n_b);
        if (hipMemcpyAsync(list, h, up_bytes, hipMemcpyHostToDevice, hs) != hipSuccess) {
            (void)hipStreamSynchronize(hs);
            return FSE_ERR_HIP;
        }
        if (!lease.pin_sent(pin)) return FSE_ERR_HIP;
        R.pieces = reinterpret_cast<const fsehip::FramePiece*>(list);
        R.range_slots = reinterpret_cast<const uint2*>(list + sizeof(fsehip::FramePiece) * n_p);
        R.blocks = reinterpret_cast<const uint32_t*>(list + sizeof(fsehip::FramePiece) * n_p + 8ull * n_ranges);
        R.bounce = R.blocks + n_u;
        R.off = reinterpret_cast<uint64_t*>(list + up_bytes);
        R.kind = reinterpret_cast<uint32_t*>(R.off + n_u);
        R.clen = R.kind + n_u;
        R.status = reinterpret_cast<int32_t*>(R.clen + n_u);
        run_result = R.status + n_u;
    }
    if (n_b) {
        R.raw_bounce = static_cast<uint8_t*>(lease.get(SCRATCH_FRAME_BOUNCE, std::min<uint64_t>(cb_cap, n_b) * bs));
        if (!R.raw_bounce) return FSE_ERR_HIP;
    }
    if (fsehip::launch_frame_seek(F, R, hs) != hipSuccess) return FSE_ERR_HIP;
    // the direct route: a run's blocks decoded in place, with F.raw and the
    // status pointer shifted so that block b lands at its place in d_out and
    // its status in the run's listed slots
    for (const fsehip::RangeRun& run : plan.runs) {
        if (fsehip::launch_frame_seed(F, R, run.slot, hs) != hipSuccess) return FSE_ERR_HIP;
        F.raw = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(d_out) + run.dst_off -
                                           (uint64_t)run.first_block * bs);
        int32_t* st = reinterpret_cast<int32_t*>(reinterpret_cast<uintptr_t>(R.status) + 4ull * run.slot -
                                                 4ull * run.first_block);
        rc = C.decode_run(run.first_block, run.n_blocks, cb_use, st, run_result);
        if (rc != FSE_OK) return rc;
    }
    // the bounce route
    F.raw = nullptr;
    F.c0 = 0;
    for (size_t c = 0; c + 1u < plan.chunk_start.size(); ++c) {
        const uint32_t j0 = plan.chunk_start[c];
        F.cb = plan.chunk_start[c + 1u] - j0;
        const uint64_t last = plan.blocks[plan.bounce[j0 + F.cb - 1u]];
        const uint64_t raw_last = std::min<uint64_t>(bs, info->n_total - last * bs);
        if (fsehip::launch_frame_gather(F, R, j0, hs) != hipSuccess) return FSE_ERR_HIP;
        rc = C.decode_chunk(R.raw_bounce, (uint64_t)(F.cb - 1u) * bs + raw_last);
        if (rc != FSE_OK) return rc;
        if (fsehip::launch_frame_gather_merge(F, R, j0, hs) != hipSuccess) return FSE_ERR_HIP;
        uint32_t max_len = 0;
        for (uint64_t p = plan.chunk_piece[c]; p < plan.chunk_piece[c + 1u]; ++p)
            max_len = std::max(max_len, plan.pieces[plan.bounce_piece[p]].len);
        for (uint64_t p = plan.chunk_piece[c]; p < plan.chunk_piece[c + 1u]; p += 1u << 30) {
            const uint32_t np = (uint32_t)std::min<uint64_t>(1u << 30, plan.chunk_piece[c + 1u] - p);
            if (fsehip::launch_frame_pieces(F, R, j0, p, np, max_len, hs) != hipSuccess) return FSE_ERR_HIP;
        }
    }
    return rc_of(fsehip::launch_frame_range_status(R, n_ranges, d_range_status, d_result, hs));
}

int fsehip_frame_decompress_range(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                                  uint64_t frame_len, uint64_t src_off, uint64_t len, uint8_t* d_out, uint64_t out_cap,
                                  int32_t* d_result, fsehip_stream_t stream) {
    const fsehip_frame_range one{src_off, len, 0};
    return fsehip_frame_decompress_ranges(info, chunk_blocks, d_frame, frame_len, &one, 1, d_out, out_cap, nullptr,
                                          d_result, stream);
}

}  // extern "C"
