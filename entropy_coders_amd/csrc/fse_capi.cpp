// fse_capi.cpp -- C ABI (include/fsehip.h) over the gfx950 kernels: the
// batched device API (blocks, streams, tables, sidecar, pack / unpack / copy,
// histogram, generate, the device bit calls), the layout helpers and the
// diagnostics.  The frame is fse_capi_frame.cpp, the host-pointer calls
// fse_capi_host.cpp; what they share is fse_capi_common.h.
#include <memory>

#include "fse_capi_common.h"

namespace fsehip {
namespace capi {

int compress_blocks_impl(const fsehip_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_out,
                         uint64_t slot_bytes, uint32_t* d_comp_len, uint32_t* d_payload_bits, uint64_t* d_sidecar,
                         int32_t* d_status, fsehip_stream_t stream, Lease* held) {
    if (!p || !d_src || !d_out || !d_comp_len || !d_status) return FSE_ERR_BAD_ARG;
    if (n_total == 0) return FSE_ERR_EMPTY;
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, n_total, false);
    if (geom_rc != FSE_OK) return geom_rc;
    const uint32_t lmax = kern_lmax(lmax_for(p));
    if (slot_bytes & 15u) return FSE_ERR_BAD_ARG;
    const uint32_t ns = p->nstates == 1 ? 1u : 2u;
    if (p->nstates > 2) return FSE_ERR_BAD_ARG;
    if (p->ckpt_interval && !ckpt_interval_ok(ns, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    EncParams P{};
    P.nstates = ns;
    P.src = d_src;
    P.n_total = n_total;
    P.block_size = bs;
    P.n_blocks = (uint32_t)n_blocks;
    P.table_log = p->table_log;
    P.ckpt_interval = d_sidecar ? p->ckpt_interval : 0;
    P.ckpt_per_block = fsehip_sidecar_per_block_ns(bs, P.ckpt_interval, ns);
    P.out = d_out;
    P.slot_bytes = slot_bytes;
    P.comp_len = d_comp_len;
    P.payload_bits = d_payload_bits;
    P.sidecar = P.ckpt_interval ? d_sidecar : nullptr;
    P.status = d_status;
    P.lanes = (ns == 2 && env_u32("FSEHIP_ENC_LANES", 64) == 32) ? 32 : 64;
    P.debug = env_u32("FSEHIP_DEBUG", 0);
    P.xlds = env_u32("FSEHIP_ENC_XLDS", 0);  // diagnostics: occupancy probe
    P.enc_wgs = env_u32("FSEHIP_ENC_WGS", 0);  // diagnostics: workgroups per CU by whole LDS granules
    P.rank_inject = env_u32("FSEHIP_RANK_INJECT", 0);  // diagnostics: fault injection into the atomic ranks
    const size_t groups = (n_blocks * P.lanes + 63) / 64;
    P.stamps = g_stamps_enc.get(groups);
    // the L >= 13 kernels keep the spread's 2^lmax symbols in global memory:
    // in each block's slot after its header words when the slot has room,
    // else in a workspace buffer (held until the launch is enqueued)
    std::unique_ptr<Lease> lease;
    if (enc_gsym(lmax) && slot_bytes < ENC_SPREAD_OFF + (1ull << lmax)) {
        if (!held) lease = std::make_unique<Lease>(stream);
        P.spread = static_cast<uint8_t*>((held ? held : lease.get())->get(SCRATCH_SPREAD, n_blocks << lmax));
        if (!P.spread) return FSE_ERR_HIP;
    }
    hipError_t e = launch_encode(P, lmax, static_cast<hipStream_t>(stream));
    if (P.stamps) g_stamps_enc.report("encode", groups, static_cast<hipStream_t>(stream));
    return rc_of(e);
}

// Sidecar-less decode at L <= 11 (both formats): the chains defer their symbols to
// a map kernel when the stream's workspace can hold the state pairs (2 bytes
// per output byte); without it the single-kernel serial decode runs.
// FSEHIP_SERIAL_DEFER=0 (diagnostics) always takes the latter.
// The map kernel runs one 256-thread workgroup per block, so batches of
// 2^24 blocks or more (grid x threads >= 2^32) take the single-kernel decode.
void defer_symbols(Lease& lease, DecParams& P, uint32_t lmax) {
    if (lmax > 11 || P.block_size < 2u || P.n_blocks >= (1u << 24) || !env_u32("FSEHIP_SERIAL_DEFER", 1)) return;
    // the small buffer first: when it cannot be had, the multi-GiB state
    // buffer is never allocated (and never held by a decode that cannot use it)
    P.bulk = static_cast<uint32_t*>(lease.get(SCRATCH_BULK, 8ull * P.n_blocks, true));
    P.states = P.bulk ? static_cast<uint32_t*>(lease.get(SCRATCH_STATES, 2ull * P.n_blocks * P.block_size, true))
                      : nullptr;
    if (!P.states || !P.bulk) P.states = P.bulk = nullptr;
}

// Decode on prebuilt tables (dtable_blocks_kernel at stride kern_lmax):
// segment-parallel with a sidecar, else serial (container mode when n_total
// is known, the reference's own termination within out_cap otherwise).
int decompress_impl(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                    const uint64_t* d_sidecar, uint8_t* d_out, uint64_t n_total, uint64_t* d_sidecar_out,
                    int32_t* d_status, uint32_t* d_out_len, uint32_t out_cap, fsehip_stream_t stream,
                    const uint32_t* d_dt, const int32_t* d_dtinfo, Lease* lease) {
    if (!p || !d_in || !d_comp_len || !d_out || !d_status || !d_dt || !d_dtinfo) return FSE_ERR_BAD_ARG;
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, n_total, true);
    if (geom_rc != FSE_OK) return geom_rc;
    // the decoders stage / read whole 16- and 32-byte chunks of a slot and
    // store 16-byte output groups: aligned slots and buffers keep every
    // chunk inside its slot and every access aligned
    if ((slot_bytes & 31u) || (reinterpret_cast<uintptr_t>(d_in) & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 15u))
        return FSE_ERR_BAD_ARG;
    const uint32_t ns = p->nstates == 1 ? 1u : 2u;
    if (p->nstates > 2) return FSE_ERR_BAD_ARG;
    if ((d_sidecar || d_sidecar_out) && !ckpt_interval_ok(ns, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    if (ns == 1 && d_sidecar_out && kern_lmax(p->max_table_log) > 12) return FSE_ERR_UNSUPPORTED;  // decode1_serial_kernel records nothing
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    DecParams P{};
    P.nstates = ns;
    P.in = d_in;
    P.slot_bytes = slot_bytes;
    P.comp_len = d_comp_len;
    P.sidecar = d_sidecar;
    P.ckpt_interval = p->ckpt_interval;
    P.ckpt_per_block = fsehip_sidecar_per_block_ns(bs, p->ckpt_interval, ns);
    P.out = d_out;
    P.n_total = n_total;
    P.block_size = bs;
    P.n_blocks = (uint32_t)n_blocks;
    P.out_cap = out_cap;
    P.status = d_status;
    P.out_len = d_out_len;
    P.sidecar_out = d_sidecar_out;
    P.dt = d_dt;
    P.dtinfo = d_dtinfo;
    if (lease && !d_sidecar && !d_sidecar_out) defer_symbols(*lease, P, kern_lmax(p->max_table_log));
    P.stamps = g_stamps_dec.get(n_blocks);
    hipError_t e = launch_decode(P, kern_lmax(p->max_table_log), static_cast<hipStream_t>(stream));
    if (P.stamps) g_stamps_dec.report("decode", n_blocks, static_cast<hipStream_t>(stream));
    return rc_of(e);
}

// The table build; `lease` (held by the caller) supplies the header-parse
// scratch when the batch is large enough for the lane-parallel parse to pay
// (a workgroup parses 64 headers), else the table kernel parses on its own.
int build_dtables_impl(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                       uint32_t n_blocks, uint32_t* d_dtables, int32_t* d_dtinfo, fsehip_stream_t stream,
                       Lease* lease) {
    if (!p || !d_in || !d_comp_len || !d_dtables || !d_dtinfo || (slot_bytes & 255u)) return FSE_ERR_BAD_ARG;
    if (n_blocks == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    DtParams D{};
    if (lease && n_blocks >= 256u && kern_lmax(p->max_table_log) <= 12 && !env_u32("FSEHIP_DT_WAVE_PARSE", 0)) {
        uint8_t* h = static_cast<uint8_t*>(lease->get(SCRATCH_HDR, hdr_scratch_bytes(n_blocks), true));
        if (h) {
            D.hdr_norm = reinterpret_cast<uint32_t*>(h);
            D.hdr_meta = reinterpret_cast<int2*>(h + 512ull * n_blocks);
        }
    }
    D.in = d_in;
    D.slot_bytes = slot_bytes;
    D.comp_len = d_comp_len;
    D.n_blocks = n_blocks;
    D.dt = d_dtables;
    D.dtinfo = d_dtinfo;
    D.xlds = env_u32("FSEHIP_DT_XLDS", 0);  // diagnostics: occupancy probe
    D.rank_inject = env_u32("FSEHIP_RANK_INJECT", 0);  // diagnostics: fault injection into the atomic ranks
    D.stamps = g_stamps_dt.get(n_blocks);
    hipError_t e = launch_dtables(D, kern_lmax(p->max_table_log), static_cast<hipStream_t>(stream));
    if (D.stamps) g_stamps_dt.report("dtables", n_blocks, static_cast<hipStream_t>(stream));
    return rc_of(e);
}

}  // namespace capi
}  // namespace fsehip

using namespace fsehip::capi;

namespace {

// Scan of the widths into the workspace of `stream`; returns the device
// tile offsets and total (valid in stream order).
int bits_scan(Lease& lease, const uint8_t* d_nbits, const uint8_t* d_ops, uint64_t count, uint64_t** tile_off,
              uint64_t** total, fsehip_stream_t stream) {
    const uint64_t nt = fsehip::bits_tiles(count);
    uint8_t* w = static_cast<uint8_t*>(lease.get(SCRATCH_BITS, 16 + nt * 12 + 16));
    if (!w) return FSE_ERR_HIP;
    *total = reinterpret_cast<uint64_t*>(w);
    *tile_off = reinterpret_cast<uint64_t*>(w + 16);
    uint32_t* tile_sum = reinterpret_cast<uint32_t*>(w + 16 + nt * 8);
    return rc_of(fsehip::launch_bits_scan(d_nbits, d_ops, count, tile_sum, *tile_off, *total,
                                          static_cast<hipStream_t>(stream)));
}

int bits_read_dev(const uint8_t* d_in, uint64_t n_bytes, uint64_t total_bits, int stack, const uint8_t* d_nbits,
                  const uint8_t* d_ops, uint64_t count, uint32_t* d_vals, uint64_t* d_result,
                  fsehip_stream_t stream) {
    if ((count && (!d_nbits || !d_vals)) || !d_result || (!d_in && n_bytes)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    Lease lease(stream);
    uint64_t *tile_off = nullptr, *total = nullptr;
    int rc = bits_scan(lease, d_nbits, d_ops, count, &tile_off, &total, stream);
    if (rc) return rc;
    return rc_of(fsehip::launch_bits_unpack(d_in, n_bytes, total_bits, stack, d_nbits, d_ops, count, tile_off, total,
                                            d_vals, d_result, static_cast<hipStream_t>(stream)));
}

// slots -> packed stream (unpack = 0) or back
int pack_dir(const uint8_t* d_slots, uint64_t slot_bytes, const uint32_t* d_comp_len, const uint64_t* d_offsets,
             uint32_t n_blocks, uint8_t* d_stream, int unpack, fsehip_stream_t stream) {
    if (!d_slots || !d_comp_len || !d_offsets || !d_stream || (slot_bytes & 15u)) return FSE_ERR_BAD_ARG;
    if (n_blocks == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return rc_of(fsehip::launch_pack(d_slots, slot_bytes, d_comp_len, d_offsets, n_blocks, d_stream, unpack,
                                     static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

uint64_t fsehip_slot_bytes(uint32_t block_size, uint32_t max_table_log) {
    const uint64_t L = max_table_log ? max_table_log : 12;
    // header <= 512 bytes; every symbol costs <= L bits (fse.rs:170-186);
    // + both final states and the marker (lib.rs:178-181).
    const uint64_t payload = ((uint64_t)block_size * L + 2 * L + 1 + 7) / 8;
    return round_up(512 + payload + 16, 256);
}

uint32_t fsehip_sidecar_per_block(uint32_t block_size, uint32_t ckpt_interval) {
    return fsehip_sidecar_per_block_ns(block_size, ckpt_interval, 2);
}

uint32_t fsehip_sidecar_per_block_ns(uint32_t block_size, uint32_t ckpt_interval, uint32_t nstates) {
    if (ckpt_interval == 0) return 0;
    return nstates == 1 ? block_size / ckpt_interval + 2u : block_size / 2u / ckpt_interval + 2u;
}

int fsehip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

#ifdef FSEHIP_DIAG
const char* fsehip_version(void) { return "fsehip 0.2 (gfx950, diagnostics build: environment knobs live)"; }
#else
const char* fsehip_version(void) { return "fsehip 0.2 (gfx950)"; }
#endif

int fsehip_release_workspace(int device, fsehip_stream_t stream) {
    const int rc = release_workspaces(device, stream, false);
    g_stage.release();
    g_pin.release();
    return rc;
}

int fsehip_compress_blocks(const fsehip_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_out,
                           uint64_t slot_bytes, uint32_t* d_comp_len, uint32_t* d_payload_bits, uint64_t* d_sidecar,
                           int32_t* d_status, fsehip_stream_t stream) {
    return compress_blocks_impl(p, d_src, n_total, d_out, slot_bytes, d_comp_len, d_payload_bits, d_sidecar, d_status,
                                stream, nullptr);
}

uint64_t fsehip_stream_out_bytes(uint32_t src_len, uint32_t max_table_log) {
    const uint64_t L = max_table_log ? std::min<uint32_t>(max_table_log, 15u) : 12;
    // as fsehip_slot_bytes: header <= 512 bytes, <= L bits per symbol, the
    // final states and the marker; regions are 16-byte aligned, not 256
    return round_up(512 + ((uint64_t)src_len * L + 2 * L + 1 + 7) / 8, 16);
}

int fsehip_compress_streams(uint32_t nstates, uint32_t table_log, uint32_t max_table_log, const uint8_t* d_src,
                            const fsehip_stream_desc* d_desc, uint32_t n_streams, uint8_t* d_out,
                            uint32_t* d_comp_len, uint32_t* d_payload_bits, int32_t* d_status,
                            fsehip_stream_t stream) {
    if (n_streams == 0) return FSE_OK;
    if (nstates > 2 || !d_src || !d_desc || !d_out || !d_comp_len || !d_status ||
        (reinterpret_cast<uintptr_t>(d_src) & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 15u))
        return FSE_ERR_BAD_ARG;
    if (n_streams > (1u << 24) || max_table_log > 15) return FSE_ERR_UNSUPPORTED;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    if (table_log > 15) table_log = 15;  // Histogram::normalize clamps (histogram.rs:96)
    if (table_log && table_log < 5) table_log = 5;
    const fsehip_params p{0, table_log, 0, max_table_log, nstates};
    const uint32_t lmax = kern_lmax(lmax_for(&p));
    fsehip::EncParams P{};
    P.nstates = nstates == 1 ? 1u : 2u;
    P.src = d_src;
    P.n_blocks = n_streams;
    P.table_log = table_log;
    P.out = d_out;
    P.comp_len = d_comp_len;
    P.payload_bits = d_payload_bits;
    P.status = d_status;
    P.lanes = 64;
    P.enc_wgs = env_u32("FSEHIP_ENC_WGS", 0);  // diagnostics: workgroups per CU by whole LDS granules
    P.desc = d_desc;
    // L >= 13: the spread's symbols always in the workspace (a region may be
    // far smaller than 512 + 2^L bytes); the lease is held until the launch
    // is enqueued
    std::unique_ptr<Lease> lease;
    if (fsehip::enc_gsym(lmax)) {
        lease = std::make_unique<Lease>(stream);
        P.spread = static_cast<uint8_t*>(lease->get(SCRATCH_SPREAD, (uint64_t)n_streams << lmax));
        if (!P.spread) return FSE_ERR_HIP;
    }
    return rc_of(fsehip::launch_encode(P, lmax, static_cast<hipStream_t>(stream)));
}

uint64_t fsehip_dtable_bytes(uint32_t max_table_log) { return 4ull << kern_lmax(max_table_log); }

int fsehip_build_dtables(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                         uint32_t n_blocks, uint32_t* d_dtables, int32_t* d_dtinfo, fsehip_stream_t stream) {
    if (n_blocks < 256u) return build_dtables_impl(p, d_in, slot_bytes, d_comp_len, n_blocks, d_dtables, d_dtinfo, stream,
                                                   nullptr);
    Lease lease(stream);  // the header-parse scratch
    return build_dtables_impl(p, d_in, slot_bytes, d_comp_len, n_blocks, d_dtables, d_dtinfo, stream, &lease);
}

int fsehip_decompress_blocks_dt(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                                const uint32_t* d_comp_len, const uint64_t* d_sidecar, const uint32_t* d_dtables,
                                const int32_t* d_dtinfo, uint8_t* d_out, uint64_t n_total, int32_t* d_status,
                                fsehip_stream_t stream) {
    if (n_total == 0) return FSE_ERR_EMPTY;
    if (!p || !d_dtables || !d_dtinfo) return FSE_ERR_BAD_ARG;
    if (d_sidecar && p->ckpt_interval == 0) return FSE_ERR_BAD_ARG;
    if (d_sidecar)
        return decompress_impl(p, d_in, slot_bytes, d_comp_len, d_sidecar, d_out, n_total, nullptr, d_status, nullptr,
                               0, stream, d_dtables, d_dtinfo);
    Lease lease(stream);  // the deferred-symbol workspace
    return decompress_impl(p, d_in, slot_bytes, d_comp_len, nullptr, d_out, n_total, nullptr, d_status, nullptr, 0,
                           stream, d_dtables, d_dtinfo, &lease);
}

int fsehip_decompress_blocks(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                             const uint32_t* d_comp_len, const uint64_t* d_sidecar, uint8_t* d_out, uint64_t n_total,
                             int32_t* d_status, fsehip_stream_t stream) {
    if (n_total == 0) return FSE_ERR_EMPTY;
    if (!p) return FSE_ERR_BAD_ARG;
    if (d_sidecar && p->ckpt_interval == 0) return FSE_ERR_BAD_ARG;
    return with_dtables(p, d_in, slot_bytes, d_comp_len, n_total, stream,
                        [&](const uint32_t* dt, const int32_t* info, Lease& lease) {
                            return decompress_impl(p, d_in, slot_bytes, d_comp_len, d_sidecar, d_out, n_total, nullptr,
                                                   d_status, nullptr, 0, stream, dt, info, &lease);
                        });
}

int fsehip_build_sidecar(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                         const uint32_t* d_comp_len, uint8_t* d_out, uint64_t n_total, uint64_t* d_sidecar_out,
                         int32_t* d_status, fsehip_stream_t stream) {
    if (n_total == 0) return FSE_ERR_EMPTY;
    if (!p || !d_sidecar_out) return FSE_ERR_BAD_ARG;
    const uint32_t ns = p->nstates == 1 ? 1u : 2u;
    // 1-state blocks above L = 12 decode on decode1_serial_kernel, which records nothing
    if (ns == 1 && kern_lmax(p->max_table_log) > 12) return FSE_ERR_UNSUPPORTED;
    if (!ckpt_interval_ok(ns, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    return with_dtables(p, d_in, slot_bytes, d_comp_len, n_total, stream, [&](const uint32_t* dt, const int32_t* info, Lease&) {
        return decompress_impl(p, d_in, slot_bytes, d_comp_len, nullptr, d_out, n_total, d_sidecar_out, d_status,
                               nullptr, 0, stream, dt, info);
    });
}

int fsehip_decompress_streams(uint32_t nstates, uint32_t max_table_log, const uint8_t* d_in, uint64_t in_stride,
                              const uint32_t* d_comp_len, uint32_t n_streams, uint8_t* d_out, uint32_t out_stride,
                              uint32_t* d_out_len, int32_t* d_status, fsehip_stream_t stream) {
    if (n_streams == 0) return FSE_ERR_EMPTY;
    if (nstates > 2 || !d_in || !d_comp_len || !d_out || !d_out_len || !d_status || out_stride == 0 ||
        (in_stride & 255u) || (reinterpret_cast<uintptr_t>(d_in) & 15u) || (out_stride & 15u) ||
        (reinterpret_cast<uintptr_t>(d_out) & 15u))  // 16-byte input chunks and output groups
        return FSE_ERR_BAD_ARG;
    if (max_table_log > 15) return FSE_ERR_UNSUPPORTED;
    const fsehip_params p{out_stride, 0, 0, max_table_log ? max_table_log : 11u, nstates ? nstates : 2u};
    return with_dtables_n(&p, d_in, in_stride, d_comp_len, n_streams, stream,
                          [&](const uint32_t* dt, const int32_t* info, Lease& lease) {
                              fsehip::DecParams P = ref_mode_params(p.nstates, d_in, in_stride, d_comp_len, d_out,
                                                                    out_stride, out_stride, n_streams, d_status,
                                                                    d_out_len, dt, info);
                              defer_symbols(lease, P, kern_lmax(p.max_table_log));
                              return rc_of(fsehip::launch_decode(P, kern_lmax(p.max_table_log),
                                                                 static_cast<hipStream_t>(stream)));
                          });
}

int fsehip_histogram_blocks(const uint8_t* d_src, uint64_t n_total, uint32_t block_size, uint32_t* d_counts,
                            uint32_t* d_table_len, fsehip_stream_t stream) {
    if (!d_src || !d_counts) return FSE_ERR_BAD_ARG;
    // no block limit here (a histogram counts no bits), so not block_geom()
    const uint32_t bs = block_size ? block_size : kDefaultBlock;
    const uint64_t n_blocks = n_total ? (n_total + bs - 1) / bs : 1;
    if (n_blocks > 1 && (bs & 15u)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return rc_of(fsehip::launch_histogram(d_src, n_total, bs, (uint32_t)n_blocks, d_counts, d_table_len,
                                          static_cast<hipStream_t>(stream)));
}

int fsehip_pack_blocks(const uint8_t* d_slots, uint64_t slot_bytes, const uint32_t* d_comp_len,
                       const uint64_t* d_offsets, uint32_t n_blocks, uint8_t* d_stream, fsehip_stream_t stream) {
    return pack_dir(d_slots, slot_bytes, d_comp_len, d_offsets, n_blocks, d_stream, 0, stream);
}

int fsehip_unpack_blocks(const uint8_t* d_stream, const uint64_t* d_offsets, const uint32_t* d_comp_len,
                         uint32_t n_blocks, uint8_t* d_slots, uint64_t slot_bytes, fsehip_stream_t stream) {
    return pack_dir(d_slots, slot_bytes, d_comp_len, d_offsets, n_blocks, const_cast<uint8_t*>(d_stream), 1, stream);
}

int fsehip_copy_blocks(const uint8_t* d_src, const uint64_t* d_src_offsets, const uint32_t* d_lens, uint32_t n_blocks,
                       uint8_t* d_dst, const uint64_t* d_dst_offsets, fsehip_stream_t stream) {
    if (n_blocks == 0) return FSE_OK;
    if (!d_src || !d_src_offsets || !d_lens || !d_dst || !d_dst_offsets) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return rc_of(fsehip::launch_copy(d_src, d_src_offsets, d_lens, n_blocks, d_dst, d_dst_offsets,
                                     static_cast<hipStream_t>(stream)));
}

int fsehip_generate(int kind, double prob, uint64_t seed, uint32_t block_size, uint8_t* d_out, uint64_t n_total,
                    fsehip_stream_t stream) {
    if (!d_out || kind < 0 || kind > 2) return FSE_ERR_BAD_ARG;
    if (n_total == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    fsehip::GenParams G{};
    G.out = d_out;
    G.n_total = n_total;
    G.block_size = block_size ? block_size : kDefaultBlock;
    G.seed = seed;
    G.kind = kind;
    if (kind == 0) {
        // LUT of benches/fse_benchmark.rs:5-20 as symbol start indices
        if (prob < 0.005) prob = 0.005;
        if (prob > 0.995) prob = 0.995;
        size_t remaining = 4096, idx = 0;
        uint32_t s = 0;
        while (remaining > 0) {
            size_t cnt = (size_t)((double)remaining * prob);
            if (cnt < 1) cnt = 1;
            if (s >= 1024) return FSE_ERR_BAD_ARG;
            G.bound[s++] = (uint16_t)idx;
            idx += cnt;
            remaining -= cnt;
        }
        G.nsym = s;
    }
    return rc_of(fsehip::launch_generate(G, static_cast<hipStream_t>(stream)));
}

// ------------------------------------------------------------- bitstream

int fsehip_bitstack_write(const uint32_t* d_vals, const uint8_t* d_nbits, uint64_t count, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_total_bits, fsehip_stream_t stream) {
    if ((count && (!d_vals || !d_nbits)) || !d_out || !d_total_bits || (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    Lease lease(stream);
    uint64_t *tile_off = nullptr, *total = nullptr;
    int rc = bits_scan(lease, d_nbits, nullptr, count, &tile_off, &total, stream);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fsehip::launch_bits_pack(d_vals, d_nbits, count, tile_off, total, reinterpret_cast<uint32_t*>(d_out),
                                 out_cap / 4u, s) != hipSuccess)
        return FSE_ERR_HIP;
    return rc_of(hipMemcpyAsync(d_total_bits, total, 8, hipMemcpyDeviceToDevice, s));
}

int fsehip_bitstack_read(const uint8_t* d_in, uint64_t n_bytes, const uint8_t* d_nbits, uint64_t count,
                         uint32_t* d_vals, uint64_t* d_result, fsehip_stream_t stream) {
    return bits_read_dev(d_in, n_bytes, 0, 1, d_nbits, nullptr, count, d_vals, d_result, stream);
}

int fsehip_bitstream_read_ops(const uint8_t* d_in, uint64_t n_bytes, uint64_t total_bits, const uint8_t* d_nbits,
                              const uint8_t* d_ops, uint64_t count, uint32_t* d_vals, uint64_t* d_result,
                              fsehip_stream_t stream) {
    if (n_bytes == 0 || (total_bits + 7u) / 8u != n_bytes) return FSE_ERR_BAD_ARG;  // stream_reader.rs:17-21 asserts
    return bits_read_dev(d_in, n_bytes, total_bits, 0, d_nbits, d_ops, count, d_vals, d_result, stream);
}

int fsehip_bitstream_read(const uint8_t* d_in, uint64_t n_bytes, uint64_t total_bits, const uint8_t* d_nbits,
                          uint64_t count, uint32_t* d_vals, uint64_t* d_result, fsehip_stream_t stream) {
    return fsehip_bitstream_read_ops(d_in, n_bytes, total_bits, d_nbits, nullptr, count, d_vals, d_result, stream);
}

// ----------------------------------------------------------- diagnostics

// Diagnostics only (not part of include/fsehip.h): resident workgroups per CU.
int fsehipx_occupancy(char* buf, int cap) {
    if (!buf || cap <= 0 || !device_ok()) return 0;
    const int n = fsehip::occupancy_report(buf, cap);
    return n < cap ? n + fsehip::occupancy_report_dec(buf + n, cap - n) : n;
}

// Diagnostics only: the lane-order check behind the table builds' atomic
// ranks, run now (fse_kernels.h rank_order_check); FSE_OK with the counts.
int fsehipx_rank_order_check(uint32_t* violations, uint64_t* atomics) {
    if (!violations || !atomics) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return rc_of(fsehip::rank_order_check(violations, atomics));
}

int fsehip_rank_fallbacks(int device, uint32_t counts[3], int reset) {
    if (!counts) return FSE_ERR_BAD_ARG;
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return FSE_ERR_NO_DEVICE;
    const bool r = reset != 0;
    uint32_t shared = 0;  // the shared-table images count with the table calls
    const bool ok = fsehip::rank_fallbacks_enc(&counts[0], r) == hipSuccess &&
                    fsehip::rank_fallbacks_dec(&counts[1], r) == hipSuccess &&
                    fsehip::rank_fallbacks_tab(&counts[2], r) == hipSuccess &&
                    fsehip::rank_fallbacks_shared(&shared, r) == hipSuccess;
    counts[2] += shared;
    (void)hipSetDevice(prev);
    return ok ? FSE_OK : FSE_ERR_HIP;
}

// Diagnostics only: force the table builds' rank method (tests of the
// fallback): -1 / 0 = atomic ranks checked per table (the default), 1 =
// peer-mask ranks.  Returns the previous mode.
int fsehipx_rank_mode(int mode) { return fsehip::rank_mode(mode < 0 ? -1 : mode > 0 ? 1 : 0); }

}  // extern "C"
