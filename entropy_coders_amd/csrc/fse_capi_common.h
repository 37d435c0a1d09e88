// fse_capi_common.h -- what the C ABI's translation units share (fse_capi.cpp:
// the batched device API; fse_capi_frame.cpp: the frame; fse_capi_host.cpp:
// the host-pointer calls).  Internal (hidden) to libfsehip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/fsehip.h"
#include "fse_kernels.h"
#include "fse_workspace.h"

namespace fsehip {
namespace capi __attribute__((visibility("hidden"))) {

constexpr uint32_t kDefaultBlock = 65536;
// Largest block: the kernels count a block's bits in u32 (payload bits,
// sidecar bit positions, suffix sums), and block_size * 15 + header must stay
// below 2^32 bits.
constexpr uint32_t kMaxBlock = 1u << 28;

// Tuning / ablation / diagnostics knobs (FSEHIP_ENC_LANES, FSEHIP_DEBUG,
// FSEHIP_STAMPS, FSEHIP_SERIAL_*, FSEHIP_*_XLDS, FSEHIP_ENC_WGS; see fse_kernels.h) exist
// only in the diagnostics build libfsehip_diag.so (make diag, -DFSEHIP_DIAG):
// several of them change the output on purpose (ablations).  The product
// libfsehip.so reads no environment variable -- every call's result depends
// on its arguments alone, as the crate's pure functions do.  (Inline, so that
// the product holds no knob's name either.)
#ifdef FSEHIP_DIAG
inline uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = getenv(name);
    return v && *v ? (uint32_t)strtoul(v, nullptr, 0) : dflt;
}
#else
inline uint32_t env_u32(const char*, uint32_t dflt) { return dflt; }
#endif

// FSEHIP_STAMPS=1: per-workgroup phase stamps, averaged and printed to
// stderr after the (synchronised) launch.  Diagnostics only.
struct Stamps {
    uint64_t* d = nullptr;
    size_t n = 0;
    uint64_t* get(size_t groups);
    void report(const char* what, size_t groups, hipStream_t s);
};
extern Stamps g_stamps_enc, g_stamps_dec, g_stamps_dt;

inline int rc_of(hipError_t e) { return e == hipSuccess ? FSE_OK : FSE_ERR_HIP; }

inline uint32_t lmax_for(const fsehip_params* p) {
    if (p->max_table_log) return p->max_table_log;
    if (p->table_log == 0) return 11;  // optimal_log2 never exceeds 11 (histogram.rs:273-276)
    return p->table_log < 11 ? 11 : p->table_log;
}

// Kernel table bound for a max_table_log: tables are instantiated at 11
// (L <= 11), 12, 13, 14 and 15 (normalize clamps requests to 15,
// histogram.rs:96); 0 = 12.  Decode tables use this stride.
inline uint32_t kern_lmax(uint32_t max_table_log) {
    if (max_table_log == 0) return 12;
    return max_table_log <= 11 ? 11 : max_table_log >= 15 ? 15 : max_table_log;
}

// A call's block size (0 = the default) and block count; an empty input is
// one block for the decoders (reference mode) and none for the frame.
// UNSUPPORTED above kMaxBlock, then BAD_ARG for more than one block of a size
// that is no multiple of 16 or for more than 2^32 - 1 blocks.
struct BlockGeom {
    uint32_t bs;
    uint64_t n_blocks;
    int rc;
};
inline BlockGeom block_geom(uint32_t block_size, uint64_t n_total, bool empty_is_one_block) {
    const uint32_t bs = block_size ? block_size : kDefaultBlock;
    if (bs > kMaxBlock) return {bs, 0, FSE_ERR_UNSUPPORTED};
    const uint64_t nb = n_total || !empty_is_one_block ? (n_total + bs - 1) / bs : 1;
    return {bs, nb, (nb > 1 && (bs & 15u)) || nb > 0xFFFFFFFFull ? FSE_ERR_BAD_ARG : FSE_OK};
}

// a checkpoint interval the kernels take: a power of two, at least 8 (1-state: 16)
inline bool ckpt_interval_ok(uint32_t ns, uint32_t interval) {
    return interval >= (ns == 1 ? 16u : 8u) && !(interval & (interval - 1));
}

// Reference mode (n_total = 0): each of the n streams, `stride` apart, ends
// where the crate's decoder stops, within out_cap bytes of its out_stride.
inline DecParams ref_mode_params(uint32_t nstates, const uint8_t* in, uint64_t stride, const uint32_t* comp_len,
                                 uint8_t* out, uint32_t out_stride, uint32_t out_cap, uint32_t n, int32_t* status,
                                 uint32_t* out_len, const uint32_t* dt, const int32_t* info) {
    DecParams P{};
    P.nstates = nstates;
    P.in = in;
    P.slot_bytes = stride;
    P.comp_len = comp_len;
    P.out = out;
    P.block_size = out_stride;
    P.n_blocks = n;
    P.out_cap = out_cap;
    P.status = status;
    P.out_len = out_len;
    P.dt = dt;
    P.dtinfo = info;
    return P;
}

// `held`: the caller's lease on the stream's workspace (the frame calls), or
// nullptr: the call takes its own when it needs the spread scratch.
int compress_blocks_impl(const fsehip_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_out,
                         uint64_t slot_bytes, uint32_t* d_comp_len, uint32_t* d_payload_bits, uint64_t* d_sidecar,
                         int32_t* d_status, fsehip_stream_t stream, Lease* held);
void defer_symbols(Lease& lease, DecParams& P, uint32_t lmax);
int decompress_impl(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                    const uint64_t* d_sidecar, uint8_t* d_out, uint64_t n_total, uint64_t* d_sidecar_out,
                    int32_t* d_status, uint32_t* d_out_len, uint32_t out_cap, fsehip_stream_t stream,
                    const uint32_t* d_dt, const int32_t* d_dtinfo, Lease* lease = nullptr);
int build_dtables_impl(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                       uint32_t n_blocks, uint32_t* d_dtables, int32_t* d_dtinfo, fsehip_stream_t stream, Lease* lease);

// Decode tables for all blocks at high occupancy into the stream's
// workspace, then `run(dt, info, lease)` enqueues the decode on them; both under
// the workspace lock.
// (with_dtables_lease: on a lease the caller already holds -- the frame calls)
template <class Run>
int with_dtables_lease(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                       uint64_t n_blocks, fsehip_stream_t stream, Lease& lease, Run run) {
    uint32_t* dt = static_cast<uint32_t*>(lease.get(SCRATCH_DT, fsehip_dtable_bytes(p->max_table_log) * n_blocks));
    int32_t* info = static_cast<int32_t*>(lease.get(SCRATCH_DTINFO, 4ull * n_blocks));
    if (!dt || !info) return FSE_ERR_HIP;
    int rc = build_dtables_impl(p, d_in, slot_bytes, d_comp_len, (uint32_t)n_blocks, dt, info, stream, &lease);
    return rc != FSE_OK ? rc : run(dt, info, lease);
}
template <class Run>
int with_dtables_n(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                   uint64_t n_blocks, fsehip_stream_t stream, Run run) {
    if (n_blocks > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    Lease lease(stream);
    return with_dtables_lease(p, d_in, slot_bytes, d_comp_len, n_blocks, stream, lease, run);
}
// by raw length.  The block size's multiple-of-16 rule is decompress_impl's,
// after the tables: block_geom() would move it ahead of them.
template <class Run>
int with_dtables(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes, const uint32_t* d_comp_len,
                 uint64_t n_total, fsehip_stream_t stream, Run run) {
    const uint32_t bs = p->block_size ? p->block_size : kDefaultBlock;
    if (bs > kMaxBlock) return FSE_ERR_UNSUPPORTED;
    return with_dtables_n(p, d_in, slot_bytes, d_comp_len, (n_total + bs - 1) / bs, stream, run);
}

}  // namespace capi
}  // namespace fsehip
