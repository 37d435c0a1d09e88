// fse_capi_shared.cpp -- shared-table coding (include/fsehip.h section 2c):
// NormHistogram's TryFrom on the host, the image build and the two batched
// calls over fse_shared.hip.
#include "fse_capi_common.h"

using namespace fsehip::capi;

namespace {

// the call-level checks the two batched calls share, before any device use
int shared_args(uint32_t nstates, const void* d_table, const void* d_in, const void* d_desc, uint32_t n_msgs,
                const void* d_out, const void* d_len, const void* d_status) {
    if (nstates > 2 || !d_table || !d_in || !d_desc || !d_out || !d_len || !d_status ||
        ((reinterpret_cast<uintptr_t>(d_table) | reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15u))
        return FSE_ERR_BAD_ARG;
    if (n_msgs > (1u << 24)) return FSE_ERR_UNSUPPORTED;
    return device_ok() ? FSE_OK : FSE_ERR_NO_DEVICE;
}

}  // namespace

extern "C" {

int norm_histogram_try_from(const int32_t table[256], fse_norm_histogram* out) {
    if (!table || !out) return FSE_ERR_BAD_ARG;
    uint64_t sum = 0;
    uint32_t last = 0;
    for (uint32_t i = 0; i < 256u; ++i) {
        sum += table[i] < 0 ? 0ull - (uint64_t)(int64_t)table[i] : (uint64_t)table[i];  // unsigned_abs
        if (table[i] != 0) last = i;
    }
    // 0.ilog2() panics; (1 << log2) != sum is Err(()) (histogram.rs:514-518)
    if (sum == 0 || (sum & (sum - 1))) return FSE_ERR_BAD_TABLE;
    for (uint32_t i = 0; i < 256u; ++i) out->norm[i] = table[i];
    out->log2 = 63u - (uint32_t)__builtin_clzll(sum);
    out->table_len = last + 1u;
    return FSE_OK;
}

uint64_t fsehip_shared_table_bytes(void) { return fsehip::SHARED_BYTES; }

int fsehip_shared_table_build(const fse_norm_histogram* d_nh, uint8_t* d_table, int32_t* d_status,
                              fsehip_stream_t stream) {
    if (!d_nh || !d_table || !d_status || (reinterpret_cast<uintptr_t>(d_table) & 15u)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return rc_of(fsehip::launch_shared_build(d_nh, d_table, d_status, static_cast<hipStream_t>(stream)));
}

uint64_t fsehip_shared_out_bytes(uint32_t src_len, uint32_t table_log) {
    const uint64_t L = std::min<uint32_t>(std::max<uint32_t>(table_log, 5u), fsehip::SHARED_LMAX);
    // <= L bits per symbol (fse.rs:170-186), both final states and the marker (lib.rs:178-181)
    return round_up(((uint64_t)src_len * L + 2 * L + 1 + 7) / 8, 16);
}

int fsehip_compress_shared(uint32_t nstates, const uint8_t* d_table, const uint8_t* d_src,
                           const fsehip_stream_desc* d_desc, uint32_t n_msgs, uint8_t* d_out, uint32_t* d_comp_len,
                           uint32_t* d_payload_bits, int32_t* d_status, fsehip_stream_t stream) {
    if (n_msgs == 0) return FSE_OK;
    if (const int rc = shared_args(nstates, d_table, d_src, d_desc, n_msgs, d_out, d_comp_len, d_status)) return rc;
    const fsehip::SharedParams P{nstates == 1 ? 1u : 2u, d_table, d_src, d_desc, n_msgs, d_out, d_comp_len,
                                 d_payload_bits, nullptr, d_status};
    return rc_of(fsehip::launch_shared_encode(P, static_cast<hipStream_t>(stream)));
}

int fsehip_decompress_shared(uint32_t nstates, const uint8_t* d_table, const uint8_t* d_in,
                             const fsehip_stream_desc* d_desc, uint32_t n_msgs, uint8_t* d_out,
                             const uint32_t* d_raw_len, uint32_t* d_out_len, int32_t* d_status, fsehip_stream_t stream) {
    if (n_msgs == 0) return FSE_OK;
    if (const int rc = shared_args(nstates, d_table, d_in, d_desc, n_msgs, d_out, d_out_len, d_status)) return rc;
    const fsehip::SharedParams P{nstates == 1 ? 1u : 2u, d_table, d_in, d_desc, n_msgs, d_out, d_out_len,
                                 nullptr, d_raw_len, d_status};
    return rc_of(fsehip::launch_shared_decode(P, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
