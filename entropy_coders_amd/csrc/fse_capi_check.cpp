// fse_capi_check.cpp -- the check-record calls of the C ABI (fsehip.h section
// 2f): header, CRC arithmetic and range rules in fse_check.cpp, kernels in
// fse_check.hip.  No workspace: what the kernels need beyond the caller's
// buffers (header bytes, the spans of a range list, the x^(8 n) constants of
// the combine) travels as kernel arguments, in stream order.
#include "fse_capi_common.h"
#include "fse_check_host.h"

using namespace fsehip::capi;

namespace {

// the whole content as one span
fsehip::CheckSpans whole(const uint8_t* d_content, uint64_t n_content, uint32_t check_log, uint32_t n_cb) {
    fsehip::CheckSpans S{};
    S.n = 1;
    fsehip::check_span(&S, 0, d_content, 0, 0, n_cb, n_content, check_log);
    return S;
}

}  // namespace

extern "C" {

int fsehip_check_build(uint32_t check_log, const uint8_t* d_content, uint64_t n_content, uint8_t* d_record,
                       fsehip_stream_t stream) {
    if (!d_record || (n_content && !d_content)) return FSE_ERR_BAD_ARG;
    if (check_log == 0) check_log = fsehip::kCheckLogMax;
    const uint64_t bytes = fsehip_check_bytes(n_content, check_log);
    if (!bytes) return FSE_ERR_UNSUPPORTED;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    fsehip_check_info info{};
    info.version = 1;
    info.algorithm = FSEHIP_CHECK_CRC32;
    info.check_log = check_log;
    info.n_content = n_content;
    info.n_cb = (uint32_t)((bytes - fsehip::kCheckHeaderBytes) / 4u);
    const fsehip::CheckSpans S = whole(d_content, n_content, check_log, info.n_cb);
    if (const int rc = fsehip::launch_check_crc(fsehip::kCheckBuild, S, d_content, n_content, check_log, d_record,
                                                nullptr, 0, nullptr, stream))
        return rc;
    return fsehip::launch_check_build_finish(&info, fsehip::check_combine_plan(n_content, check_log, info.n_cb),
                                             d_record, stream);
}

int fsehip_check_verify(const fsehip_check_info* info, const uint8_t* d_record, const uint8_t* d_content,
                        uint64_t n_content, int32_t* d_check_status, int32_t* d_result, fsehip_stream_t stream) {
    uint8_t hdr[32];
    if (!info || !d_record || !d_result || fsehip::check_info_ok(info) != FSE_OK ||
        fsehip_check_write_header(info, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    if (n_content != info->n_content || (n_content && (!d_content || !d_check_status))) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const fsehip::CheckSpans S = whole(d_content, n_content, info->check_log, info->n_cb);
    if (const int rc = fsehip::launch_check_crc(fsehip::kCheckVerify, S, d_content, n_content, info->check_log, nullptr,
                                                d_check_status, 0, nullptr, stream))
        return rc;
    return fsehip::launch_check_verify_finish(hdr, info,
                                              fsehip::check_combine_plan(n_content, info->check_log, info->n_cb),
                                              d_record, d_check_status, d_result, stream);
}

int fsehip_check_verify_ranges(const fsehip_check_info* info, const uint8_t* d_record,
                               const fsehip_frame_range* ranges, uint32_t n_ranges, const uint8_t* d_out,
                               uint64_t out_cap, int32_t* d_range_status, int32_t* d_result, fsehip_stream_t stream) {
    uint8_t hdr[32];
    if (!info || !d_record || !d_result || fsehip::check_info_ok(info) != FSE_OK ||
        fsehip_check_write_header(info, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    if (n_ranges && (!ranges || !d_range_status)) return FSE_ERR_BAD_ARG;
    bool any = false;
    for (uint32_t r = 0; r < n_ranges; ++r) any = any || ranges[r].len;
    if (any && !d_out) return FSE_ERR_BAD_ARG;
    if (const int rc = fsehip::check_ranges_ok(info, out_cap, ranges, n_ranges)) return rc;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    if (const int rc = fsehip::launch_check_ranges_begin(hdr, d_record, n_ranges, d_range_status, d_result, stream))
        return rc;
    const uint64_t B = 1ull << info->check_log;
    for (uint32_t r0 = 0; r0 < n_ranges; r0 += fsehip::kCheckSpans) {
        fsehip::CheckSpans S{};
        S.n = std::min(fsehip::kCheckSpans, n_ranges - r0);
        for (uint32_t i = 0; i < S.n; ++i) {
            const fsehip_frame_range& g = ranges[r0 + i];
            uint64_t b0, nb;
            fsehip::check_plan_range(info->n_content, info->check_log, g.src_off, g.len, &b0, &nb);
            // block b0 starts b0 * B - src_off bytes into the range's destination
            fsehip::check_span(&S, i, d_out, nb ? g.dst_off + (b0 * B - g.src_off) : 0, b0, nb, info->n_content,
                               info->check_log);
        }
        if (const int rc = fsehip::launch_check_crc(fsehip::kCheckRanges, S, d_out, info->n_content, info->check_log,
                                                    const_cast<uint8_t*>(d_record), d_range_status, r0, d_result,
                                                    stream))
            return rc;
    }
    return FSE_OK;
}

}  // extern "C"
