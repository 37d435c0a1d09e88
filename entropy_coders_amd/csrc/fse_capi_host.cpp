// fse_capi_host.cpp -- the host-pointer calls of the C ABI.
//
// The reference-shaped entry points (fse_compress2, fse_decompress2,
// histogram_count, the building blocks, the bit calls) stage host buffers
// through device memory (fse_workspace.h: g_stage, g_pin) and run the same
// kernels as the batched API on the null stream; there is no CPU compute
// path: without a usable HIP device they return FSE_ERR_NO_DEVICE.
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "fse_capi_common.h"

using namespace fsehip::capi;

namespace {

struct Meta {
    uint32_t comp_len;
    uint32_t payload_bits;
    int32_t status;
    uint32_t pad;
};

// an error after work was enqueued: nothing may still read or write the pinned buffers
int sync_fail(int rc) {
    (void)hipStreamSynchronize(nullptr);
    return rc;
}

// The end of compress_one / decompress_one: one kernel returns the record
// (d_meta) and the first pin_out bytes of d_out through the pinned h_ret
// (record at 0, bytes at 256); the rest of a longer output comes by
// hipMemcpy.  `len` is the record's field that holds the byte count.
int host_return(const uint8_t* d_meta, const uint8_t* d_out, uint32_t Meta::*len, uint8_t* h_ret, size_t pin_out,
                uint8_t* dst, size_t dst_cap, size_t* dst_len, Meta* h) {
    const uint32_t* d_len = &(reinterpret_cast<const Meta*>(d_meta)->*len);
    if (fsehip::launch_host_return(d_meta, d_out, d_len, h_ret, h_ret + 256, (uint32_t)pin_out, nullptr) != hipSuccess)
        return sync_fail(FSE_ERR_HIP);
    if (hipStreamSynchronize(nullptr) != hipSuccess) return FSE_ERR_HIP;
    memcpy(h, h_ret, sizeof *h);
    if (h->status != FSE_OK) return h->status;
    const size_t n = h->*len;
    // compress_one's test (a decoder stays within the out_cap it was given)
    if (*dst_len > dst_cap || dst_cap - *dst_len < n) return FSE_ERR_DST_TOO_SMALL;
    const size_t head = std::min<size_t>(n, pin_out);
    memcpy(dst + *dst_len, h_ret + 256, head);
    if (n > head && hipMemcpy(dst + *dst_len + head, d_out + head, n - head, hipMemcpyDeviceToHost) != hipSuccess)
        return FSE_ERR_HIP;
    *dst_len += n;
    return FSE_OK;
}

int compress_one(const uint8_t* src, size_t n, uint32_t table_log, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                 uint64_t* payload_bits, uint32_t nstates = 2) {
    if (!dst_len) return FSE_ERR_BAD_ARG;
    if (n == 0) return FSE_ERR_EMPTY;  // size.ilog2() panics (histogram.rs:266)
    if (n > kMaxBlock) return FSE_ERR_UNSUPPORTED;
    if (table_log > 15) table_log = 15;  // Histogram::normalize clamps (histogram.rs:96)
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    fsehip_params p{(uint32_t)round_up(n, 16), table_log, 0, table_log ? std::max<uint32_t>(table_log, 11) : 11,
                    nstates};
    const uint64_t slot = fsehip_slot_bytes(p.block_size, p.max_table_log);
    const size_t in_bytes = round_up(n, 16);
    const size_t pin_out = std::min<size_t>(slot, kPinOut);
    uint8_t* d_src = g_stage.get(STAGE_SRC, in_bytes + 16);
    uint8_t* d_out = g_stage.get(STAGE_OUT, slot);
    uint8_t* d_meta = g_stage.get(STAGE_REC, sizeof(Meta));
    uint8_t* h_in = g_pin.get(PIN_IN, in_bytes);
    uint8_t* h_ret = g_pin.get(PIN_RET, 256 + pin_out);
    if (!d_src || !d_out || !d_meta || !h_in || !h_ret) return FSE_ERR_HIP;
    memcpy(h_in, src, n);
    if (hipMemcpyAsync(d_src, h_in, in_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    Meta* m = reinterpret_cast<Meta*>(d_meta);
    int rc = fsehip_compress_blocks(&p, d_src, n, d_out, slot, &m->comp_len, &m->payload_bits, nullptr,
                                    &m->status, nullptr);
    if (rc) return sync_fail(rc);
    Meta h;
    rc = host_return(d_meta, d_out, &Meta::comp_len, h_ret, pin_out, dst, dst_cap, dst_len, &h);
    if (rc == FSE_OK && payload_bits) *payload_bits = h.payload_bits;
    return rc;
}

// Host block decode (reference mode: the raw length is not in the format):
// the block's table (stride 15, any L) and the serial decoder with the
// reference's own termination within the caller's capacity.
constexpr uint32_t LOG_MIN_HOST = 5;  // TABLE_LOG_MIN (lib.rs:9)
// The header's first field is the table log (histogram.rs:438: read(4) + 5).
// The host decoders size the tables and pick the kernels by its class: <= 11,
// 12 (the kernels of both keep the table in LDS) and 13 and above; a bad
// header fails the parse in any class.
constexpr uint32_t kClassLog[3] = {11, 12, 15};
struct LogClass {
    uint32_t log;  // above 15 only in a corrupt header
    int index;
    uint32_t max_table_log;  // kClassLog[index]
};
LogClass host_log_class(uint8_t first_byte) {
    const uint32_t L = (uint32_t)(first_byte & 15u) + LOG_MIN_HOST;
    const int c = L <= 11u ? 0 : L == 12u ? 1 : 2;
    return {L, c, kClassLog[c]};
}
int decompress_one(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len, uint32_t nstates) {
    if (!dst_len || *dst_len > dst_cap) return FSE_ERR_BAD_ARG;
    if (n == 0) return FSE_ERR_EMPTY;  // BitStreamReader::new asserts (stream_reader.rs:17)
    if (n > (1u << 30)) return FSE_ERR_UNSUPPORTED;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const uint64_t padded = round_up(n + 16, 256);
    const uint64_t cap64 = std::min<uint64_t>(dst_cap - *dst_len, 0x7FFFFFFFu);
    const size_t pin_out = std::min<size_t>(cap64, kPinOut);
    // one device buffer: the result record (Meta) at 0, the stream at 256
    uint8_t* d_buf = g_stage.get(STAGE_SRC, 256 + padded);
    uint8_t* d_out = g_stage.get(STAGE_OUT, std::max<uint64_t>(cap64, 16));
    const uint32_t mtl = host_log_class(src[0]).max_table_log;
    uint8_t* d_dt = g_stage.get(STAGE_TABLES, fsehip_dtable_bytes(mtl) + 16);
    uint8_t* h_in = g_pin.get(PIN_IN, 256 + padded);
    uint8_t* h_ret = g_pin.get(PIN_RET, 256 + pin_out);
    if (!d_buf || !d_out || !d_dt || !h_in || !h_ret) return FSE_ERR_HIP;
    // the record and the zero-padded stream go over in one copy
    const Meta h0{(uint32_t)n, 0, 0, 0};
    memcpy(h_in, &h0, sizeof h0);
    memcpy(h_in + 256, src, n);
    memset(h_in + 256 + n, 0, padded - n);
    if (hipMemcpyAsync(d_buf, h_in, 256 + padded, hipMemcpyHostToDevice, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    uint8_t* d_in = d_buf + 256;
    Meta* m = reinterpret_cast<Meta*>(d_buf);
    fsehip_params p{0, 0, 0, mtl, nstates};
    uint32_t* dt = reinterpret_cast<uint32_t*>(d_dt);
    int32_t* info = reinterpret_cast<int32_t*>(d_dt + fsehip_dtable_bytes(mtl));
    int rc = fsehip_build_dtables(&p, d_in, padded, &m->comp_len, 1, dt, info, nullptr);
    if (rc) return sync_fail(rc);
    // payload_bits holds the decoded byte count (0 on error)
    if (mtl == 11) {
        // the latency-first single-stream decoder (chain on the scalar unit,
        // fused table through the scalar cache, payload streamed by chunks)
        fsehip::DecParams P = ref_mode_params(nstates, d_in, padded, &m->comp_len, d_out, 0, (uint32_t)cap64, 1,
                                              &m->status, &m->payload_bits, dt, info);
        P.states = reinterpret_cast<uint32_t*>(g_stage.get(STAGE_FTAB, fsehip::single_ftab_bytes()));  // fused bulk table
        if (!P.states) return sync_fail(FSE_ERR_HIP);
        if (fsehip::launch_single(P, 11, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    } else {
        rc = decompress_impl(&p, d_in, padded, &m->comp_len, nullptr, d_out, 0, nullptr, &m->status, &m->payload_bits,
                             (uint32_t)cap64, nullptr, dt, info);
        if (rc) return sync_fail(rc);
    }
    Meta h;
    return host_return(d_buf, d_out, &Meta::payload_bits, h_ret, pin_out, dst, dst_cap, dst_len, &h);
}

// fn(i) for i in [0, n) on up to 16 host threads (contiguous ranges), one
// thread per ~2 MB of copying: the staging memcpys of a large batch are the
// call's host-side cost (one core copies ~5-10 GB/s).
template <class Fn>
void for_streams(size_t n, uint64_t bytes, Fn fn) {
    const size_t T = (size_t)std::min<uint64_t>({16, (bytes >> 21) + 1, n});
    if (T <= 1) {
        for (size_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::vector<std::thread> th;
    auto range = [&](size_t t) {
        for (size_t i = n * t / T; i < n * (t + 1) / T; ++i) fn(i);
    };
    size_t started = 1;  // ranges handed to threads (range 0 runs here)
    try {
        th.reserve(T - 1);
        for (; started < T; ++started) th.emplace_back(range, started);
    } catch (...) {  // no thread to be had (resource limits): the rest runs here
    }
    range(0);
    for (size_t t = started; t < T; ++t) range(t);
    for (auto& x : th) x.join();
}

// Batches of at most this many streams at table log <= 11 decode one stream
// per wave on the scalar unit (single_decode_kernel), larger ones on the
// serial ring kernel (32 lanes of chains per CU).  Measured with 64 KiB C2
// streams, host buffers in and out (tools/many_ab.py, profiles/r06/many/):
// 3 streams 2.13 -> 1.48 ms, 16 streams 2.27 -> 2.08 ms (1-state 3.38 ->
// 2.01), but 64 streams 2.62 -> 2.90: the scalar chains share their CU's
// scalar cache, whose 16 KiB fused tables then evict one another.
#ifndef FSE_SCALAR_MANY
#define FSE_SCALAR_MANY 32
#endif
constexpr size_t kScalarMany = FSE_SCALAR_MANY;

// One batch: the streams idx[0..m) (each 0 < n <= kManyStream, non-null).
// One pinned staging copy in (lengths + streams at a common stride), the
// header parse + decode tables + serial decoders of fsehip_decompress_streams
// on the default stream (one chain per stream, thousands at once), one copy
// back of the per-stream record (length, status) and output.
int decompress_batch(const uint8_t* const* srcs, const size_t* src_lens, const std::vector<size_t>& idx, uint8_t* dst,
                     size_t dst_stride, size_t* dst_lens, int32_t* statuses, uint32_t nstates) {
    const size_t m = idx.size();
    size_t maxn = 1;
    int cls = 0;
    uint64_t in_total = 0;
    for (size_t i : idx) {
        maxn = std::max(maxn, src_lens[i]);
        in_total += src_lens[i];
        cls = std::max(cls, host_log_class(srcs[i][0]).index);
    }
    const uint32_t mtl = kClassLog[cls];
    const uint64_t in_stride = round_up(maxn + 32, 256);
    const uint64_t out_stride = round_up(dst_stride, 16);
    const uint64_t head = round_up(4ull * m, 256);  // the lengths ahead of the streams
    const uint64_t in_bytes = head + in_stride * m;
    const uint64_t rec = round_up(8ull * m, 256);  // (length, status) per stream ahead of the output
    const uint64_t out_bytes = rec + out_stride * m;
    uint8_t* d_in = g_stage.get(STAGE_BATCH_IN, in_bytes);
    uint8_t* d_out = g_stage.get(STAGE_BATCH_OUT, out_bytes);
    uint8_t* h_in = g_pin.get(PIN_IN, in_bytes);
    uint8_t* h_out = g_pin.get(PIN_RET, out_bytes);
    if (!d_in || !d_out || !h_in || !h_out) return FSE_ERR_HIP;
    uint32_t* lens = reinterpret_cast<uint32_t*>(h_in);
    for_streams(m, in_total, [&](size_t k) {
        const size_t n = src_lens[idx[k]];
        uint8_t* s = h_in + head + k * in_stride;
        lens[k] = (uint32_t)n;
        memcpy(s, srcs[idx[k]], n);
        memset(s + n, 0, std::min<uint64_t>(in_stride, round_up(n, 32) + 32) - n);
    });
    if (hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    const uint32_t* d_len = reinterpret_cast<const uint32_t*>(d_in);
    uint32_t* d_olen = reinterpret_cast<uint32_t*>(d_out);
    int32_t* d_stat = reinterpret_cast<int32_t*>(d_out + 4ull * m);
    const fsehip_params p{(uint32_t)out_stride, 0, 0, mtl, nstates};
    int rc = with_dtables_n(&p, d_in + head, in_stride, d_len, m, nullptr,
                            [&](const uint32_t* dt, const int32_t* info, Lease& lease) {
                                fsehip::DecParams P =
                                    ref_mode_params(nstates, d_in + head, in_stride, d_len, d_out + rec,
                                                    (uint32_t)out_stride, (uint32_t)dst_stride, (uint32_t)m, d_stat,
                                                    d_olen, dt, info);
                                if (mtl == 11u && m <= kScalarMany) {
                                    // few streams: one scalar-unit chain each (the single
                                    // call's kernel), ~2x faster per chain than a ring lane
                                    P.states = static_cast<uint32_t*>(
                                        lease.get(SCRATCH_STATES, fsehip::single_ftab_bytes() * m, true));
                                    if (P.states) return rc_of(fsehip::launch_single(P, 11, nullptr));
                                }
                                defer_symbols(lease, P, kern_lmax(mtl));
                                return rc_of(fsehip::launch_decode(P, kern_lmax(mtl), nullptr));
                            });
    if (rc) return sync_fail(rc);
    if (hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    if (hipStreamSynchronize(nullptr) != hipSuccess) return FSE_ERR_HIP;
    const uint32_t* olen = reinterpret_cast<const uint32_t*>(h_out);
    const int32_t* ost = reinterpret_cast<const int32_t*>(h_out + 4ull * m);
    uint64_t out_total = 0;
    for (size_t k = 0; k < m; ++k) out_total += ost[k] == FSE_OK ? olen[k] : 0;
    for_streams(m, out_total, [&](size_t k) {
        const size_t i = idx[k];
        statuses[i] = ost[k];
        dst_lens[i] = ost[k] == FSE_OK ? olen[k] : 0;
        if (ost[k] == FSE_OK) memcpy(dst + i * dst_stride, h_out + rec + k * out_stride, olen[k]);
    });
    return FSE_OK;
}

// Many host streams in one call (lib.rs:187-248 per stream).  Streams the
// batch takes (up to 4 MiB each) go in groups of at most kManyStage bytes
// of staging each way; longer ones, and calls of one or two streams, take
// the single-stream path one by one (its chain is ~2x faster than a serial
// ring chain, and a lone long stream should not set the stride of all).
constexpr size_t kManyStream = size_t(4) << 20;
constexpr uint64_t kManyStage = uint64_t(512) << 20;
int decompress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                    size_t dst_stride, size_t* dst_lens, int32_t* statuses, uint32_t nstates) {
    if (n_streams == 0) return FSE_OK;
    if (!srcs || !src_lens || !dst || !dst_lens || !statuses || dst_stride == 0) return FSE_ERR_BAD_ARG;
    if (n_streams > (1u << 24) || dst_stride > 0x7FFFFFFFull) return FSE_ERR_UNSUPPORTED;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const uint64_t out_stride = round_up(dst_stride, 16);
    // Groups by the class of the header's table log (host_log_class): each
    // takes the kernels and decode-table stride of its class, so one stream
    // with a large (or corrupt) log neither moves the others off the L <= 11
    // kernels nor multiplies their table scratch; a log above 15 can only
    // fail, on the single path.  A group is capped by its staging bytes and
    // by its decode-table + header scratch.
    std::vector<size_t> single, group[3];
    uint64_t gmax[3] = {0, 0, 0};  // each group's largest staged stream
    auto run_group = [&](int c) -> int {
        std::vector<size_t>& g = group[c];
        gmax[c] = 0;
        if (g.empty()) return FSE_OK;
        if (g.size() <= 2) {  // not worth the batch kernels' fixed cost
            single.insert(single.end(), g.begin(), g.end());
            g.clear();
            return FSE_OK;
        }
        const int rc = decompress_batch(srcs, src_lens, g, dst, dst_stride, dst_lens, statuses, nstates);
        g.clear();
        return rc;
    };
    for (size_t i = 0; i < n_streams; ++i) {
        const size_t n = src_lens[i];
        if (n == 0 || !srcs[i] || n > kManyStream || n_streams <= 2 || out_stride > kManyStage / 4) {
            single.push_back(i);  // statuses and long streams: the single call's own path
            continue;
        }
        const LogClass lc = host_log_class(srcs[i][0]);
        if (lc.log > 15u) {
            single.push_back(i);
            continue;
        }
        const int c = lc.index;
        const uint64_t in_s = round_up(n + 32, 256), gm = std::max(gmax[c], in_s);
        const uint64_t per_table = fsehip_dtable_bytes(lc.max_table_log) + fsehip::hdr_scratch_bytes(1) + 8u;
        const uint64_t m1 = group[c].size() + 1;
        if (!group[c].empty() && (m1 * std::max(gm, out_stride) > kManyStage || m1 * per_table > kManyStage)) {
            if (int rc = run_group(c)) return rc;
        }
        group[c].push_back(i);
        gmax[c] = std::max(gmax[c], in_s);
    }
    for (int c = 0; c < 3; ++c)
        if (int rc = run_group(c)) return rc;
    for (size_t i : single) {
        size_t len = 0;
        const int32_t st = src_lens[i] == 0 ? FSE_ERR_EMPTY  // BitStreamReader::new asserts (stream_reader.rs:17)
                           : !srcs[i]      ? FSE_ERR_BAD_ARG
                                           : decompress_one(srcs[i], src_lens[i], dst + i * dst_stride, dst_stride,
                                                            &len, nstates);
        if (st == FSE_ERR_HIP || st == FSE_ERR_NO_DEVICE) return st;
        statuses[i] = st;
        dst_lens[i] = st == FSE_OK ? len : 0;
    }
    return FSE_OK;
}

// Many host buffers compressed in one call (lib.rs:146-183 / 112-143 per
// buffer), the mirror image of decompress_many.  One batch: the buffers
// idx[0..m) (each 0 < n <= kMaxBlock, non-null) packed back to back at
// 16-byte aligned offsets behind their descriptors -- no common stride, and
// no over-read allowance: the streams kernel reads exactly [src_off, src_off
// + src_len) -- one copy in, fsehip_compress_streams into worst-case regions
// (so the device never runs out of room and DST_TOO_SMALL is decided here
// from the real length), the results compacted on the device
// (stream_offsets_kernel + copy_blocks_kernel), the records and then the
// compressed bytes copied back, and scattered to dst.
struct ManyRec {  // head of the device result buffer
    uint64_t total;
    uint64_t pad;
};
std::atomic<uint64_t> g_compress_stage{kManyStage};

int compress_batch(const uint8_t* const* srcs, const size_t* src_lens, const size_t* idx, size_t m, uint8_t* dst,
                   size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses, uint32_t nstates) {
    // input staging: descriptors | output offsets (for the compaction) | sources
    const uint64_t desc_bytes = round_up(sizeof(fsehip_stream_desc) * m, 256);
    const uint64_t ooff_bytes = round_up(8ull * m, 256);
    uint64_t in_total = 0, cap_total = 0;
    for (size_t k = 0; k < m; ++k) {
        in_total += round_up(src_lens[idx[k]], 16);
        cap_total += fsehip_stream_out_bytes((uint32_t)src_lens[idx[k]], 11);
    }
    const uint64_t in_bytes = desc_bytes + ooff_bytes + in_total;
    // result buffer: total | comp_len, payload_bits, status | packed offsets | packed streams
    const uint64_t rec_bytes = round_up(sizeof(ManyRec) + 12ull * m, 256);
    const uint64_t poff_bytes = round_up(8ull * m, 256);
    uint8_t* h_in = g_pin.get(PIN_IN, in_bytes);
    uint8_t* d_in = g_stage.get(STAGE_BATCH_IN, in_bytes);
    uint8_t* d_reg = g_stage.get(STAGE_BATCH_OUT, cap_total);
    uint8_t* d_res = g_stage.get(STAGE_BATCH_RES, rec_bytes + poff_bytes + cap_total);
    if (!h_in || !d_in || !d_reg || !d_res) return FSE_ERR_HIP;
    fsehip_stream_desc* desc = reinterpret_cast<fsehip_stream_desc*>(h_in);
    uint64_t* ooff = reinterpret_cast<uint64_t*>(h_in + desc_bytes);
    uint64_t so = 0, oo = 0;
    for (size_t k = 0; k < m; ++k) {
        const uint32_t n = (uint32_t)src_lens[idx[k]];
        const uint64_t cap = fsehip_stream_out_bytes(n, 11);
        desc[k] = fsehip_stream_desc{so, oo, n, (uint32_t)cap};
        ooff[k] = oo;
        so += round_up(n, 16);
        oo += cap;
    }
    uint8_t* h_src = h_in + desc_bytes + ooff_bytes;
    for_streams(m, in_total, [&](size_t k) { memcpy(h_src + desc[k].src_off, srcs[idx[k]], desc[k].src_len); });
    if (hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) return sync_fail(FSE_ERR_HIP);
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d_res + sizeof(ManyRec));
    uint32_t* d_bits = d_len + m;
    int32_t* d_stat = reinterpret_cast<int32_t*>(d_bits + m);
    uint64_t* d_poff = reinterpret_cast<uint64_t*>(d_res + rec_bytes);
    uint8_t* d_packed = d_res + rec_bytes + poff_bytes;
    int rc = fsehip_compress_streams(nstates, 0, 11, d_in + desc_bytes + ooff_bytes,
                                     reinterpret_cast<const fsehip_stream_desc*>(d_in), (uint32_t)m, d_reg, d_len,
                                     d_bits, d_stat, nullptr);
    if (rc) return sync_fail(rc);
    if (fsehip::launch_stream_offsets(d_len, (uint32_t)m, d_poff, reinterpret_cast<uint64_t*>(d_res), nullptr) !=
            hipSuccess ||
        fsehip::launch_copy(d_reg, reinterpret_cast<const uint64_t*>(d_in + desc_bytes), d_len, (uint32_t)m, d_packed,
                            d_poff, nullptr) != hipSuccess)
        return sync_fail(FSE_ERR_HIP);
    uint8_t* h_rec = g_pin.get(PIN_RET, rec_bytes);
    if (!h_rec) return sync_fail(FSE_ERR_HIP);
    if (hipMemcpyAsync(h_rec, d_res, sizeof(ManyRec) + 12ull * m, hipMemcpyDeviceToHost, nullptr) != hipSuccess)
        return sync_fail(FSE_ERR_HIP);
    if (hipStreamSynchronize(nullptr) != hipSuccess) return FSE_ERR_HIP;
    // the records leave the pinned buffer before it may grow for the streams (fse_workspace.h PinSlot)
    std::vector<uint32_t> rec(3 * m);
    const uint64_t total = reinterpret_cast<const ManyRec*>(h_rec)->total;
    memcpy(rec.data(), h_rec + sizeof(ManyRec), 12ull * m);
    const uint32_t *olen = rec.data(), *obits = olen + m;
    const int32_t* ost = reinterpret_cast<const int32_t*>(obits + m);
    if (total > cap_total) return FSE_ERR_HIP;
    uint8_t* h_out = g_pin.get(PIN_RET, std::max<uint64_t>(total, 16));
    if (!h_out) return FSE_ERR_HIP;
    if (total && hipMemcpy(h_out, d_packed, total, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    std::vector<uint64_t> poff(m);
    uint64_t po = 0;
    for (size_t k = 0; k < m; ++k) {
        poff[k] = po;
        po += round_up(olen[k], 16);
    }
    for_streams(m, total, [&](size_t k) {
        const size_t i = idx[k];
        int32_t st = ost[k];
        if (st == FSE_OK && olen[k] > dst_stride) st = FSE_ERR_DST_TOO_SMALL;
        statuses[i] = st;
        dst_lens[i] = st == FSE_OK ? olen[k] : 0;
        if (payload_bits) payload_bits[i] = st == FSE_OK ? obits[k] : 0;
        if (st == FSE_OK) memcpy(dst + i * dst_stride, h_out + poff[k], olen[k]);
    });
    return FSE_OK;
}

// A call of kCompressSingle buffers or fewer takes compress_one per buffer
// (one wave and one synchronise each); larger calls the batch, in groups of
// at most g_compress_stage bytes of staging each way.
constexpr size_t kCompressSingle = 1;
int compress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                  size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses, uint32_t nstates) {
    if (n_streams == 0) return FSE_OK;
    if (!srcs || !src_lens || !dst || !dst_lens || !statuses || dst_stride == 0) return FSE_ERR_BAD_ARG;
    if (n_streams > (1u << 24)) return FSE_ERR_UNSUPPORTED;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const uint64_t stage = g_compress_stage.load(std::memory_order_relaxed);
    std::vector<size_t> batch;
    uint64_t in_b = 0, out_b = 0;
    auto run = [&]() -> int {
        if (batch.empty()) return FSE_OK;
        int rc = FSE_OK;
        if (n_streams <= kCompressSingle) {
            for (size_t i : batch) {
                size_t len = 0;
                uint64_t bits = 0;
                const int st = compress_one(srcs[i], src_lens[i], 0, dst + i * dst_stride, dst_stride, &len, &bits,
                                            nstates);
                if (st == FSE_ERR_HIP || st == FSE_ERR_NO_DEVICE) return st;
                statuses[i] = st;
                dst_lens[i] = st == FSE_OK ? len : 0;
                if (payload_bits) payload_bits[i] = st == FSE_OK ? bits : 0;
            }
        } else {
            rc = compress_batch(srcs, src_lens, batch.data(), batch.size(), dst, dst_stride, dst_lens, payload_bits,
                                statuses, nstates);
        }
        batch.clear();
        in_b = out_b = 0;
        return rc;
    };
    for (size_t i = 0; i < n_streams; ++i) {
        const size_t n = src_lens[i];
        const int32_t st = n == 0 ? FSE_ERR_EMPTY  // size.ilog2() panics (histogram.rs:266)
                           : !srcs[i] ? FSE_ERR_BAD_ARG
                           : n > kMaxBlock ? FSE_ERR_UNSUPPORTED
                                           : FSE_OK;
        if (st != FSE_OK) {
            statuses[i] = st;
            dst_lens[i] = 0;
            if (payload_bits) payload_bits[i] = 0;
            continue;
        }
        const uint64_t a = round_up(n, 16) + sizeof(fsehip_stream_desc) + 8, o = fsehip_stream_out_bytes((uint32_t)n, 11) + 20;
        if (!batch.empty() && (in_b + a > stage || out_b + o > stage))
            if (int rc = run()) return rc;
        batch.push_back(i);
        in_b += a;
        out_b += o;
    }
    return run();
}

// One normalisation on the GPU (fse_blocks.hip norm_kernel).
int normalize_dev(int mode, const uint8_t* src, size_t n, const fse_histogram* h, uint32_t log2,
                  fse_norm_histogram* out) {
    if (!out) return FSE_ERR_BAD_ARG;
    if (mode == 2 && n > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;  // histogram.rs:19 assert
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d_src = mode == 2 ? g_stage.get(STAGE_SRC, round_up(n, 16) + 16) : nullptr;
    uint8_t* d_io = g_stage.get(STAGE_REC, sizeof(fse_norm_histogram) + sizeof(fse_histogram) + 16);
    if ((mode == 2 && !d_src) || !d_io) return FSE_ERR_HIP;
    auto* d_nh = reinterpret_cast<fse_norm_histogram*>(d_io);
    auto* d_h = reinterpret_cast<fse_histogram*>(d_io + sizeof(fse_norm_histogram));
    int32_t* d_st = reinterpret_cast<int32_t*>(d_io + sizeof(fse_norm_histogram) + sizeof(fse_histogram));
    if (mode == 2 && n && hipMemcpy(d_src, src, n, hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    if (mode != 2 && hipMemcpy(d_h, h, sizeof(fse_histogram), hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    fsehip::NormArgs A{};
    A.mode = mode;
    A.src = d_src;
    A.n = n;
    A.counts = d_h->counts;
    if (mode != 2) {
        A.size = h->size;
        A.table_len = h->table_len;
    }
    A.log2 = log2;
    A.out = d_nh;
    A.status = d_st;
    if (fsehip::launch_norm(A, nullptr) != hipSuccess) return FSE_ERR_HIP;
    int32_t st = 0;
    if (hipMemcpy(&st, d_st, 4, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if (st != FSE_OK) return st;
    return rc_of(hipMemcpy(out, d_nh, sizeof(fse_norm_histogram), hipMemcpyDeviceToHost));
}

int table_new(const fse_norm_histogram* nh, int enc, void* out, size_t bytes) {
    if (!nh || !out) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d = g_stage.get(STAGE_BATCH_IN, sizeof(fse_norm_histogram) + 16 + bytes);
    if (!d) return FSE_ERR_HIP;
    auto* d_nh = reinterpret_cast<fse_norm_histogram*>(d);
    int32_t* d_st = reinterpret_cast<int32_t*>(d + sizeof(fse_norm_histogram));
    uint8_t* d_tab = d + sizeof(fse_norm_histogram) + 16;
    if (hipMemcpy(d_nh, nh, sizeof(*nh), hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    if (hipMemset(d_tab, 0, bytes) != hipSuccess) return FSE_ERR_HIP;
    if (fsehip::launch_table(d_nh, enc, reinterpret_cast<fse_encode_table*>(d_tab),
                             reinterpret_cast<fse_decode_table*>(d_tab), d_st, nullptr) != hipSuccess)
        return FSE_ERR_HIP;
    int32_t st = 0;
    if (hipMemcpy(&st, d_st, 4, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if (st != FSE_OK) return st;
    return rc_of(hipMemcpy(out, d_tab, bytes, hipMemcpyDeviceToHost));
}

int bits_read_host(const uint8_t* src, size_t n, uint64_t total_bits, int stack, const uint8_t* nbits,
                   const uint8_t* ops, size_t count, uint32_t* vals, uint64_t res[3]) {
    if ((count && (!nbits || !vals)) || (!src && n)) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d_in = g_stage.get(STAGE_SRC, round_up(n, 4) + 16);
    uint8_t* d_nb = g_stage.get(STAGE_OUT, count + 16);
    uint8_t* d_v = g_stage.get(STAGE_BATCH_OUT, count * 4 + 16);
    uint8_t* d_res = g_stage.get(STAGE_REC, 32);
    uint8_t* d_ops = ops ? g_stage.get(STAGE_TABLES, count + 16) : nullptr;
    if (!d_in || !d_nb || !d_v || !d_res || (ops && !d_ops)) return FSE_ERR_HIP;
    if (hipMemset(d_in, 0, round_up(n, 4) + 16) != hipSuccess) return FSE_ERR_HIP;
    if (n && hipMemcpy(d_in, src, n, hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    if (count && hipMemcpy(d_nb, nbits, count, hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    if (ops && count && hipMemcpy(d_ops, ops, count, hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    uint64_t* r = reinterpret_cast<uint64_t*>(d_res);
    int rc = stack ? fsehip_bitstack_read(d_in, n, d_nb, count, reinterpret_cast<uint32_t*>(d_v), r, nullptr)
                   : fsehip_bitstream_read_ops(d_in, n, total_bits, d_nb, d_ops, count,
                                               reinterpret_cast<uint32_t*>(d_v), r, nullptr);
    if (rc) return rc;
    if (hipMemcpy(res, r, 24, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if ((int64_t)res[2] != FSE_OK) return (int)(int64_t)res[2];
    if (res[0] && hipMemcpy(vals, d_v, res[0] * 4, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    return FSE_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- host API

int fse_compress2(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                  uint64_t* payload_bits) {
    return compress_one(src, n, 0, dst, dst_cap, dst_len, payload_bits);
}

int fse_compress2_log(const uint8_t* src, size_t n, uint32_t table_log, uint8_t* dst, size_t dst_cap,
                      size_t* dst_len, uint64_t* payload_bits) {
    // Histogram::normalize clamps any request into 5..15 (histogram.rs:96):
    // 0 acts as 5 (table_log 0 in the batched params means NormHistogram::new)
    return compress_one(src, n, std::max<uint32_t>(table_log, 5u), dst, dst_cap, dst_len, payload_bits);
}

int fse_decompress2(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    return decompress_one(src, n, dst, dst_cap, dst_len, 2);
}

int fse_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len, uint64_t* payload_bits) {
    // lib.rs:112-143; n == 1 is valid here (a lone seed state), unlike fse_compress2
    return compress_one(src, n, 0, dst, dst_cap, dst_len, payload_bits, 1);
}

int fse_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    return decompress_one(src, n, dst, dst_cap, dst_len, 1);
}

int fse_decompress2_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                         size_t dst_stride, size_t* dst_lens, int32_t* statuses) {
    return decompress_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, statuses, 2);
}

int fse_decompress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                        size_t dst_stride, size_t* dst_lens, int32_t* statuses) {
    return decompress_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, statuses, 1);
}

int fse_compress2_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                       size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses) {
    return compress_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, payload_bits, statuses, 2);
}

int fse_compress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                      size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses) {
    return compress_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, payload_bits, statuses, 1);
}

int histogram_count(const uint8_t* src, size_t n, uint32_t counts[256], uint32_t* table_len) {
    if (!counts) return FSE_ERR_BAD_ARG;
    if (n > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;  // histogram.rs:19 assert
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d_src = g_stage.get(STAGE_SRC, round_up(n, 16) + 16);
    uint8_t* d_cnt = g_stage.get(STAGE_REC, 257 * 4);
    if (!d_src || !d_cnt) return FSE_ERR_HIP;
    if (n && hipMemcpy(d_src, src, n, hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    uint32_t* c = reinterpret_cast<uint32_t*>(d_cnt);
    hipError_t e = fsehip::launch_histogram(d_src, n, (uint32_t)std::max<size_t>(n, 1), 1, c, c + 256, nullptr);
    if (e != hipSuccess) return FSE_ERR_HIP;
    uint32_t h[257];
    if (hipMemcpy(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    memcpy(counts, h, 256 * sizeof(uint32_t));
    if (table_len) *table_len = h[256];
    return FSE_OK;
}

// ------------------------------------------------------- building blocks

int histogram_new(const uint8_t* src, size_t n, fse_histogram* out) {
    if (!out) return FSE_ERR_BAD_ARG;
    uint32_t tl = 0;
    int rc = histogram_count(src, n, out->counts, &tl);
    if (rc) return rc;
    out->size = (uint32_t)n;
    out->table_len = tl;
    return FSE_OK;
}

int histogram_normalize(const fse_histogram* h, uint32_t log2, fse_norm_histogram* out) {
    if (!h || h->table_len > 256) return FSE_ERR_BAD_ARG;
    return normalize_dev(0, nullptr, 0, h, log2, out);
}

int histogram_normalize_optimal(const fse_histogram* h, fse_norm_histogram* out) {
    if (!h || h->table_len > 256) return FSE_ERR_BAD_ARG;
    return normalize_dev(1, nullptr, 0, h, 0, out);
}

int norm_histogram_new(const uint8_t* src, size_t n, fse_norm_histogram* out) {
    if (!src && n) return FSE_ERR_BAD_ARG;
    return normalize_dev(2, src, n, nullptr, 0, out);
}

int norm_histogram_write(const fse_norm_histogram* nh, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                         uint64_t* bits_written) {
    if (!nh || !dst_len || *dst_len > dst_cap) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d = g_stage.get(STAGE_REC, sizeof(fse_norm_histogram) + 16 + 512);
    if (!d) return FSE_ERR_HIP;
    auto* d_nh = reinterpret_cast<fse_norm_histogram*>(d);
    uint32_t* d_meta = reinterpret_cast<uint32_t*>(d + sizeof(fse_norm_histogram));  // bits, status
    uint8_t* d_out = d + sizeof(fse_norm_histogram) + 16;
    if (hipMemcpy(d_nh, nh, sizeof(*nh), hipMemcpyHostToDevice) != hipSuccess) return FSE_ERR_HIP;
    if (fsehip::launch_hdr_write(d_nh, d_out, d_meta, reinterpret_cast<int32_t*>(d_meta + 1), nullptr) != hipSuccess)
        return FSE_ERR_HIP;
    uint32_t meta[2];
    if (hipMemcpy(meta, d_meta, 8, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if ((int32_t)meta[1] != FSE_OK) return (int32_t)meta[1];
    const size_t len = (meta[0] + 7u) / 8u;
    if (dst_cap - *dst_len < len) return FSE_ERR_DST_TOO_SMALL;
    if (len && (!dst || hipMemcpy(dst + *dst_len, d_out, len, hipMemcpyDeviceToHost) != hipSuccess))
        return FSE_ERR_HIP;
    *dst_len += len;
    if (bits_written) *bits_written = meta[0];
    return FSE_OK;
}

int norm_histogram_read(const uint8_t* src, size_t n, fse_norm_histogram* out, size_t* consumed) {
    if (!out || (!src && n)) return FSE_ERR_BAD_ARG;
    if (n == 0) return FSE_ERR_EMPTY;  // BitStreamReader::new asserts a non-empty slice (stream_reader.rs:17)
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const size_t take = std::min<size_t>(n, 512);  // a header never exceeds 483 bytes (write_bound)
    uint8_t* d = g_stage.get(STAGE_REC, sizeof(fse_norm_histogram) + 16 + 528);
    if (!d) return FSE_ERR_HIP;
    auto* d_nh = reinterpret_cast<fse_norm_histogram*>(d);
    uint32_t* d_meta = reinterpret_cast<uint32_t*>(d + sizeof(fse_norm_histogram));  // used, status
    uint8_t* d_in = d + sizeof(fse_norm_histogram) + 16;
    if (hipMemset(d_in, 0, 528) != hipSuccess || hipMemcpy(d_in, src, take, hipMemcpyHostToDevice) != hipSuccess)
        return FSE_ERR_HIP;
    // the reader sees the whole slice's length (its bounds checks), the
    // header's bits come from the first 512 bytes
    if (fsehip::launch_hdr_read(d_in, (uint32_t)std::min<size_t>(n, 0xFFFFFFFFu), d_nh, d_meta,
                                reinterpret_cast<int32_t*>(d_meta + 1), nullptr) != hipSuccess)
        return FSE_ERR_HIP;
    uint32_t meta[2];
    if (hipMemcpy(meta, d_meta, 8, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if ((int32_t)meta[1] != FSE_OK) return (int32_t)meta[1];
    if (hipMemcpy(out, d_nh, sizeof(*out), hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    if (consumed) *consumed = meta[0];
    return FSE_OK;
}

int encode_table_new(const fse_norm_histogram* nh, fse_encode_table* out) {
    return table_new(nh, 1, out, sizeof(fse_encode_table));
}

int decode_table_new(const fse_norm_histogram* nh, fse_decode_table* out) {
    return table_new(nh, 0, out, sizeof(fse_decode_table));
}

int fse_compress_nh(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                    uint64_t* payload_bits, fse_norm_histogram* nh) {
    const size_t at = dst_len ? *dst_len : 0;
    int rc = fse_compress(src, n, dst, dst_cap, dst_len, payload_bits);
    if (rc || !nh) return rc;
    // the returned NormHistogram is the one the block's header carries
    return norm_histogram_read(dst + at, *dst_len - at, nh, nullptr);
}

// ------------------------------------------------------------- bitstream

int bitstack_write(const uint32_t* vals, const uint8_t* nbits, size_t count, uint8_t* dst, size_t dst_cap,
                   size_t* dst_len, uint64_t* bits_written) {
    if (!dst_len || *dst_len > dst_cap || (count && (!vals || !nbits))) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    uint8_t* d_v = g_stage.get(STAGE_SRC, count * 4 + 16);
    uint8_t* d_nb = g_stage.get(STAGE_OUT, count + 16);
    uint8_t* d_out = g_stage.get(STAGE_BATCH_OUT, count * 4 + 16);
    uint8_t* d_tot = g_stage.get(STAGE_REC, 16);
    if (!d_v || !d_nb || !d_out || !d_tot) return FSE_ERR_HIP;
    if (count && (hipMemcpy(d_v, vals, count * 4, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(d_nb, nbits, count, hipMemcpyHostToDevice) != hipSuccess))
        return FSE_ERR_HIP;
    uint64_t* tot = reinterpret_cast<uint64_t*>(d_tot);
    int rc = fsehip_bitstack_write(reinterpret_cast<const uint32_t*>(d_v), d_nb, count, d_out, count * 4 + 16, tot,
                                   nullptr);
    if (rc) return rc;
    uint64_t bits = 0;
    if (hipMemcpy(&bits, tot, 8, hipMemcpyDeviceToHost) != hipSuccess) return FSE_ERR_HIP;
    const size_t len = (size_t)((bits + 7u) / 8u);
    if (dst_cap - *dst_len < len) return FSE_ERR_DST_TOO_SMALL;
    if (len && (!dst || hipMemcpy(dst + *dst_len, d_out, len, hipMemcpyDeviceToHost) != hipSuccess))
        return FSE_ERR_HIP;
    *dst_len += len;
    if (bits_written) *bits_written = bits;
    return FSE_OK;
}

int bitstack_read(const uint8_t* src, size_t n, const uint8_t* nbits, size_t count, uint32_t* vals, size_t* n_read,
                  int* finished) {
    uint64_t res[3] = {0, 0, 0};
    int rc = bits_read_host(src, n, 0, 1, nbits, nullptr, count, vals, res);
    if (rc) return rc;
    if (n_read) *n_read = (size_t)res[0];
    // finish() after the successful reads: all bits consumed (reads stop at
    // the first None, which consumes nothing)
    if (finished) *finished = res[0] == count ? (int)res[1] : 0;
    return FSE_OK;
}

int bitstream_read_ops(const uint8_t* src, size_t n, uint64_t total_bits, const uint8_t* nbits, const uint8_t* ops,
                       size_t count, uint32_t* vals, size_t* n_done, uint64_t* bits_left) {
    if (ops)
        for (size_t i = 0; i < count; ++i)
            if (ops[i] > FSE_BITS_ADVANCE) return FSE_ERR_BAD_ARG;
    uint64_t res[3] = {0, 0, 0};
    int rc = bits_read_host(src, n, total_bits, 0, nbits, ops, count, vals, res);
    if (rc) return rc;
    if (n_done) *n_done = (size_t)res[0];
    if (bits_left) {
        uint64_t used = 0;
        for (size_t i = 0; i < res[0]; ++i)
            if (!ops || ops[i] != FSE_BITS_PEEK) used += std::min<uint32_t>(nbits[i], 32u);
        *bits_left = total_bits - used;
    }
    return FSE_OK;
}

int bitstream_read(const uint8_t* src, size_t n, uint64_t total_bits, const uint8_t* nbits, size_t count,
                   uint32_t* vals, size_t* n_read, uint64_t* bits_left) {
    return bitstream_read_ops(src, n, total_bits, nbits, nullptr, count, vals, n_read, bits_left);
}

// Tests only: the staging bytes per batch of fse_compress2_many /
// fse_compress_many (0 = the product's 512 MiB), so that a test reaches the
// split between batches with small inputs.  Returns the previous value.
uint64_t fsehipx_compress_many_stage(uint64_t bytes) {
    return g_compress_stage.exchange(bytes ? bytes : kManyStage, std::memory_order_relaxed);
}

}  // extern "C"
