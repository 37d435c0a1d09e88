// fse_estimate.cpp -- the size estimate's host side (fsehip.h sections 2g and
// 2i): the integer cost model applied to a caller's table, the choice among
// three kinds and, with a base, among four, the sizes and the container's
// kind from its magic.
//
// Plain C++ with no HIP include, as fse_elem.cpp: the same source builds
// into libfsehip.so and, with g++ alone, into the sanitizer fuzzes of
// tests/native/estimate_fuzz.cpp and estimate_diff_fuzz.cpp.  The kernels are fse_estimate.hip, the
// device calls fse_capi_estimate.cpp.
#include <string.h>

#include "../../include/fsehip.h"
#include "fse_estimate_host.h"

namespace {

bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }

// the kernel class of a max_table_log, as the encoder picks it (kern_lmax of
// lmax_for in fse_capi_common.h)
uint32_t kernel_class(uint32_t table_log, uint32_t max_table_log) {
    uint32_t m = max_table_log;
    if (m == 0u) m = table_log == 0u ? 11u : table_log < 11u ? 11u : table_log;
    return m <= 11u ? 11u : m >= 15u ? 15u : m;
}

}  // namespace

namespace fsehip {

uint32_t est_kernel_class(uint32_t table_log, uint32_t max_table_log) { return kernel_class(table_log, max_table_log); }

}  // namespace fsehip

extern "C" {

uint32_t fsehip_log2q8(uint32_t c) { return c >= 1u && c <= 32768u ? fsehip::log2q8(c) : 0u; }

int fsehip_estimate_choose(const uint64_t est[3]) {
    if (!est) return -1;
    int best = -1;
    for (int k = 0; k < 3; ++k)
        if (est[k] != FSEHIP_EST_NONE && (best < 0 || est[k] < est[best])) best = k;
    return best;
}

int fsehip_estimate_block_host(const uint32_t counts[256], uint32_t raw_len, const int32_t norm[256],
                               uint32_t norm_log, uint32_t hdr_bytes, const fsehip_frame_params* p,
                               fsehip_block_estimate* out) {
    if (!counts || !p || !out || p->nstates > 2u) return FSE_ERR_BAD_ARG;
    const uint32_t ns = p->nstates == 1u ? 1u : 2u;
    memset(out, 0, sizeof(*out));
    out->type = FSEHIP_EST_RAW;
    out->rec = raw_len;
    if (raw_len && counts[0] == raw_len) {
        out->type = FSEHIP_EST_RLE;
        out->rec = 1;
        return FSE_OK;
    }
    if (!norm || raw_len < 2u) return FSE_OK;  // the statistics refused the block; TOO_SHORT
    if (norm_log < 5u || norm_log > 15u) return FSE_ERR_BAD_ARG;
    uint64_t Q = 0;
    for (int s = 0; s < 256; ++s) {
        if (!counts[s]) continue;
        if (norm[s] == 0 || norm[s] < -1 || norm[s] > (int32_t)(1u << norm_log)) return FSE_ERR_BAD_ARG;
        Q += (uint64_t)counts[s] * fsehip::cost8(norm[s], norm_log);
    }
    if (norm_log > kernel_class(p->table_log, p->max_table_log)) return FSE_OK;  // the encoder's UNSUPPORTED
    uint64_t bits, rec;
    fsehip::est_record(Q, norm_log, hdr_bytes, raw_len, p->ckpt_interval, ns, &bits, &rec);
    if (rec < raw_len) {
        out->type = FSEHIP_EST_FSE;
        out->rec = (uint32_t)rec;
        out->bits = (uint32_t)bits;
        out->table_log = norm_log;
    }
    return FSE_OK;
}

int fsehip_container_kind(const uint8_t* buf, size_t len) {
    if (!buf && len) return FSE_ERR_BAD_ARG;
    if (len < 4u || buf[0] != 'F' || buf[1] != 'S' || buf[2] != 'E') return FSE_ERR_BAD_FRAME;
    switch (buf[3]) {
        case 'F': return (int)FSEHIP_KIND_FRAME;
        case 'P': return (int)FSEHIP_KIND_PLANES;
        case 'D': return (int)FSEHIP_KIND_DELTA;
        case 'K': return (int)FSEHIP_KIND_SEALED;
        case 'B': return (int)FSEHIP_KIND_DIFF;
        case 'M': return (int)FSEHIP_KIND_PACK;
        case 'V': return (int)FSEHIP_KIND_VPACK;
        case 'S': return (int)FSEHIP_KIND_SPACK;
        default: return FSE_ERR_BAD_FRAME;
    }
}

uint64_t fsehip_estimate_image_bytes(uint32_t kind, uint64_t n_elems, uint32_t elem_bytes) {
    if (kind > FSEHIP_KIND_DELTA || !width_ok(elem_bytes)) return 0;
    if (kind == FSEHIP_KIND_FRAME) return n_elems > UINT64_MAX / elem_bytes ? 0 : n_elems * elem_bytes;
    if (kind == FSEHIP_KIND_PLANES && elem_bytes == 1u) return 0;
    // w * roundup(n_elems, 16): fsehip_planes_scratch_bytes, fsehip_delta_scratch_bytes
    if (n_elems > UINT64_MAX - 15u) return 0;
    const uint64_t stride = (n_elems + 15u) & ~15ull;
    return stride > UINT64_MAX / elem_bytes ? 0 : stride * elem_bytes;
}

uint64_t fsehip_estimate_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes, uint32_t kind_mask,
                                       uint32_t block_size) {
    if (kind_mask == 0u || kind_mask > 7u || !width_ok(elem_bytes)) return 0;
    const uint64_t bs = block_size ? block_size : 65536u;
    uint64_t most = 0;
    for (uint32_t k = 0; k < 3; ++k) {
        if (!(kind_mask >> k & 1u) || (k == FSEHIP_KIND_PLANES && elem_bytes == 1u)) continue;
        const uint64_t image = fsehip_estimate_image_bytes(k, n_elems, elem_bytes);
        if (n_elems && !image) return 0;  // overflow
        const uint64_t nb = image / bs + (image % bs ? 1u : 0u);
        most = nb > most ? nb : most;
    }
    return most > UINT64_MAX / 1024u ? 0 : most * 1024u;
}

// ---- section 2i: the diff frame as fourth kind

int fsehip_estimate_choose_base(const uint64_t est[5]) {
    if (!est) return -1;
    int best = -1;
    for (int k = 0; k < 5; ++k)
        if (k != (int)FSEHIP_KIND_SEALED && est[k] != FSEHIP_EST_NONE && (best < 0 || est[k] < est[best])) best = k;
    return best;
}

uint64_t fsehip_estimate_base_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes, uint32_t kind_mask,
                                            uint32_t block_size) {
    if (kind_mask == 0u || (kind_mask & ~23u) || !width_ok(elem_bytes)) return 0;
    uint64_t most = kind_mask & 7u ? fsehip_estimate_scratch_bytes(n_elems, elem_bytes, kind_mask & 7u, block_size) : 0;
    if (kind_mask & 16u) {
        // the diff image has the delta image's size, the largest: where another overflows, it does
        const uint64_t diff = fsehip_estimate_scratch_bytes(n_elems, elem_bytes, 1u << FSEHIP_KIND_DELTA, block_size);
        if (n_elems && !diff) return 0;
        most = diff > most ? diff : most;
    }
    return most;
}

}  // extern "C"
