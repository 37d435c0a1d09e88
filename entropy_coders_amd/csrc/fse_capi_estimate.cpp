// fse_capi_estimate.cpp -- the size-estimate calls of the C ABI (fsehip.h
// sections 2g and 2i): the cost model, the choice and the sizes in
// fse_estimate.cpp, kernels in fse_estimate.hip.  fsehip_estimate and
// fsehip_estimate_base are, per kind, a zeroed count array, one histogram
// launch and one estimate launch on the caller's scratch and stream; the
// frame's counts are fsehip_histogram_blocks'.
#include "fse_capi_common.h"
#include "fse_estimate_host.h"

using namespace fsehip::capi;

namespace {

bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }
bool kind_takes(uint32_t kind, uint32_t w) { return kind != FSEHIP_KIND_PLANES || w != 1u; }

// the frame rules of fsehip_estimate_blocks for an image of n_image bytes
int frame_rules(const fsehip_frame_params* p, uint64_t n_image, uint32_t* bs, uint64_t* n_blocks) {
    const auto [b, nb, geom_rc] = block_geom(p->block_size, n_image, false);
    if (geom_rc != FSE_OK) return geom_rc;
    if (p->nstates > 2) return FSE_ERR_BAD_ARG;
    if (p->ckpt_interval && !ckpt_interval_ok(p->nstates == 1 ? 1u : 2u, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    *bs = b;
    *n_blocks = nb;
    return FSE_OK;
}

fsehip::EstBlocks est_args(const fsehip_frame_params* p, const uint32_t* counts, uint64_t n_image, uint32_t bs,
                           uint64_t n_blocks, uint64_t* total) {
    fsehip::EstBlocks E{};
    E.counts = counts;
    E.n_image = n_image;
    E.block_size = bs;
    E.n_blocks = (uint32_t)n_blocks;
    E.table_log = p->table_log;
    E.lmax = fsehip::est_kernel_class(p->table_log, p->max_table_log);
    E.ckpt_interval = p->ckpt_interval;
    E.nstates = p->nstates == 1 ? 1u : 2u;
    E.total = total;
    return E;
}

// fsehip_estimate_image_bytes, and the diff image, which has the delta image's size
uint64_t image_bytes(uint32_t kind, uint64_t n_elems, uint32_t w) {
    return fsehip_estimate_image_bytes(kind == FSEHIP_KIND_DIFF ? FSEHIP_KIND_DELTA : kind, n_elems, w);
}

// the counts of one kind's image: zeroed and added to, or the frame's own kernel
int image_counts(uint32_t kind, uint32_t w, const void* d_src, const void* d_base, uint64_t n_elems, uint64_t n_image,
                 uint32_t bs, uint64_t n_blocks, uint32_t* d_counts, fsehip_stream_t stream) {
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (kind == FSEHIP_KIND_FRAME)
        return rc_of(fsehip::launch_histogram(static_cast<const uint8_t*>(d_src), n_image, bs, (uint32_t)n_blocks,
                                              d_counts, nullptr, hs));
    if (hipMemsetAsync(d_counts, 0, 1024ull * n_blocks, hs) != hipSuccess) return FSE_ERR_HIP;
    if (kind == FSEHIP_KIND_DIFF) return fsehip::launch_diff_histogram(w, d_src, d_base, n_elems, bs, d_counts, stream);
    return fsehip::launch_image_histogram(w, kind == FSEHIP_KIND_DELTA, d_src, n_elems, bs, d_counts, stream);
}

// fsehip_estimate (n_est = 3: kinds 0..2) and fsehip_estimate_base (n_est = 5:
// the diff frame too, entry 3 always NONE); the caller has refused the bits
// its mask does not have
int estimate_kinds(const fsehip_frame_params* p, uint32_t kind_mask, uint32_t n_est, uint32_t elem_bytes,
                   const void* d_src, const void* d_base, uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_bytes,
                   uint64_t* d_est, fsehip_stream_t stream) {
    if (!p || !d_est || kind_mask == 0u) return FSE_ERR_BAD_ARG;
    if (!width_ok(elem_bytes)) return FSE_ERR_UNSUPPORTED;
    uint64_t n_image[5] = {}, n_blocks[5] = {}, fixed[5];
    uint32_t bs = 0;
    bool on[5];
    for (uint32_t k = 0; k < 5; ++k) {
        on[k] = k < n_est && k != FSEHIP_KIND_SEALED && (kind_mask >> k & 1u) && kind_takes(k, elem_bytes);
        fixed[k] = FSEHIP_EST_NONE;
        if (!on[k]) continue;
        n_image[k] = image_bytes(k, n_elems, elem_bytes);
        if (n_elems && !n_image[k]) return FSE_ERR_UNSUPPORTED;
        if (const int rc = frame_rules(p, n_image[k], &bs, &n_blocks[k])) return rc;
        fixed[k] = (k == FSEHIP_KIND_FRAME ? 32u : 48u) + 4u * n_blocks[k];
    }
    const uint64_t need = n_est == 3 ? fsehip_estimate_scratch_bytes(n_elems, elem_bytes, kind_mask, p->block_size)
                                     : fsehip_estimate_base_scratch_bytes(n_elems, elem_bytes, kind_mask, p->block_size);
    if (n_elems && (!d_src || (need && !d_scratch))) return FSE_ERR_BAD_ARG;
    if (!aligned(d_src, elem_bytes) || !aligned(d_scratch, 16) || !aligned(d_est, 8)) return FSE_ERR_BAD_ARG;
    // the base counts only where the diff frame is asked for and there is something to subtract
    if (on[FSEHIP_KIND_DIFF] && n_elems && (!d_base || !aligned(d_base, elem_bytes))) return FSE_ERR_BAD_ARG;
    if (scratch_bytes < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    if (const int rc = fsehip::launch_est_init(d_est, fixed, 3, stream)) return rc;
    if (n_est == 5)
        if (const int rc = fsehip::launch_est_init(d_est + 3, fixed + 3, 2, stream)) return rc;
    uint32_t* counts = reinterpret_cast<uint32_t*>(d_scratch);
    for (uint32_t k = 0; k < n_est; ++k) {
        if (!on[k] || n_blocks[k] == 0) continue;
        if (const int rc = image_counts(k, elem_bytes, d_src, d_base, n_elems, n_image[k], bs, n_blocks[k], counts, stream))
            return rc;
        const fsehip::EstBlocks E = est_args(p, counts, n_image[k], bs, n_blocks[k], d_est + k);
        if (const int rc = fsehip::launch_est_blocks(E, stream)) return rc;
    }
    return FSE_OK;
}

}  // namespace

extern "C" {

int fsehip_image_histogram(uint32_t kind, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                           uint32_t block_size, uint32_t* d_counts, fsehip_stream_t stream) {
    if (kind > FSEHIP_KIND_DELTA) return FSE_ERR_BAD_ARG;
    if (!width_ok(elem_bytes) || !kind_takes(kind, elem_bytes)) return FSE_ERR_UNSUPPORTED;
    if (n_elems == 0) return FSE_OK;
    const uint64_t n_image = fsehip_estimate_image_bytes(kind, n_elems, elem_bytes);
    if (!n_image) return FSE_ERR_UNSUPPORTED;
    if (!d_src || !d_counts || !aligned(d_src, elem_bytes) || !aligned(d_counts, 4)) return FSE_ERR_BAD_ARG;
    // no block limit here (a histogram counts no bits), as fsehip_histogram_blocks
    const uint32_t bs = block_size ? block_size : kDefaultBlock;
    const uint64_t n_blocks = (n_image + bs - 1) / bs;
    if ((n_blocks > 1 && (bs & 15u)) || n_blocks > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return image_counts(kind, elem_bytes, d_src, nullptr, n_elems, n_image, bs, n_blocks, d_counts, stream);
}

int fsehip_estimate_blocks(const fsehip_frame_params* p, const uint32_t* d_counts, uint64_t n_image_bytes,
                           uint8_t* d_type, uint32_t* d_rec, uint32_t* d_bits, uint8_t* d_log, uint64_t* d_total,
                           fsehip_stream_t stream) {
    if (!p || !d_total || (n_image_bytes && !d_counts)) return FSE_ERR_BAD_ARG;
    if (!aligned(d_counts, 4) || !aligned(d_rec, 4) || !aligned(d_bits, 4) || !aligned(d_total, 8))
        return FSE_ERR_BAD_ARG;
    uint32_t bs;
    uint64_t n_blocks;
    if (const int rc = frame_rules(p, n_image_bytes, &bs, &n_blocks)) return rc;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    const uint64_t fixed[3] = {32u + 4u * n_blocks, 0, 0};
    if (const int rc = fsehip::launch_est_init(d_total, fixed, 1, stream)) return rc;
    fsehip::EstBlocks E = est_args(p, d_counts, n_image_bytes, bs, n_blocks, d_total);
    E.type = d_type;
    E.rec = d_rec;
    E.bits = d_bits;
    E.log = d_log;
    return fsehip::launch_est_blocks(E, stream);
}

int fsehip_estimate(const fsehip_frame_params* p, uint32_t kind_mask, uint32_t elem_bytes, const void* d_src,
                    uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_bytes, uint64_t* d_est,
                    fsehip_stream_t stream) {
    if (kind_mask > 7u) return FSE_ERR_BAD_ARG;
    return estimate_kinds(p, kind_mask, 3, elem_bytes, d_src, nullptr, n_elems, d_scratch, scratch_bytes, d_est, stream);
}

int fsehip_diff_image_histogram(uint32_t elem_bytes, const void* d_src, const void* d_base, uint64_t n_elems,
                                uint32_t block_size, uint32_t* d_counts, fsehip_stream_t stream) {
    if (!width_ok(elem_bytes)) return FSE_ERR_UNSUPPORTED;
    if (n_elems == 0) return FSE_OK;
    const uint64_t n_image = image_bytes(FSEHIP_KIND_DIFF, n_elems, elem_bytes);
    if (!n_image) return FSE_ERR_UNSUPPORTED;
    if (!d_src || !d_base || !d_counts || !aligned(d_src, elem_bytes) || !aligned(d_base, elem_bytes) ||
        !aligned(d_counts, 4))
        return FSE_ERR_BAD_ARG;
    const uint32_t bs = block_size ? block_size : kDefaultBlock;
    const uint64_t n_blocks = (n_image + bs - 1) / bs;
    if ((n_blocks > 1 && (bs & 15u)) || n_blocks > 0xFFFFFFFFull) return FSE_ERR_BAD_ARG;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return image_counts(FSEHIP_KIND_DIFF, elem_bytes, d_src, d_base, n_elems, n_image, bs, n_blocks, d_counts, stream);
}

int fsehip_estimate_base(const fsehip_frame_params* p, uint32_t kind_mask, uint32_t elem_bytes, const void* d_src,
                         const void* d_base, uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_bytes,
                         uint64_t* d_est, fsehip_stream_t stream) {
    if (kind_mask & ~23u) return FSE_ERR_BAD_ARG;  // bits 0, 1, 2 and 4
    return estimate_kinds(p, kind_mask, 5, elem_bytes, d_src, d_base, n_elems, d_scratch, scratch_bytes, d_est, stream);
}

}  // extern "C"
