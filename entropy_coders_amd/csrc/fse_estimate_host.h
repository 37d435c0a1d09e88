// fse_estimate_host.h -- what the size estimate's translation units share
// (fsehip.h sections 2g and 2i): the integer cost model of fse_estimate.cpp, written
// once for the host and the device, and the launchers of fse_estimate.hip,
// called by fse_capi_estimate.cpp.  Plain C++ with no HIP include (a stream
// travels as void*), as fse_elem_host.h.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../include/fsehip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSE_EST_HD __host__ __device__ inline
#else
#define FSE_EST_HD inline
#endif

namespace fsehip {

// 256 * log2(c) for 1 <= c <= 32768, within 1.01 (exact at powers of two): the
// integer part, then eight squarings of the mantissa (31 fraction bits), each
// giving one more bit.  x stays below 2^32 before every squaring.
FSE_EST_HD uint32_t log2q8(uint32_t c) {
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(c);
    uint64_t x = (uint64_t)c << (31u - hb);
    uint32_t y = hb;
    for (int i = 0; i < 8; ++i) {
        x = (x * x) >> 31;
        y <<= 1;
        if (x >> 32) {
            x >>= 1;
            y |= 1u;
        }
    }
    return y;
}

// bits * 256 of one symbol of normalised count c at table log L (-1 costs L bits)
FSE_EST_HD uint32_t cost8(int32_t c, uint32_t L) { return 256u * L - log2q8(c < 1 ? 1u : (uint32_t)c); }

// fsehip_sidecar_per_block_ns
FSE_EST_HD uint32_t est_spb(uint32_t n, uint32_t ckpt_interval, uint32_t nstates) {
    if (ckpt_interval == 0u) return 0u;
    return nstates == 1u ? n / ckpt_interval + 2u : n / 2u / ckpt_interval + 2u;
}

// The rule from Q = sum of counts[s] * cost8(norm[s], L) on: the payload bits,
// and the record's bytes with its header and checkpoints.
FSE_EST_HD void est_record(uint64_t Q, uint32_t L, uint32_t hdr_bytes, uint32_t raw_len, uint32_t ckpt_interval,
                           uint32_t nstates, uint64_t* bits, uint64_t* rec) {
    *bits = ((Q + 255u) >> 8) + (uint64_t)nstates * L + 1u;
    *rec = hdr_bytes + ((*bits + 7u) >> 3) + 8ull * est_spb(raw_len, ckpt_interval, nstates);
}

// The encoder's kernel class for a frame's table_log and max_table_log (11..15).
uint32_t est_kernel_class(uint32_t table_log, uint32_t max_table_log);

// One fsehip_estimate_blocks launch.  counts: u32 x 256 per block of an image
// of n_image bytes in blocks of block_size; the per-block outputs may be
// null; every FSE/RAW/RLE record's bytes are added to *total (which the caller
// has set to the container's fixed bytes).  lmax: the kernel class, a table
// log above it is stored RAW as the encoder's UNSUPPORTED blocks are.
struct EstBlocks {
    const uint32_t* counts;
    uint64_t n_image;
    uint32_t block_size, n_blocks;
    uint32_t table_log, lmax, ckpt_interval, nstates;
    uint8_t* type;
    uint32_t* rec;
    uint32_t* bits;
    uint8_t* log;
    uint64_t* total;
};

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t.
// d[i] = v[i], i < n <= 3
int launch_est_init(uint64_t* d, const uint64_t v[3], uint32_t n, void* stream);
int launch_est_blocks(const EstBlocks& E, void* stream);
// the counts of the plane (delta = false; w 2, 4, 8) or delta (w 1, 2, 4, 8)
// image's blocks, added into `counts`, which the caller has zeroed
int launch_image_histogram(uint32_t w, bool delta, const void* src, uint64_t n_elems, uint32_t block_size,
                           uint32_t* counts, void* stream);
// the same of the diff image (w 1, 2, 4, 8) of src against base, which may overlap
int launch_diff_histogram(uint32_t w, const void* src, const void* base, uint64_t n_elems, uint32_t block_size,
                          uint32_t* counts, void* stream);

}  // namespace fsehip
