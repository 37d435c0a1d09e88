// fse_frame.cpp -- the frame's header, host side (fsehip.h section 2b).
//
// Plain C++ with no HIP include: the same source builds into libfsehip.so
// and, with g++ alone, into the sanitizer fuzz of tests/native/frame_fuzz.cpp.
// The device side (directory, records) is fse_frame.hip.
#include <string.h>

#include "../../include/fsehip.h"

namespace {

constexpr uint32_t kDefaultBlock = 65536;
constexpr uint32_t kMaxBlock = 1u << 28;
constexpr uint32_t kHeaderBytes = 32;

uint32_t get_u32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
void put_u32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// every header rule of the format; records_off is derived, not checked
bool fields_ok(const fsehip_frame_info& f) {
    if (f.version != 1u || f.nstates < 1u || f.nstates > 2u) return false;
    if (f.max_table_log < 11u || f.max_table_log > 15u) return false;
    if (f.flags & ~1u) return false;
    if (f.block_size == 0u || f.block_size > kMaxBlock) return false;
    if (f.reserved != 0u) return false;
    if (f.flags & 1u) {
        const uint32_t c = f.ckpt_interval;
        if (c < (f.nstates == 1u ? 16u : 8u) || (c & (c - 1u))) return false;
    } else if (f.ckpt_interval != 0u) {
        return false;
    }
    // ceil without overflow: n_total may be any u64
    const uint64_t nb = f.n_total / f.block_size + (f.n_total % f.block_size ? 1u : 0u);
    if (nb != (uint64_t)f.n_blocks) return false;
    if (f.n_blocks > 1u && (f.block_size & 15u)) return false;
    return true;
}

}  // namespace

extern "C" {

uint64_t fsehip_frame_bound(uint64_t n_total, uint32_t block_size) {
    const uint64_t bs = block_size ? block_size : kDefaultBlock;
    const uint64_t nb = n_total / bs + (n_total % bs ? 1u : 0u);
    return kHeaderBytes + 4u * nb + n_total;
}

int fsehip_frame_read_header(const uint8_t* hdr, size_t len, fsehip_frame_info* out) {
    if (!out || (!hdr && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (len < kHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (hdr[0] != 'F' || hdr[1] != 'S' || hdr[2] != 'E' || hdr[3] != 'F') return FSE_ERR_BAD_FRAME;
    fsehip_frame_info f;
    memset(&f, 0, sizeof(f));
    f.version = hdr[4];
    f.nstates = hdr[5];
    f.max_table_log = hdr[6];
    f.flags = hdr[7];
    f.block_size = get_u32(hdr + 8);
    f.ckpt_interval = get_u32(hdr + 12);
    f.n_total = (uint64_t)get_u32(hdr + 16) | ((uint64_t)get_u32(hdr + 20) << 32);
    f.n_blocks = get_u32(hdr + 24);
    f.reserved = get_u32(hdr + 28);
    if (!fields_ok(f)) return FSE_ERR_BAD_FRAME;
    f.records_off = kHeaderBytes + 4ull * f.n_blocks;
    *out = f;
    return FSE_OK;
}

int fsehip_frame_write_header(const fsehip_frame_info* info, uint8_t hdr[32]) {
    if (!info || !hdr || !fields_ok(*info)) return FSE_ERR_BAD_ARG;
    hdr[0] = 'F';
    hdr[1] = 'S';
    hdr[2] = 'E';
    hdr[3] = 'F';
    hdr[4] = (uint8_t)info->version;
    hdr[5] = (uint8_t)info->nstates;
    hdr[6] = (uint8_t)info->max_table_log;
    hdr[7] = (uint8_t)info->flags;
    put_u32(hdr + 8, info->block_size);
    put_u32(hdr + 12, info->ckpt_interval);
    put_u32(hdr + 16, (uint32_t)info->n_total);
    put_u32(hdr + 20, (uint32_t)(info->n_total >> 32));
    put_u32(hdr + 24, info->n_blocks);
    put_u32(hdr + 28, 0u);
    return FSE_OK;
}

}  // extern "C"
