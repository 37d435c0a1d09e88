// fse_crc_dev.hpp -- the device pieces the CRC kernels of the check record
// (fse_check.hip, fsehip.h section 2f) and of the member check record
// (fse_mcheck.hip, section 2l) share: a 16-byte word and a lane's state
// through the tables of fse_check_host.h held in LDS, and the mask of a first
// word's bytes that are not content.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsehip {

namespace {

// the four bytes of v through tables j0 .. j0 + 3
__device__ __forceinline__ uint32_t look4(const uint32_t* T, uint32_t v, uint32_t j0) {
    return T[j0 * 256 + (v & 0xFFu)] ^ T[(j0 + 1) * 256 + ((v >> 8) & 0xFFu)] ^
           T[(j0 + 2) * 256 + ((v >> 16) & 0xFFu)] ^ T[(j0 + 3) * 256 + (v >> 24)];
}
// the state a word leaves at its end, from state 0
__device__ __forceinline__ uint32_t word16(const uint32_t* T, const uint4& w) {
    return look4(T, w.x, 0) ^ look4(T, w.y, 4) ^ look4(T, w.z, 8) ^ look4(T, w.w, 12);
}
// a lane's state one stride on
__device__ __forceinline__ uint32_t carry(const uint32_t* T, uint32_t st) { return look4(T, st, 16); }

// dword d of a word whose first `lead` bytes are not content
__device__ __forceinline__ uint32_t mask_lead(uint32_t v, uint32_t lead, uint32_t d) {
    if (lead >= 4u * d + 4u) return 0u;
    if (lead > 4u * d) return v & (0xFFFFFFFFu << (8u * (lead - 4u * d)));
    return v;
}

}  // namespace

}  // namespace fsehip
