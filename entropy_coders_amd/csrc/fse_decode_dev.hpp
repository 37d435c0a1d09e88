// fse_decode_dev.hpp -- the device pieces more than one decoder family
// (fse_decode_seg.hip, fse_decode_tables.hip, fse_decode_serial.hip,
// fse_decode_single.hip) uses: the decode table entry as dtable_blocks_kernel
// writes it and every decoder reads it, and the backward bit reader over
// global memory (the segment decoder's windowed blocks and
// decode1_serial_kernel).  What one family alone uses stays in its file.
#pragma once
#include "fse_device.hpp"

namespace fsehip {

// ------------------------------------------------------------------------
// Decode table entry (fse.rs:260-265 DecodeTransform, repacked for the
// decode loop): nb | symbol << 8 | new_state << SH.  With SH = 18 (L <= 14)
// the high half is the LDS byte offset of the next state's base entry
// (4 * new_state), nb in bits 0-4 serves directly as a v_bfe width/offset
// operand, and the byte sum of two entries' low bytes is nb0 + nb1.  L = 15
// needs the 15-bit new_state at SH = 17 (global-window kernels only).
// ------------------------------------------------------------------------
template <int LMAX>
struct Dte {
    static constexpr uint32_t SH = LMAX > 14 ? 17u : 18u;
    __device__ static __forceinline__ uint32_t make(uint32_t nb, uint32_t sym, uint32_t ns) {
        return nb | (sym << 8) | (ns << SH);
    }
    __device__ static __forceinline__ uint32_t ns(uint32_t e) { return e >> SH; }
};
__device__ __forceinline__ uint32_t dte_nb(uint32_t e) { return e & 0xFFu; }
__device__ __forceinline__ uint32_t dte_sym(uint32_t e) { return (e >> 8) & 0xFFu; }

// ------------------------------------------------------------------------
// Backward bit reader over global memory (BitStackReader semantics,
// stack_reader.rs:17-215): `pos` = bits remaining above the block start,
// buf holds stream bits [base, base+64); refills pull the next lower word.
// ------------------------------------------------------------------------
struct WindowReader {
    const uint32_t* w;
    uint64_t buf;
    int32_t base;
    int32_t pos;
    __device__ __forceinline__ void init(const uint32_t* words, int32_t p) {
        w = words;
        pos = p;
        base = ((p + 31) & ~31) - 64;
        if (base < 0) base = 0;
        buf = (uint64_t)w[base >> 5] | ((uint64_t)w[(base >> 5) + 1] << 32);
    }
    __device__ __forceinline__ uint32_t pop(uint32_t nb) {
        pos -= (int32_t)nb;
        return (uint32_t)(buf >> (uint32_t)(pos - base)) & ((1u << nb) - 1u);
    }
    __device__ __forceinline__ void refill() {
        if (pos - base < 32 && base > 0) {
            base -= 32;
            buf = (buf << 32) | (uint64_t)w[base >> 5];
        }
    }
};

}  // namespace fsehip
