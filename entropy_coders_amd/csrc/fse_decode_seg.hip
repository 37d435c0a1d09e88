// fse_decode_seg.hip -- segment-parallel decode of a batch of blocks on
// prebuilt tables and the sidecar index, gfx950.
//
//   decode_pre_kernel  one workgroup of 256 or 512 threads per block, the
//                      compressed block and its table (fse_decode_tables.hip)
//                      staged in LDS by DMA, every lane decodes one sidecar
//                      segment (checkpoint to checkpoint) and checks its end
//                      against the next checkpoint; 2-state and 1-state
//
// PASS 1 takes the blocks its stage holds and defers the others to a list
// pass (2, or 3 and then 2) with a larger stage; a block above every stage,
// and every block at LMAX = 15 (the 128 KiB table leaves no LDS for the
// image: pass 0), reads its payload through a register window from global
// memory.  Up to L = 14 the image sits beside the table (32 and 64 KiB
// tables at 13 and 14: 2 and 1 workgroups per CU).  launch_decode_seg holds
// the stage sizes and the passes of each table log.
#include <algorithm>

#include "fse_decode_dev.hpp"
#include "fse_decode_host.h"

namespace fsehip {

// cache policy of the segment decoder's LDS-DMA staging loads: nt (2), as the image and table
// are read once (C3 0.96 -> 0.91-0.96 ms, C2 decode 0.558 -> 0.552-0.554 ms, same box)
constexpr int STAGE_AUX = 2;

// Output group: pairs per lane between stores (32 pairs = 64 B, one HBM
// burst).  Segment starts are multiples of ckpt_interval, so groups are 64 B
// aligned whenever ckpt_interval >= 32.
constexpr uint32_t DEC_GROUP = 32;

// Sidecar cross-check: a segment that is not the block's last must end
// exactly where the next checkpoint says the decoder is (bit position and
// both states, a = 4 * state); a mismatch means the index does not belong to
// this stream (corrupt, or built with another checkpoint interval).
__device__ __forceinline__ bool ckpt_match(uint64_t e, int32_t hdr_bits, uint32_t smask, int32_t pos, uint32_t a0,
                                           uint32_t a1) {
    return (int32_t)(uint32_t)e + hdr_bits == pos && ((((uint32_t)(e >> 32) & smask) << 2) == a0) &&
           ((((uint32_t)(e >> 48) & smask) << 2) == a1);
}

// Container-mode end of a 2-state block after its main loop (the oracle's
// decompress2_impl with the raw length; lib.rs:227-244): the last one or two
// symbols come from the final states, and a valid block has then read every
// payload bit.  `ent(s)` is the table entry of state s; the reader pops.
template <int LMAX, class Ent, class Pop>
__device__ __forceinline__ int32_t finish2(uint32_t o, uint32_t n, uint32_t& s0, uint32_t& s1, int32_t& pos,
                                           int32_t hdr_bits, uint8_t* __restrict__ out, Ent ent, Pop pop) {
    for (;;) {
        if (o + 2u == n) {
            out[o++] = (uint8_t)dte_sym(ent(s0));
            out[o++] = (uint8_t)dte_sym(ent(s1));
            break;
        }
        if (o + 1u == n) {
            out[o++] = (uint8_t)dte_sym(ent(s0));
            break;
        }
        const uint32_t e0 = ent(s0);
        uint32_t nb = dte_nb(e0);
        if (pos - (int32_t)nb < hdr_bits) {
            out[o++] = (uint8_t)dte_sym(e0);
            if (o < n) out[o++] = (uint8_t)dte_sym(ent(s1));
            break;
        }
        s0 = Dte<LMAX>::ns(e0) + pop(nb);
        out[o++] = (uint8_t)dte_sym(e0);
        const uint32_t e1 = ent(s1);
        nb = dte_nb(e1);
        if (pos - (int32_t)nb < hdr_bits) {
            out[o++] = (uint8_t)dte_sym(e1);
            if (o < n) out[o++] = (uint8_t)dte_sym(ent(s0));
            break;
        }
        s1 = Dte<LMAX>::ns(e1) + pop(nb);
        out[o++] = (uint8_t)dte_sym(e1);
    }
    return o != n ? FSE_ERR_LENGTH_MISMATCH : pos == hdr_bits ? FSE_OK : FSE_ERR_BAD_SIDECAR;
}

// Main-loop pairs [p0, p1) of one segment read through a global-memory
// window (blocks the LDS stage cannot hold, and every block at LMAX = 15);
// the sidecar guarantees the bits, so no read checks.  `dt` may be LDS.
template <int LMAX>
__device__ __forceinline__ int32_t decode_segment(WindowReader& br, uint32_t& s0, uint32_t& s1, uint32_t p0,
                                                  uint32_t p1, bool last, uint32_t n, uint32_t Pm,
                                                  uint8_t* __restrict__ out, const uint32_t* dt, int32_t hdr_bits) {
    uint32_t p = p0;
    for (; p + 8u <= p1; p += 8u) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t e0 = dt[s0], e1 = dt[s1];
            const uint32_t v0 = br.pop(dte_nb(e0));
            const uint32_t v1 = br.pop(dte_nb(e1));
            s0 = Dte<LMAX>::ns(e0) + v0;
            s1 = Dte<LMAX>::ns(e1) + v1;
            const uint32_t pr = __builtin_amdgcn_perm(e1, e0, 0x0c0c0501u);
            if (j & 1) w[j >> 1] |= pr << 16; else w[j >> 1] = pr;
            br.refill();
        }
        *reinterpret_cast<uint4*>(out + 2u * p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (; p < p1; ++p) {
        const uint32_t e0 = dt[s0], e1 = dt[s1];
        const uint32_t v0 = br.pop(dte_nb(e0));
        const uint32_t v1 = br.pop(dte_nb(e1));
        s0 = Dte<LMAX>::ns(e0) + v0;
        s1 = Dte<LMAX>::ns(e1) + v1;
        out[2u * p] = (uint8_t)dte_sym(e0);
        out[2u * p + 1u] = (uint8_t)dte_sym(e1);
        br.refill();
    }
    if (!last) return FSE_OK;
    return finish2<LMAX>(2u * Pm, n, s0, s1, br.pos, hdr_bits, out, [&](uint32_t s) { return dt[s]; },
                         [&](uint32_t nb) {
                             const uint32_t v = br.pop(nb);
                             br.refill();
                             return v;
                         });
}

// 1-state segment (fse_decompress, lib.rs:187-211) through the window.
template <int LMAX>
__device__ __forceinline__ int32_t decode_segment1(WindowReader& br, uint32_t& s, uint32_t p, uint32_t p1, bool last,
                                                   uint32_t n, uint8_t* __restrict__ out, const uint32_t* dt,
                                                   int32_t hdr_bits) {
    for (; p < p1; ++p) {
        const uint32_t e = dt[s];
        s = Dte<LMAX>::ns(e) + br.pop(dte_nb(e));
        br.refill();
        out[p] = (uint8_t)dte_sym(e);
    }
    if (!last) return FSE_OK;
    out[n - 1u] = (uint8_t)dte_sym(dt[s]);  // Decoder::finish (lib.rs:208)
    return br.pos == hdr_bits ? FSE_OK : FSE_ERR_BAD_SIDECAR;
}

// ------------------------------------------------------------------------
// Segment decode of a block staged in LDS (L <= 14, SH = 18).  One LdsChain
// is one segment's decoder pair: two tANS states as LDS byte offsets
// a0/a1 (4 * state) and the shared bit position.  Per pair the lane reads
// both table entries and ONE payload dword, all three issued together:
// a pair consumes <= 2L <= 28 < 32 bits, so the window base
// lo = (pos - 28) & ~31 (pos - lo in [28, 59]: the pair's bits and the
// 64-bit window both fit) moves down by at most one word per pair and the
// window's upper word is one of the previous pair's two words.  (It was
// pos - 24 while only L <= 12 ran here: at L = 13 and 14 a pair of rare
// symbols takes 26 or 28 bits and then read below the window; the wide
// randomized sweep found one.)  Then pos -= nb0 + nb1 (byte sum of
// the entries), v1 = the low nb1 bits at pos, v0 = the nb0 bits above
// (stack order: decoder 0 pops first), and the next offsets.  ~13 VALU and
// 3 LDS reads per pair, no branch.  The image has a 16-byte pad below it,
// so the window may start at word -1.
// ------------------------------------------------------------------------
constexpr int32_t PAIR_MAX_BITS = 28;  // 2 x 14: the largest pair at the LDS-staged table logs
struct LdsChain {
    static constexpr bool SINGLE_STEP = false;  // segments are whole pairs
    int32_t pos, B;
    uint32_t whi, wlo, a0, a1;
    __device__ __forceinline__ void init(const uint32_t* pay, int32_t p, uint32_t s0, uint32_t s1) {
        pos = p;
        a0 = s0 << 2;
        a1 = s1 << 2;
        // the first pair reads word lo/32 and takes word lo/32 + 1 from here
        B = (p - PAIR_MAX_BITS) & ~31;
        wlo = 0;
        whi = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(pay) + (B >> 3) + 4);
    }
    __device__ __forceinline__ uint32_t pair(const uint32_t* pay, const uint8_t* dtb) {
        const int32_t lo = (pos - PAIR_MAX_BITS) & ~31;
        const uint32_t w0 = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(pay) + (lo >> 3));
        const uint32_t e0 = *reinterpret_cast<const uint32_t*>(dtb + a0);
        const uint32_t e1 = *reinterpret_cast<const uint32_t*>(dtb + a1);
        const uint32_t w1 = lo == B ? whi : wlo;
        pos -= (int32_t)((e0 + e1) & 0xFFu);
        const uint32_t x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (uint32_t)(pos - lo));
        B = lo;
        whi = w1;
        wlo = w0;
        const uint32_t v1 = __builtin_amdgcn_ubfe(x, 0u, e1);
        const uint32_t v0 = __builtin_amdgcn_ubfe(x, e1, e0);
        a0 = (e0 >> 16) + (v0 << 2);
        a1 = (e1 >> 16) + (v1 << 2);
        return __builtin_amdgcn_perm(e1, e0, 0x0c0c0501u);  // sym0 | sym1 << 8
    }
    __device__ __forceinline__ uint32_t s0() const { return a0 >> 2; }
    __device__ __forceinline__ uint32_t s1() const { return a1 >> 2; }
    // decode-table entry of state s (Dte layout)
    __device__ static __forceinline__ uint32_t entry(const uint8_t* dtb, uint32_t s) {
        return *reinterpret_cast<const uint32_t*>(dtb + 4u * s);
    }
};
// Two pairs -> four output bytes (lo.b0 lo.b1 hi.b0 hi.b1).
template <class Chain, class Tab>
__device__ __forceinline__ uint32_t two_pairs(Chain& c, const uint32_t* pay, const Tab& dtb) {
    const uint32_t lo = c.pair(pay, dtb);
    const uint32_t hi = c.pair(pay, dtb);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);  // lo.b0 lo.b1 hi.b0 hi.b1
}
// Bits [pos, pos + 32) of an LDS-staged block (pos >= 0): one ds_read2 of
// the two words holding them and a v_alignbit (the end-of-block steps).
__device__ __forceinline__ uint32_t lds_bits32(const uint32_t* pay, int32_t pos) {
    const uint32_t* wp = pay + ((uint32_t)pos >> 5);
    return __builtin_amdgcn_alignbit(wp[1], wp[0], (uint32_t)pos);
}

// 32 pairs = one whole 64-byte piece of output per lane, stored back to
// back (full HBM write bursts instead of masked partial ones).
__device__ __forceinline__ void store_group(uint8_t* __restrict__ dst, const uint32_t* w) {
    uint4* o4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (uint32_t q = 0; q < DEC_GROUP / 8u; ++q) o4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// Output pieces through the wave's rows.  Lane (row r, column i) = lane
// 16r + i holds a 64-byte piece = chunks C[0..3] of 16 bytes (w[4c..4c+3]).
// A 4x4 transpose of (row, chunk) per column -- permlane32_swap on chunk
// pairs (0,2), (1,3), then permlane16_swap on (0,1), (2,3) -- leaves in lane
// (r, i), slot k, chunk r of lane (k, i)'s piece.  Store k then writes 16
// whole pieces (4 lanes x 16 contiguous bytes each) instead of 64 lanes'
// separate 16-byte pieces of 64 lines: 16 VALU per 32 pairs.
__device__ __forceinline__ void rows_transpose(uint32_t* w) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const auto r = __builtin_amdgcn_permlane32_swap(w[4 * c + d], w[4 * (c + 2) + d], false, false);
            w[4 * c + d] = r[0];
            w[4 * (c + 2) + d] = r[1];
        }
#pragma unroll
    for (int c = 0; c < 4; c += 2)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const auto r = __builtin_amdgcn_permlane16_swap(w[4 * c + d], w[4 * (c + 1) + d], false, false);
            w[4 * c + d] = r[0];
            w[4 * (c + 1) + d] = r[1];
        }
}

// The first `nb` bytes (1..16) of a 16-byte chunk t[] from the lane's own
// registers: one 16-byte store, or dword stores and byte stores for the last
// 1..3.  No byte at or past dst + nb is touched (the next block's bytes
// belong to another workgroup).  dst is 16-byte aligned.
__device__ __forceinline__ void store_chunk(uint8_t* __restrict__ dst, const uint32_t* t, uint32_t nb) {
    if (nb >= 16u) {
        __builtin_nontemporal_store(u32x4{t[0], t[1], t[2], t[3]}, reinterpret_cast<u32x4*>(dst));
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (nb >= 4u * i + 4u) {
            *reinterpret_cast<uint32_t*>(dst + 4u * i) = t[i];
        } else if (nb > 4u * i) {
            dst[4u * i] = (uint8_t)t[i];
            if (nb > 4u * i + 1u) dst[4u * i + 1u] = (uint8_t)(t[i] >> 8);
            if (nb > 4u * i + 2u) dst[4u * i + 2u] = (uint8_t)(t[i] >> 16);
        }
    }
}

// Output groups of one chain per lane, wave-synchronous (every lane of the
// wave runs ng_max iterations), stored through rows_transpose: obase[k] /
// ong[k] are the offset in `out` and the whole-group count of the piece of
// lane (k, column) -- the owner of this lane's slot k; own_off is the lane's
// own.  A lane decodes its my_ng whole groups and then, in iteration my_ng,
// the `tail` bytes its segment has beyond them (0..63: the block's last
// segment, or every segment when checkpoints are closer than a group) while
// the wave's other lanes decode a whole group: at C2 the last segment's lane
// does its 31 pairs beside its wave's second group (before, it ran them
// alone, pair by pair, after the groups, with the other seven waves waiting
// at the final barrier).  An iteration with such a lane (a wave-uniform
// test) goes 16 bytes at a time in a rolled loop, every pair predicated on
// the lane's count, so no pair past a segment's end is decoded and the
// chain ends in the state after the segment's last pair.  A lane with a
// tail stores each chunk itself from its own registers (store_chunk); the
// whole pieces of the wave's other lanes are collected chunk by chunk and
// go through the transpose like every other iteration's.  (Unrolled over
// the 32 pairs the predicated iteration took 84 VGPRs against 64, 2
// workgroups per CU instead of 3; rolled it takes 79.  Storing the whole
// pieces of that iteration as four separate 16-byte chunks per lane instead
// measured C2 decode 0.50 -> 0.70 ms: a sixteenth of the output in partial
// non-temporal writes.  profiles/lane_serial/.)
template <class Chain, class Tab>
__device__ __forceinline__ void run_groups_tx(Chain& c, uint32_t my_ng, uint32_t tail, uint32_t ng_max,
                                              const uint32_t* pay, const Tab& dtb, uint8_t* __restrict__ out,
                                              const uint32_t* obase, const uint32_t* ong, uint32_t row,
                                              uint32_t own_off) {
    for (uint32_t g = 0; g < ng_max; ++g) {
        uint32_t w[DEC_GROUP / 2u];
        const bool part = g == my_ng && tail != 0u;
        if (__ballot(part) != 0ull) {
            // bytes of this iteration's piece: the chain's pair() makes two,
            // a 1-state segment may end on a single step
            const uint32_t nb = g < my_ng ? 2u * DEC_GROUP : part ? tail : 0u;
#pragma unroll
            for (uint32_t j = 0; j < DEC_GROUP / 2u; ++j) w[j] = 0;
#pragma unroll 1
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t lim = nb > 16u * q ? nb - 16u * q : 0u;  // bytes from this chunk on
                const uint32_t cnt = lim >> 1;
                uint32_t t[4];
#pragma unroll
                for (uint32_t j = 0; j < 8u; j += 2u) {
                    uint32_t x = 0;
                    if (j < cnt) x = c.pair(pay, dtb);
                    if (j + 1u < cnt) x = __builtin_amdgcn_perm(c.pair(pay, dtb), x, 0x05040100u);
                    if constexpr (Chain::SINGLE_STEP) {
                        if ((lim & 1u) && j == cnt) x = c.step_sym(pay, dtb);
                        if ((lim & 1u) && j + 1u == cnt) x |= c.step_sym(pay, dtb) << 16;
                    }
                    t[j >> 1] = x;
                }
                if (part && lim) store_chunk(out + (own_off + g * 2u * DEC_GROUP + 16u * q), t, lim);
                // the chunk enters the piece from the top: after the four
                // trips chunk q sits in w[4q .. 4q + 3]
#pragma unroll
                for (uint32_t i = 0; i < DEC_GROUP / 2u - 4u; ++i) w[i] = w[i + 4u];
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) w[DEC_GROUP / 2u - 4u + i] = t[i];
            }
        } else if (g < my_ng) {
#pragma unroll
            for (uint32_t j = 0; j < DEC_GROUP; j += 2u) w[j >> 1] = two_pairs(c, pay, dtb);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < DEC_GROUP / 2u; ++j) w[j] = 0;
        }
        rows_transpose(w);
        // non-temporal: the output is written once and not read back here, so
        // it should not displace the images, tables and sidecars in L2
        // (C3 0.95 -> 0.91 ms, C2 decode 0.60 -> 0.57 ms, same box)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (g < ong[k])  // (a 32-bit offset from the block's scalar base)
                __builtin_nontemporal_store(
                    u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]},
                    reinterpret_cast<u32x4*>(out + (obase[k] + g * 2u * DEC_GROUP + 16u * row)));
    }
}

// `ng` whole output groups of two independent chains, their pairs
// interleaved (one lane, two segments: while one chain waits on its LDS
// reads the other's arithmetic issues).
template <class Chain, class Tab>
__device__ __forceinline__ void run_chains2(Chain& a, Chain& b, const uint32_t* pay, const Tab& dtb, uint32_t pa,
                                            uint32_t pb, uint32_t ng, uint8_t* __restrict__ out) {
    for (uint32_t g = 0; g < ng; ++g) {
        uint32_t wa[DEC_GROUP / 2u], wb[DEC_GROUP / 2u];
#pragma unroll
        for (uint32_t j = 0; j < DEC_GROUP; j += 2u) {
            const uint32_t la = a.pair(pay, dtb);
            const uint32_t lb = b.pair(pay, dtb);
            const uint32_t ha = a.pair(pay, dtb);
            const uint32_t hb = b.pair(pay, dtb);
            wa[j >> 1] = __builtin_amdgcn_perm(ha, la, 0x05040100u);
            wb[j >> 1] = __builtin_amdgcn_perm(hb, lb, 0x05040100u);
        }
        store_group(out + 2u * (pa + g * DEC_GROUP), wa);
        store_group(out + 2u * (pb + g * DEC_GROUP), wb);
    }
}

// Pairs [p, p1) of one chain, then (when `last`) the container-mode end.
template <class Chain, class Tab>
__device__ __forceinline__ int32_t run_chain(Chain& c, const uint32_t* pay, const Tab& dtb, uint32_t p, uint32_t p1,
                                             bool last, uint32_t n, uint32_t Pm, uint8_t* __restrict__ out,
                                             int32_t hdr_bits) {
    for (; p + DEC_GROUP <= p1; p += DEC_GROUP) {
        uint32_t w[DEC_GROUP / 2u];
#pragma unroll
        for (uint32_t j = 0; j < DEC_GROUP; j += 2u) w[j >> 1] = two_pairs(c, pay, dtb);
        store_group(out + 2u * p, w);
    }
    for (; p < p1; ++p) {
        const uint32_t pr = c.pair(pay, dtb);
        out[2u * p] = (uint8_t)pr;
        out[2u * p + 1u] = (uint8_t)(pr >> 8);
    }
    if (!last) return FSE_OK;
    // states as indices for the shared end; the chain keeps byte offsets
    uint32_t s0 = c.s0(), s1 = c.s1();
    return finish2<11>(2u * Pm, n, s0, s1, c.pos, hdr_bits, out, [&](uint32_t s) { return Chain::entry(dtb, s); },
                       [&](uint32_t nb) {
                           c.pos -= (int32_t)nb;
                           return __builtin_amdgcn_ubfe(lds_bits32(pay, c.pos), 0u, nb);
                       });
}

// 1-state chain (fse_decompress blocks) without a refill branch (round 6;
// the register window it replaced refilled under a divergent branch every
// few symbols and needed 110 VGPRs, 2 workgroups per CU at 512 threads:
// C2 1-state decode 0.75-0.78 -> 0.57 ms per GiB, profiles/r06/w1/): each call
// cuts x = the 32 bits just below pos from the word pair around pos - 32
// (word pos / 32 carried from the previous call, the word below it read:
// one ds_read, a compare, a select and a v_alignbit), then takes one symbol's
// field (step) or two symbols' fields (pair: <= 2 x 14 bits) from the top
// of x.  The image has 16 pad bytes below it (the word below word 0).
struct LdsChain1 {
    int32_t pos;
    uint32_t Q, whi, wlo, a;
    __device__ __forceinline__ void init(const uint32_t* pay, int32_t p, uint32_t s) {
        pos = p;
        a = s << 2;
        Q = ((uint32_t)p >> 3) & ~3u;
        wlo = 0;
        whi = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(pay) + Q);
    }
    __device__ __forceinline__ uint32_t window(const uint32_t* pay) {
        const uint32_t q = ((uint32_t)pos >> 3) & ~3u;
        const uint32_t wq = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(pay) + q - 4u);
        const uint32_t hi = q == Q ? whi : wlo;
        Q = q;
        whi = hi;
        wlo = wq;
        return __builtin_amdgcn_alignbit(hi, wq, (uint32_t)pos);
    }
    // one symbol; returns the table entry (symbol in bits 8-15)
    __device__ __forceinline__ uint32_t step(const uint32_t* pay, const uint8_t* dtb) {
        const uint32_t e = *reinterpret_cast<const uint32_t*>(dtb + a);
        const uint32_t x = window(pay);
        pos -= (int32_t)(e & 0xFFu);
        a = (e >> 16) + (__builtin_amdgcn_ubfe(x, 0u - e, e) << 2);
        return e;
    }
    // two symbols from one window; returns sym0 | sym1 << 8
    __device__ __forceinline__ uint32_t pair(const uint32_t* pay, const uint8_t* dtb) {
        const uint32_t e0 = *reinterpret_cast<const uint32_t*>(dtb + a);
        const uint32_t x = window(pay);
        const uint32_t o0 = 0u - e0;  // low 5 bits: 32 - nb0
        const uint32_t a1 = (e0 >> 16) + (__builtin_amdgcn_ubfe(x, o0, e0) << 2);
        const uint32_t e1 = *reinterpret_cast<const uint32_t*>(dtb + a1);
        a = (e1 >> 16) + (__builtin_amdgcn_ubfe(x, o0 - e1, e1) << 2);
        pos -= (int32_t)((e0 + e1) & 0xFFu);
        return __builtin_amdgcn_perm(e1, e0, 0x0c0c0501u);
    }
};
struct Chain1x2 {
    static constexpr bool SINGLE_STEP = true;  // a segment may hold an odd count of symbols
    LdsChain1 c;
    __device__ __forceinline__ uint32_t pair(const uint32_t* pay, const uint8_t* dtb) { return c.pair(pay, dtb); }
    __device__ __forceinline__ uint32_t step_sym(const uint32_t* pay, const uint8_t* dtb) {
        return dte_sym(c.step(pay, dtb));
    }
};

// Steps [p, p1) of one 1-state segment; the last segment then emits the
// final state's symbol (container mode: the raw length ends the block, as
// the reference's next read fails right there for a valid stream).
__device__ __forceinline__ int32_t run_chain1(LdsChain1& c, const uint32_t* pay, const uint8_t* dtb, uint32_t p,
                                              uint32_t p1, bool last, uint32_t n, uint8_t* __restrict__ out,
                                              int32_t hdr_bits) {
    constexpr uint32_t G = 2u * DEC_GROUP;  // 64 symbols = one 64-byte piece of output
    for (; p + G <= p1; p += G) {
        uint32_t w[G / 4u];
#pragma unroll
        for (uint32_t j = 0; j < G; j += 4u) {
            const uint32_t lo = c.pair(pay, dtb), hi = c.pair(pay, dtb);
            w[j >> 2] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
        uint4* o4 = reinterpret_cast<uint4*>(out + p);
#pragma unroll
        for (uint32_t q = 0; q < G / 16u; ++q) o4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    for (; p < p1; ++p) out[p] = (uint8_t)dte_sym(c.step(pay, dtb));
    if (!last) return FSE_OK;
    out[n - 1u] = (uint8_t)dte_sym(*reinterpret_cast<const uint32_t*>(dtb + c.a));  // finish (lib.rs:208)
    return c.pos == hdr_bits ? FSE_OK : FSE_ERR_BAD_SIDECAR;
}

// ------------------------------------------------------------------------
// Segment-parallel decode with prebuilt tables (fsehip_decompress_blocks_dt,
// the second kernel of fsehip_decompress_blocks; C3 times it alone).  One
// 256-thread workgroup per block:
//   1. DMA (global_load_lds) the compressed block and its table into LDS;
//   2. lane t decodes sidecar segment 33t mod 256 of each round (lanes that
//      walk their segments in lockstep then read payload words ~33 segments
//      apart, spread over the banks, instead of ~1 segment apart), storing
//      32 pairs (64 B) at a time;
//   3. every segment's end is checked against the next checkpoint.
// Blocks above the PMAX-byte stage are deferred (pass 1: status
// FSE_DEFERRED) to a second launch with a 66 KiB stage (pass 2); at
// LMAX = 15 the table alone fills the LDS and every block reads its payload
// through a global-memory window (pass 0).
// ------------------------------------------------------------------------
// Segment of thread tid in a round of 256.
template <uint32_t NT = 256u>
__device__ __forceinline__ uint32_t seg_of(uint32_t tid) {
    return (tid * 33u) & (NT - 1u);  // a bijection of [0, NT): 33 is odd
}

template <int LMAX, uint32_t PMAX, uint32_t NW = 4u>
struct PreSmem {
    uint32_t pad[4];  // below the image: the window may start at word -1
    uint32_t pay[PMAX / 4];
    uint32_t dt[1u << LMAX];
    int err[NW];
};

// One block (gb) by the whole workgroup; LDS reuse across calls is safe:
// every reader of the image and table has passed the final barrier before
// the next call's staging writes them.
template <int LMAX, uint32_t PMAX, int NS, uint32_t NT, class Smem>
__device__ __forceinline__ void decode_pre_block(const DecParams& P, Smem& sm, const uint64_t gb) {
    constexpr bool BIG = LMAX > 14;  // no LDS image
    constexpr uint32_t NW = NT / 64u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (gb >= P.n_blocks) return;
    const uint8_t* in = P.in + gb * P.slot_bytes;
    const uint32_t clen = P.comp_len[gb];
    const uint64_t ooff = gb * (uint64_t)P.block_size;
    const uint32_t n = (uint32_t)min((uint64_t)P.block_size, P.n_total - ooff);
    uint8_t* out = P.out + ooff;
    const int32_t info = P.dtinfo[gb];
    const bool in_lds = !BIG && clen <= PMAX;
    if (P.pass >= 2 && P.status[gb] != FSE_DEFERRED) return;  // done by an earlier pass
    FSE_STAMP(P, 0);
    if (info < 0 || n < (NS == 2 ? 2u : 1u)) {
        if (tid == 0) P.status[gb] = info < 0 ? info : FSE_ERR_LENGTH_MISMATCH;
        return;
    }
    // too big for this stage: a later list pass decodes it (pass 3: a list
    // pass that defers its own oversized blocks again)
    if ((P.pass == 1 || P.pass == 3) && !in_lds) {
        if (tid == 0) P.status[gb] = FSE_DEFERRED;
        return;
    }
    const int32_t hdr_bits = (info & 0xFFFF) * 8;
    const uint32_t L = (uint32_t)info >> 16;
    {  // stage the block image and the table
        if (in_lds) {
            const uint32_t nvec = (clen + 15u) >> 4;
            const uint4* src4 = reinterpret_cast<const uint4*>(in);
            uint4* dst4 = reinterpret_cast<uint4*>(sm.pay);
            for (uint32_t i = wv * 64u; i < nvec; i += NT)
                if (i + lane < nvec) __builtin_amdgcn_global_load_lds(src4 + i + lane, dst4 + i, 16, 0, STAGE_AUX);
        }
        {
            const uint32_t dvec = 1u << L >> 2;  // 4 << L bytes
            const uint4* t4 = reinterpret_cast<const uint4*>(P.dt + gb * (uint64_t)(1u << LMAX));
            uint4* d4 = reinterpret_cast<uint4*>(sm.dt);
            for (uint32_t i = wv * 64u; i < dvec; i += NT)
                if (i + lane < dvec) __builtin_amdgcn_global_load_lds(t4 + i + lane, d4 + i, 16, 0, STAGE_AUX);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    FSE_STAMP(P, 3);
    const uint32_t smask = (1u << L) - 1u;
    // main-loop steps: pairs (NS = 2) or symbols below the last one (NS = 1)
    const uint32_t Pm = NS == 2 ? ((n & 1u) ? (n - 3u) / 2u : n / 2u - 1u) : n - 1u;
    const uint32_t I = P.ckpt_interval;
    const uint32_t nseg = Pm / I + 1u;
    const uint64_t* sc = P.sidecar + gb * P.ckpt_per_block;
    const uint32_t maxbp = clen * 8u - (uint32_t)hdr_bits;
    using Chain = LdsChain;
    const uint8_t* dtb = reinterpret_cast<const uint8_t*>(sm.dt);
    const uint32_t* gw = reinterpret_cast<const uint32_t*>(in);
    int32_t err = FSE_OK;
    uint32_t base0 = 0;
    if (NS == 2 && !BIG && in_lds && NT <= 256u) {  // (512 lanes: one segment each per round, 64 VGPRs)
        // Two segments per lane while a round has more segments than lanes
        // (checkpoints every <= 64 pairs at 64 KiB): segments s and s + NT
        // decoded interleaved, two independent chains per lane.
        for (; base0 + NT < nseg; base0 += 2u * NT) {
            const uint32_t sa = base0 + seg_of<NT>(tid), sb = sa + NT;
            bool act[2] = {sa < nseg, sb < nseg};
            const uint32_t sg[2] = {sa, sb};
            Chain c[2];
            uint32_t pp[2], pe[2];
            uint64_t en[2];
            int32_t r[2] = {FSE_OK, FSE_OK};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pp[k] = sg[k] * I;
                pe[k] = min(pp[k] + I, Pm);
                en[k] = 0;
                if (!act[k]) continue;
                const uint64_t e = sc[sg[k]];
                en[k] = sg[k] == nseg - 1u ? 0ull : sc[sg[k] + 1u];
                if ((uint32_t)e > maxbp) {  // corrupt index: never read outside the block
                    r[k] = FSE_ERR_BAD_SIDECAR;
                    act[k] = false;
                    continue;
                }
                c[k].init(sm.pay, hdr_bits + (int32_t)(uint32_t)e, (uint32_t)(e >> 32) & smask,
                          (uint32_t)(e >> 48) & smask);
            }
            const uint32_t ng = (act[0] && act[1]) ? min(pe[0] - pp[0], pe[1] - pp[1]) / DEC_GROUP : 0u;
            run_chains2(c[0], c[1], sm.pay, dtb, pp[0], pp[1], ng, out);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!act[k]) continue;
                const bool last = sg[k] == nseg - 1u;
                r[k] = run_chain(c[k], sm.pay, dtb, pp[k] + ng * DEC_GROUP, pe[k], last, n, Pm, out, hdr_bits);
                if (r[k] == FSE_OK && !last &&
                    !ckpt_match(en[k], hdr_bits, smask, c[k].pos, c[k].s0() << 2, c[k].s1() << 2))
                    r[k] = FSE_ERR_BAD_SIDECAR;
            }
            if (r[0] != FSE_OK) err = r[0];
            if (r[1] != FSE_OK) err = r[1];
        }
    }
    if (NS == 2 && !BIG && in_lds) {
        // One segment per lane, every lane of a wave in step, output pieces
        // stored through the row transpose (run_groups_tx), a segment's pairs
        // beyond its whole groups included; then, for the last segment, the
        // block's end.
        for (; base0 < nseg; base0 += NT) {
            const uint32_t seg = base0 + seg_of<NT>(tid);
            bool act = seg < nseg;
            const uint32_t p0 = seg * I, p1 = act ? min(p0 + I, Pm) : p0;
            const bool lastseg = seg == nseg - 1u;
            int32_t r = FSE_OK;
            Chain c;
            uint64_t en = 0;
            if (act) {
                const uint64_t e = sc[seg];
                en = lastseg ? 0ull : sc[seg + 1u];
                if ((uint32_t)e > maxbp) {  // corrupt index: never read outside the block
                    r = FSE_ERR_BAD_SIDECAR;
                    act = false;
                } else {
                    c.init(sm.pay, hdr_bits + (int32_t)(uint32_t)e, (uint32_t)(e >> 32) & smask,
                           (uint32_t)(e >> 48) & smask);
                }
            }
            const uint32_t my_ng = act ? (p1 - p0) / DEC_GROUP : 0u;
            const uint32_t tail = act ? 2u * ((p1 - p0) % DEC_GROUP) : 0u;  // bytes beyond the whole groups
            const uint32_t ng_max = wave_max(my_ng + (tail ? 1u : 0u));
            if (ng_max) {
                uint32_t obase[4];
                uint32_t ong[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t os = base0 + seg_of<NT>((tid & ~63u) + 16u * k + (tid & 15u));
                    const uint32_t oq = os * I;
                    ong[k] = os < nseg ? (min(oq + I, Pm) - oq) / DEC_GROUP : 0u;
                    obase[k] = 2u * oq;
                }
                run_groups_tx(c, my_ng, tail, ng_max, sm.pay, dtb, out, obase, ong, (tid >> 4) & 3u, 2u * p0);
            }
            if (act) {  // every pair is decoded: only the block's end is left, for the last segment
                r = run_chain(c, sm.pay, dtb, p1, p1, lastseg, n, Pm, out, hdr_bits);
                if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, c.pos, c.s0() << 2, c.s1() << 2))
                    r = FSE_ERR_BAD_SIDECAR;
            }
            if (r != FSE_OK) err = r;
        }
    }
    if (NS == 1 && !BIG && in_lds) {
        // 1-state: the same transposed stores, 64 symbols (one 64-byte piece)
        // per group, two chain steps per packed pair
        constexpr uint32_t G1 = 2u * DEC_GROUP;
        for (; base0 < nseg; base0 += NT) {
            const uint32_t seg = base0 + seg_of<NT>(tid);
            bool act = seg < nseg;
            const uint32_t p0 = seg * I, p1 = act ? min(p0 + I, Pm) : p0;
            const bool lastseg = seg == nseg - 1u;
            int32_t r = FSE_OK;
            Chain1x2 c;
            uint64_t en = 0;
            if (act) {
                const uint64_t e = sc[seg];
                en = lastseg ? 0ull : sc[seg + 1u];
                if ((uint32_t)e > maxbp) {  // corrupt index: never read outside the block
                    r = FSE_ERR_BAD_SIDECAR;
                    act = false;
                } else {
                    c.c.init(sm.pay, hdr_bits + (int32_t)(uint32_t)e, (uint32_t)(e >> 32) & smask);
                }
            }
            const uint32_t my_ng = act ? (p1 - p0) / G1 : 0u;
            const uint32_t tail = act ? (p1 - p0) % G1 : 0u;  // symbols = bytes beyond the whole groups
            const uint32_t ng_max = wave_max(my_ng + (tail ? 1u : 0u));
            if (ng_max) {
                uint32_t obase[4];
                uint32_t ong[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t os = base0 + seg_of<NT>((tid & ~63u) + 16u * k + (tid & 15u));
                    const uint32_t oq = os * I;
                    ong[k] = os < nseg ? (min(oq + I, Pm) - oq) / G1 : 0u;
                    obase[k] = oq;
                }
                run_groups_tx(c, my_ng, tail, ng_max, sm.pay, dtb, out, obase, ong, (tid >> 4) & 3u, p0);
            }
            if (act) {  // every step is decoded: only the final state's symbol is left, for the last segment
                r = run_chain1(c.c, sm.pay, dtb, p1, p1, lastseg, n, out, hdr_bits);
                if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, c.c.pos, c.c.a, 0u))
                    r = FSE_ERR_BAD_SIDECAR;
            }
            if (r != FSE_OK) err = r;
        }
    }
    for (uint32_t base = base0; base < nseg; base += NT) {
        const uint32_t seg = base + (NS == 2 ? seg_of<NT>(tid) : tid);
        if (seg >= nseg) continue;
        const uint64_t e = sc[seg];
        const uint32_t p0 = seg * I, p1 = min(p0 + I, Pm);
        const uint32_t bp = (uint32_t)e;
        uint32_t s0 = (uint32_t)(e >> 32) & smask, s1 = NS == 2 ? (uint32_t)(e >> 48) & smask : 0u;
        const bool lastseg = seg == nseg - 1u;
        const uint64_t en = lastseg ? 0ull : sc[seg + 1u];
        int32_t r;
        if (bp > maxbp) {  // corrupt index: never read outside the block
            r = FSE_ERR_BAD_SIDECAR;
        } else if (NS == 1) {
            if (!BIG && in_lds) {
                LdsChain1 c;
                c.init(sm.pay, hdr_bits + (int32_t)bp, s0);
                r = run_chain1(c, sm.pay, dtb, p0, p1, lastseg, n, out, hdr_bits);
                if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, c.pos, c.a, 0u)) r = FSE_ERR_BAD_SIDECAR;
            } else {
                WindowReader br;
                br.init(gw, hdr_bits + (int32_t)bp);
                r = decode_segment1<LMAX>(br, s0, p0, p1, lastseg, n, out, sm.dt, hdr_bits);
                if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, br.pos, s0 << 2, 0u))
                    r = FSE_ERR_BAD_SIDECAR;
            }
        } else if (!BIG && in_lds) {
            Chain c;
            c.init(sm.pay, hdr_bits + (int32_t)bp, s0, s1);
            r = run_chain(c, sm.pay, dtb, p0, p1, lastseg, n, Pm, out, hdr_bits);
            if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, c.pos, c.a0, c.a1)) r = FSE_ERR_BAD_SIDECAR;
        } else {
            WindowReader br;
            br.init(gw, hdr_bits + (int32_t)bp);
            r = decode_segment<LMAX>(br, s0, s1, p0, p1, lastseg, n, Pm, out, sm.dt, hdr_bits);
            if (r == FSE_OK && !lastseg && !ckpt_match(en, hdr_bits, smask, br.pos, s0 << 2, s1 << 2))
                r = FSE_ERR_BAD_SIDECAR;
        }
        if (r != FSE_OK) err = r;
    }
    err = -(int32_t)wave_max((uint32_t)(-err));
    if (lane == 0) sm.err[wv] = err;
    __syncthreads();
    FSE_STAMP(P, 4);
    if (tid == 0) {
        int32_t e2 = FSE_OK;
        for (uint32_t w = 0; w < NW; ++w)
            if (sm.err[w] != FSE_OK) e2 = sm.err[w];
        P.status[gb] = e2;
        if (P.out_len) P.out_len[gb] = e2 ? 0u : n;
    }
}

// PASS 0 (every block) / 1 (blocks the stage holds; the others are marked
// FSE_DEFERRED): one block per workgroup, grid = blocks.  PASS 2 (the
// 66 KiB stage, 2 workgroups per CU): a grid of about one workgroup per slot
// on the chip; workgroup w collects the deferred blocks among w, w + G,
// w + 2G, ... (256 status reads at once, compacted in LDS) and decodes them
// one after the other, so a batch with few or no deferred blocks costs a few
// microseconds instead of a full-grid launch of empty workgroups (~0.03 ms
// per GiB).
// Waves per SIMD that the workgroups a CU's 160 KiB of LDS holds come to:
// the register allocator is held to that occupancy (80 VGPRs for the three
// 512-thread workgroups of the 44 KiB stage), as it otherwise spends
// registers on scheduling freedom that costs a resident workgroup.
template <class Smem>
constexpr uint32_t lds_waves_per_simd(uint32_t nw) {
    const uint32_t w = (160u << 10) / (uint32_t)sizeof(Smem) * nw / 4u;
    return w < 1u ? 1u : w > 8u ? 8u : w;
}

template <int LMAX, uint32_t PMAX, int NS, int PASS, uint32_t NT = 256u>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(
    lds_waves_per_simd<PreSmem<LMAX, (LMAX > 14) ? 16u : PMAX, NT / 64u>>(NT / 64u)))) void
decode_pre_kernel(DecParams P) {
    constexpr bool BIG = LMAX > 14;
    constexpr uint32_t NW = NT / 64u;
    __shared__ PreSmem<LMAX, BIG ? 16u : PMAX, NW> sm;
    if constexpr (PASS <= 1) {
        decode_pre_block<LMAX, PMAX, NS, NT>(P, sm, blockIdx.x);
    } else {
        // the deferred blocks among this workgroup's NT candidates, as one
        // ballot mask per wave (64 B of LDS instead of an NT-entry list: the
        // L = 12 list pass fits 2 workgroups per CU with a 65,392-byte stage)
        __shared__ uint64_t dmask[NW];
        const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
        const uint64_t G = gridDim.x;
        for (uint64_t r0 = blockIdx.x; r0 < P.n_blocks; r0 += G * NT) {
            const uint64_t gb = r0 + G * tid;
            const bool d = gb < P.n_blocks && P.status[gb] == FSE_DEFERRED;
            const uint64_t m = __ballot(d);
            if (lane == 0) dmask[wv] = m;
            __syncthreads();
            for (uint32_t w = 0; w < NW; ++w) {
                for (uint64_t mw = dmask[w]; mw; mw &= mw - 1u)  // workgroup-uniform
                    decode_pre_block<LMAX, PMAX, NS, NT>(P, sm, r0 + G * (64u * w + (uint32_t)__builtin_ctzll(mw)));
            }
            __syncthreads();  // dmask is rewritten by the next round
        }
    }
}

// ------------------------------------------------------------------------
// launch wrapper
// ------------------------------------------------------------------------
#ifndef FSE_DEC_PP
#define FSE_DEC_PP (44u << 10)  // a variant build may lower it (occupancy probes)
#endif
// The two passes of table log L: pass 1 with the `first` stage for the
// blocks it holds, then a list pass (a grid of one workgroup per slot on the
// chip, per_cu workgroups per CU) with the `list` stage for the deferred
// ones.  Blocks above the list stage use the windowed global-memory reader.
//   L <= 11  44 KiB (3 workgroups per CU), then 66 KiB (2 per CU) for
//            near-uniform data, ~65 KB
//   L = 12   36 KiB (3 per CU), then the most that keeps 2 per CU beside the
//            16 KiB table (near-uniform blocks, ~65.3 KB, fit; 1 per CU with
//            66 KiB)
//   L 13, 14 as L <= 11; the 32 and 64 KiB tables leave the list pass 1 per CU
struct SegStages {
    uint32_t first, list, per_cu;
};
constexpr SegStages seg_stages(int L) {
    return L == 12 ? SegStages{FSE_DEC_PP - 8192u, 65392u, 2u} : SegStages{FSE_DEC_PP, 66u << 10, L <= 11 ? 2u : 1u};
}
// PS14: the small first stage of the three passes at L = 14, 2-state, 512
// threads (2 workgroups per CU beside the 64 KiB table)
constexpr uint32_t PS14 = 12u << 10;
// Threads per workgroup for blocks with more than 256 segments (checkpoints
// every <= 64 pairs or 128 symbols at 64 KiB): 512, one segment per thread --
// the same LDS per block, more waves per CU -- at every 2-state table log,
// and for 1-state at L = 11 only
constexpr uint32_t seg_wide_nt(int L, int NS) { return NS == 2 || L == 11 ? 512u : 256u; }

template <int L, int NS, uint32_t NT>
static void launch_seg_passes(const DecParams& P, uint32_t cus, hipStream_t stream) {
    auto run = [&](auto kern, uint32_t pass, uint32_t per_cu) {
        DecParams Q = P;
        Q.pass = pass;
        const dim3 gq(pass <= 1 ? P.n_blocks : std::min<uint32_t>(P.n_blocks, per_cu * cus));
        hipLaunchKernelGGL(kern, gq, dim3(NT), 0, stream, Q);
    };
    constexpr SegStages S = seg_stages(L);
    if constexpr (L == 15) {
        // 128 KiB table, 1 workgroup per CU: no image stage, every block reads
        // through the window (512 threads: 8 waves instead of 4, near-uniform
        // C5 L = 15 decode 72.7 -> 77.2 GiB/s, profiles/r06/w15/)
        run(decode_pre_kernel<15, 16, NS, 0, NT>, 0, 0);
    } else if constexpr (L == 14 && NS == 2 && NT == 512u) {
        // 64 KiB table: a 12 KiB stage first (2 workgroups per CU: skewed
        // blocks fit), then the 44 and 66 KiB stages as list passes (1 per
        // CU): C5 skewed L = 14 decode 342 -> 368 GiB/s, near-uniform
        // unchanged (profiles/r06/sd/)
        run(decode_pre_kernel<14, PS14, 2, 1, 512>, 1, 0);
        run(decode_pre_kernel<14, S.first, 2, 3, 512>, 3, 1);
        run(decode_pre_kernel<14, S.list, 2, 2, 512>, 2, 1);
    } else {
        // (at L = 13, 512 threads, a 16 KiB first stage, 3 per CU, measured a
        // wash: skewed +2.5 %, near-uniform -1 %, profiles/r06/sd/)
        run(decode_pre_kernel<L, S.first, NS, 1, NT>, 1, 0);
        run(decode_pre_kernel<L, S.list, NS, 2, NT>, 2, S.per_cu);
    }
}

hipError_t launch_decode_seg(const DecParams& P, uint32_t lmax, hipStream_t stream) {
    static const uint32_t cus = [] {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return (uint32_t)n;
    }();
    const uint32_t bs = P.block_size;
    // main-loop steps of a full block: pairs (2-state) or symbols (1-state)
    const uint32_t pm = bs < 2u ? 0u : P.nstates == 1 ? bs - 1u : (bs & 1u) ? (bs - 3u) / 2u : bs / 2u - 1u;
    const bool wide = pm / std::max(P.ckpt_interval, 1u) + 1u > 256u;  // segments per block
    with_lmax(lmax, [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        if (P.nstates == 1) (wide ? launch_seg_passes<L, 1, seg_wide_nt(L, 1)> : launch_seg_passes<L, 1, 256u>)(P, cus, stream);
        else (wide ? launch_seg_passes<L, 2, seg_wide_nt(L, 2)> : launch_seg_passes<L, 2, 256u>)(P, cus, stream);
    });
    return hipGetLastError();
}

int occupancy_lines_seg(char* buf, int len, int cap) {
    len = occupancy_line(buf, len, cap, "decode_pre<11,45056,2,1>",
                         reinterpret_cast<const void*>(decode_pre_kernel<11, 45056u, 2, 1>));
    len = occupancy_line(buf, len, cap, "decode_pre<11,45056,2,1,512>",
                         reinterpret_cast<const void*>(decode_pre_kernel<11, 45056u, 2, 1, 512>));
    return occupancy_line(buf, len, cap, "decode_pre<11,67584,2,2>",
                          reinterpret_cast<const void*>(decode_pre_kernel<11, 67584u, 2, 2>));
}

}  // namespace fsehip
