// fse_decode_serial.hip -- sidecar-less decode of a batch of blocks on
// prebuilt tables (fse_decode_tables.hip), gfx950: one lane walks each block
// with the reference's end checks.  Container mode (raw length known) or the
// reference's own termination within a capacity (host streams of unknown
// length); the 2-state kernels can record the sidecar as they go.
//
//   serial_ring_kernel     L <= 12, 2-state and 1-state: K blocks per
//                          workgroup, lane j of the decode wave walking block
//                          j on u16 tables in LDS, a loader wave streaming
//                          each block's payload into an LDS ring
//   sym_map_kernel         L <= 11: the ring kernel's deferred symbols
//                          (DEF = true: the chains store states), mapped to
//                          bytes by one workgroup per block
//   serial2_decode_kernel  L 13..15, 2-state: one lane per block, the table
//                          in LDS, the bits through a register window
//   decode1_serial_kernel  L 13..15, 1-state (fse_decompress): one lane per
//                          block on the table in HBM
#include <type_traits>

#include "fse_decode_dev.hpp"
#include "fse_decode_host.h"

namespace fsehip {

// ------------------------------------------------------------------------
// fse_decompress (lib.rs:187-211) without a sidecar: one lane per block
// walks the stream with every read checked, on tables from
// dtable_blocks_kernel.  Container mode (raw length known) or the
// reference's own termination with a capacity (host streams).
// ------------------------------------------------------------------------
template <int LMAX>
__global__ __launch_bounds__(64) void decode1_serial_kernel(DecParams P) {
    const uint64_t gb = blockIdx.x;
    if (gb >= P.n_blocks) return;
    const int32_t info = P.dtinfo[gb];
    // single-symbol table (every nb 0): the whole wave scans it
    uint32_t nbor = 0;
    if (info >= 0) {
        const uint32_t* t = P.dt + gb * (uint64_t)(1u << LMAX);
        for (uint32_t i = threadIdx.x; i < (1u << ((uint32_t)info >> 16)); i += 64u) nbor |= t[i] & 0xFFu;
    }
    const bool single = __ballot(nbor != 0u) == 0ull;
    if (threadIdx.x != 0) return;
    if (info < 0) {
        P.status[gb] = info;
        if (P.out_len) P.out_len[gb] = 0;
        return;
    }
    const uint8_t* in = P.in + gb * P.slot_bytes;
    const uint32_t clen = P.comp_len[gb];
    const int32_t hdr_bits = (info & 0xFFFF) * 8;
    const uint32_t L = (uint32_t)info >> 16;
    const uint32_t* dt = P.dt + gb * (uint64_t)(1u << LMAX);
    uint8_t* out = P.out + gb * (uint64_t)P.block_size;
    const bool known = P.n_total != 0;  // container length, else reference mode with a capacity
    const uint32_t n = known ? (uint32_t)min((uint64_t)P.block_size, P.n_total - gb * (uint64_t)P.block_size) : 0u;
    const uint32_t cap = known ? n : P.out_cap;
    int32_t err = FSE_OK;
    uint32_t o = 0;
    const int32_t top = (int32_t)(clen - 1u) * 8 + (int32_t)ilog2u(in[clen - 1]);  // marker (BitStackReader::new)
    WindowReader br;
    br.init(reinterpret_cast<const uint32_t*>(in), top);
    if (br.pos - (int32_t)L < hdr_bits) {
        err = FSE_ERR_TOO_SHORT;  // lib.rs:197 unwrap
    } else {
        uint32_t s = br.pop(L);
        br.refill();
        for (;;) {
            if (known && single && o + 1u >= n) break;  // raw length ends a single-symbol block
            const uint32_t e = dt[s];
            const uint32_t nb = dte_nb(e);
            if (br.pos - (int32_t)nb < hdr_bits) break;  // decode_symbol -> None
            if (o >= cap) {  // a single-symbol table never ends in the reference (the oracle refuses
                             // it up front); any other stream simply needs more room
                err = single ? FSE_ERR_SINGLE_SYMBOL : FSE_ERR_DST_TOO_SMALL;
                break;
            }
            s = Dte<LMAX>::ns(e) + br.pop(nb);
            br.refill();
            out[o++] = (uint8_t)dte_sym(e);
        }
        if (err == FSE_OK) {
            if (o >= cap) err = FSE_ERR_DST_TOO_SMALL;
            else out[o++] = (uint8_t)dte_sym(dt[s]);  // Decoder::finish (lib.rs:208)
        }
        if (known && (err == FSE_ERR_DST_TOO_SMALL || (err == FSE_OK && o != n))) err = FSE_ERR_LENGTH_MISMATCH;
    }
    P.status[gb] = err;
    if (P.out_len) P.out_len[gb] = err ? 0u : o;
}

// ------------------------------------------------------------------------
// Sidecar-less decode of 2-state blocks (any valid fse_compress2 stream,
// e.g. from the CPU crate), optionally recording the sidecar.  The two
// interleaved decoders make the stream essentially serial: a decoder
// started mid-block with guessed states practically never falls into step
// with the exact one (oracle/syncsim.py: 35 of 40 random starts in a C2
// block never did, the rest after 25K-40K symbols), so speculative segment
// decoding cannot replace the sidecar for this format.  The
// serial decode is instead made as short a dependency chain as possible and
// run at high occupancy.  This kernel serves tables above L = 12 (128 KiB
// at L = 15): the block's prebuilt table sits in LDS, one lane walks the
// stream (lib.rs:227-244) and the bits come through a register window fed
// from 16-byte chunks loaded a chunk ahead.  At L <= 12 serial_ring_kernel
// below replaces it (3x faster at C2).
//   Container mode (n_total > 0): the raw length ends the block, as the
//   oracle's decompress2 with a known length.
//   Reference mode (n_total == 0, the host fse_decompress2): the block ends
//   where a decoder's read fails (lib.rs:228-243), within out_cap bytes; a
//   single-symbol table never ends in the reference and is refused.
// ------------------------------------------------------------------------
struct ChunkReader {
    const uint4* w4;  // the block as 16-byte quads
    uint64_t buf;     // stream bits [base, base + 64)
    int32_t base, pos;
    uint4 cl, ch, nl, nh;  // chunk c (words 8c..8c+7) and chunk c-1, loading
    int32_t c;
    __device__ __forceinline__ void init(const uint8_t* in, int32_t p) {
        w4 = reinterpret_cast<const uint4*>(in);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(in);
        pos = p;
        base = max(((p + 31) & ~31) - 64, 0);
        buf = (uint64_t)w[base >> 5] | ((uint64_t)w[(base >> 5) + 1] << 32);
        c = ((base >> 5) - 1) >> 3;  // chunk of the next word to enter the window
        cl = w4[2 * max(c, 0)];
        ch = w4[2 * max(c, 0) + 1];
        nl = w4[2 * max(c - 1, 0)];
        nh = w4[2 * max(c - 1, 0) + 1];
    }
    __device__ __forceinline__ uint32_t pop(uint32_t nb) {
        pos -= (int32_t)nb;
        return (uint32_t)(buf >> (uint32_t)(pos - base)) & ((1u << nb) - 1u);
    }
    __device__ __forceinline__ void refill() {
        if (pos - base < 32 && base > 0) {
            base -= 32;
            const int32_t wi = base >> 5;
            if ((wi >> 3) != c) {  // every 8th refill: move down a chunk, prefetch the next
                cl = nl;
                ch = nh;
                c -= 1;
                nl = w4[2 * max(c - 1, 0)];
                nh = w4[2 * max(c - 1, 0) + 1];
            }
            const uint32_t j = (uint32_t)wi & 7u;
            const uint4 q = j < 4u ? cl : ch;
            const uint32_t k = j & 3u;
            const uint32_t v = k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w;
            buf = (buf << 32) | v;
        }
    }
};

template <int LMAX>
__global__ __launch_bounds__(64) void serial2_decode_kernel(DecParams P) {
    __shared__ uint32_t tab[1u << LMAX];
    const uint64_t gb = blockIdx.x;
    if (gb >= P.n_blocks) return;
    const int32_t info = P.dtinfo[gb];
    const uint32_t lane = threadIdx.x;
    uint32_t nbor = 0;  // OR of the staged entries' nb: 0 = single-symbol table
    if (info >= 0) {  // stage the table (prebuilt by dtable_blocks_kernel)
        const uint32_t nv = (1u << ((uint32_t)info >> 16)) >> 2;  // 16-byte chunks
        const uint4* t4 = reinterpret_cast<const uint4*>(P.dt + gb * (uint64_t)(1u << LMAX));
        uint4* d4 = reinterpret_cast<uint4*>(tab);
        for (uint32_t i = lane; i < nv; i += 64u) {
            const uint4 q = t4[i];
            d4[i] = q;
            nbor |= (q.x | q.y | q.z | q.w) & 0xFFu;
        }
    }
    const bool single = __ballot(nbor != 0u) == 0ull;
    __syncthreads();
    if (lane != 0) return;
    const uint8_t* in = P.in + gb * P.slot_bytes;
    const uint32_t clen = P.comp_len[gb];
    const bool known = P.n_total != 0;
    const uint64_t ooff = gb * (uint64_t)P.block_size;
    const uint32_t n = known ? (uint32_t)min((uint64_t)P.block_size, P.n_total - ooff) : 0u;
    const uint32_t lim = known ? n : P.out_cap;  // bytes the block may produce
    uint8_t* out = P.out + ooff;
    int32_t err = info < 0 ? info : FSE_OK;
    if (err == FSE_OK && known && n < 2) err = FSE_ERR_LENGTH_MISMATCH;
    if (err == FSE_OK && !known && single) err = FSE_ERR_SINGLE_SYMBOL;  // the reference loops forever
    const int32_t hdr_bits = (info & 0xFFFF) * 8;
    const uint32_t L = (uint32_t)info >> 16;
    uint32_t o = 0;
    if (err == FSE_OK) {
        const int32_t top = (int32_t)(clen - 1u) * 8 + (int32_t)ilog2u(in[clen - 1]);
        if (top - 2 * (int32_t)L < hdr_bits) err = FSE_ERR_TOO_SHORT;  // lib.rs:224-225
    }
    if (err == FSE_OK) {
        ChunkReader br;
        br.init(in, (int32_t)(clen - 1u) * 8 + (int32_t)ilog2u(in[clen - 1]));
        uint32_t s0 = br.pop(L);
        br.refill();
        uint32_t s1 = br.pop(L);
        br.refill();
        const uint32_t I = P.ckpt_interval;
        uint64_t* rec = (P.sidecar_out && I) ? P.sidecar_out + gb * P.ckpt_per_block : nullptr;
        const uint32_t ckmask = I ? I - 1u : 0u;
        uint32_t pidx = 0;
        auto record = [&]() {
            if (rec && (pidx & ckmask) == 0u && pidx / I < P.ckpt_per_block)
                rec[pidx / I] = (uint64_t)(uint32_t)(br.pos - hdr_bits) | ((uint64_t)s0 << 32) | ((uint64_t)s1 << 48);
        };
        // bulk: groups of 8 pairs that can neither reach the raw length (or
        // the capacity) nor run out of bits (<= 2L bits a pair): no end
        // checks, and the 16 output bytes leave as one dwordx4 store, so few
        // stores are in flight when the next chunk's load is waited on
        while (o + 18u < lim && br.pos - hdr_bits >= 16 * (int32_t)L) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j, ++pidx) {
                record();
                const uint32_t e0 = tab[s0];
                s0 = Dte<LMAX>::ns(e0) + br.pop(dte_nb(e0));
                br.refill();
                const uint32_t e1 = tab[s1];
                s1 = Dte<LMAX>::ns(e1) + br.pop(dte_nb(e1));
                br.refill();
                const uint32_t v = dte_sym(e0) | (dte_sym(e1) << 8);
                if (j & 1u) w[j >> 1] |= v << 16; else w[j >> 1] = v;
            }
            *reinterpret_cast<uint4*>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
            o += 16;
        }
        // tail: pair by pair with the reference's end checks
        const int32_t full = known ? FSE_ERR_LENGTH_MISMATCH : FSE_ERR_DST_TOO_SMALL;
        for (;; ++pidx) {
            record();
            if (known && o + 2u >= n) {  // the raw length ends the block (o is even here)
                if (o < n) out[o++] = (uint8_t)dte_sym(tab[s0]);
                if (o < n) out[o++] = (uint8_t)dte_sym(tab[s1]);
                break;
            }
            const uint32_t e0 = tab[s0];
            uint32_t nb = dte_nb(e0);
            if (br.pos - (int32_t)nb < hdr_bits) {  // decoder 0 cannot read: lib.rs:242-243
                if (o + 2u > lim) { err = full; break; }
                out[o++] = (uint8_t)dte_sym(e0);
                out[o++] = (uint8_t)dte_sym(tab[s1]);
                break;
            }
            s0 = Dte<LMAX>::ns(e0) + br.pop(nb);
            br.refill();
            if (o >= lim) { err = full; break; }
            out[o++] = (uint8_t)dte_sym(e0);
            const uint32_t e1 = tab[s1];
            nb = dte_nb(e1);
            if (br.pos - (int32_t)nb < hdr_bits) {  // decoder 1 cannot read: lib.rs:235-239
                if (o + 2u > lim) { err = full; break; }
                out[o++] = (uint8_t)dte_sym(e1);
                out[o++] = (uint8_t)dte_sym(tab[s0]);
                break;
            }
            s1 = Dte<LMAX>::ns(e1) + br.pop(nb);
            br.refill();
            if (o >= lim) { err = full; break; }
            out[o++] = (uint8_t)dte_sym(e1);
        }
        if (err == FSE_OK && known && o != n) err = FSE_ERR_LENGTH_MISMATCH;
    }
    P.status[gb] = err;
    if (P.out_len) P.out_len[gb] = err ? 0u : o;
}

// ------------------------------------------------------------------------
// Sidecar-less 2-state decode at L <= 12 (the serial decode above, made
// 3x faster at C2).  Two things bound that kernel: its single lane is
// provably lane 0, so the compiler runs the chain as wave-uniform SALU+VALU
// code (~30 issue slots per pair for one chain), and its register window
// waits on the global prefetch at every refill (the compiler merges the
// prefetched registers at each refill branch, so it waits for the load,
// and for any output store issued after it).  Here:
//   - K blocks per workgroup, lane j of wave 0 walking block j: one VALU
//     instruction advances K chains, and LDS caps the chains per CU (K = 6
//     at L <= 11: 6 x (6 KiB table + 512 B ring) = 40.0 KB, 4 workgroups =
//     24 chains per CU; K = 3 at L = 12: 3 x 12.5 KiB, 12 chains per CU);
//   - wave 1 streams each block's payload top down into its 128-word LDS
//     ring in 256-byte chunks (one dword per lane), one chunk ahead of the
//     one being decoded (a chunk lasts ~170 pairs, ~17 us: far longer than a
//     load), and publishes the lowest word landed (ctl[0]);
//   - the decode lanes read only LDS (one payload word and the two table
//     entries per pair, issued together, as the segment decoder's
//     LdsChain), publish the highest word they may still read every 8 pairs
//     (ctl[1]) and store their output without ever waiting on memory.
// Same end checks, statuses and sidecar recording as serial2.
// ------------------------------------------------------------------------
constexpr uint32_t RING_WORDS = 128u, RING_MASK = RING_WORDS - 1u, RING_CHUNK = 64u;
#ifndef FSE_RING_GROUP
#define FSE_RING_GROUP 32
#endif
// state words (pairs, or two 1-state symbols) per bulk iteration with the
// symbols deferred; a multiple of 8 (whole 16-byte groups for sym_map_kernel).
// The loop's control (~45 instructions an iteration: the ring wait, the
// stores, the published position) is paid once per group: C2 sidecar-less
// decode 8.07 ms at 8, 7.31 at 16, 7.01 at 32, 7.20 at 64 (profiles/r06/rg/)
constexpr uint32_t RING_GROUP = FSE_RING_GROUP;
#ifndef FSE_RING_GROUP_SYM
#define FSE_RING_GROUP_SYM 32
#endif
// the same for the kernels that write the symbols themselves (L = 12, the
// fallback without the state workspace, sidecar rebuilds): 32 against 8,
// skewed L = 12 sidecar-less 17.5 -> 16.3 ms per GiB, C2 sidecar rebuild
// 11.7 -> 10.7 ms (profiles/r06/rg/)
constexpr uint32_t RING_GROUP_SYM = FSE_RING_GROUP_SYM;
static_assert(RING_GROUP_SYM % 8u == 0u && RING_GROUP_SYM <= 64u, "ring group");
static_assert(RING_GROUP % 8u == 0u && RING_GROUP <= 64u, "ring group: the tail waits for (2 RING_GROUP + 4) L bits, 45 words at 64");

// Relaxed workgroup-scope atomics keep these as plain ds_read/ds_write (a
// volatile access through a generic pointer becomes a FLAT access that
// waits on vmcnt, i.e. on the output stores); the asm barriers pin their
// place among the ring reads and writes, and LDS runs one wave's accesses
// in order.
__device__ __forceinline__ int32_t lds_load_volatile(int32_t* p) {
    const int32_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __asm__ __volatile__("" ::: "memory");
    return v;
}
__device__ __forceinline__ void lds_store_volatile(int32_t* p, int32_t v) {
    __asm__ __volatile__("" ::: "memory");
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The ring handoff proper: the loader publishes "landed" with release
// semantics after its ring writes, the decoder reads it with acquire (only
// on its slow path, when the cached value is not low enough).  The
// decoder's "still needed" hints stay relaxed: a stale value is a higher
// one, which only makes the loader wait.
__device__ __forceinline__ int32_t lds_load_acquire(int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store_release(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

typedef __attribute__((address_space(3))) const uint16_t lds_cu16;
typedef __attribute__((address_space(3))) const uint8_t lds_cu8;
typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
__device__ __forceinline__ uint32_t lds_u16_at(uint32_t a) { return *(lds_cu16*)(uintptr_t)a; }
__device__ __forceinline__ uint32_t lds_u8_at(uint32_t a) { return *(lds_cu8*)(uintptr_t)a; }
__device__ __forceinline__ uint32_t lds_u32_at(uint32_t a) { return *(lds_cu32*)(uintptr_t)a; }
template <class T>
__device__ __forceinline__ uint32_t lds_addr(T* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) T*)p;
}

// The sidecar-less decoder's tables in LDS: for the K blocks of a
// workgroup, u16 entries nb | newState << NBW (ent[K][2^LMAX]) followed by
// u8 symbols (sym[K][2^LMAX]), 3 bytes per state (6 KiB at L = 11, 12 KiB
// at L = 12, against 8 / 16 KiB of dtable_blocks_kernel's u32 entries), so
// with 528-byte rings 6 blocks fit a 40 KB workgroup at L <= 11 and 3 at
// L = 12 (4 workgroups per CU).  A chain's state is its entry's LDS byte
// address halved, B = H + state (H = its entry table / 2): the entry is at
// 2B and the symbol at B + SO, SO = sym - ent / 2 being the same for every
// chain (the ds_read's immediate offset), and the next state is
// H + newState + bits (one add3).
// NBW = 5 (L <= 11): nb < 16 leaves bit 4 clear, so the entry is the v_bfe
// width as it is and -e its offset below the top.  NBW = 4 (L = 12,
// newState needs 12 bits): nb = e & 15.  newState = e >> NBW.
template <uint32_t NBW>
struct RingTab {
    static_assert(NBW == 4 || NBW == 5, "nb field width");
    uint32_t H;   // this chain's entry table (LDS byte address) / 2
    uint32_t SO;  // symbol of state B: LDS byte B + SO
    __device__ __forceinline__ uint32_t entry_at(uint32_t B) const { return lds_u16_at(B << 1); }
    __device__ __forceinline__ uint32_t sym_at(uint32_t B) const { return ((lds_cu8*)(uintptr_t)B)[SO]; }
    // nb as a bit-field operand (v_bfe reads its low five bits)
    __device__ __forceinline__ uint32_t nbf(uint32_t e) const { return NBW == 5 ? e : e & 15u; }
    __device__ __forceinline__ uint32_t ns(uint32_t e) const { return e >> NBW; }
    // by state index (end-of-block steps)
    __device__ __forceinline__ uint32_t nb(uint32_t s) const { return entry_at(H + s) & ((1u << NBW) - 1u); }
    __device__ __forceinline__ uint32_t symbol(uint32_t s) const { return sym_at(H + s); }
    __device__ __forceinline__ uint32_t next_base(uint32_t s) const { return ns(entry_at(H + s)); }
};

// Ring of one chain: RING_WORDS words of the payload by word index mod
// RING_WORDS, plus a mirror of slot 0 in slot RING_WORDS, so that words
// (q, q + 1) are always two adjacent slots (one ds_read2_b32).
constexpr uint32_t RING_STRIDE = RING_WORDS + 4u;

// A serial chain over its ring.  NS = 2: a pair (<= 24 bits) per step;
// NS = 1: one symbol.  Each step reads x = the 32 payload bits just below
// pos (words (pos - 32) / 32 and the one above, issued together with the
// table reads: they depend only on pos), then takes decoder 0's nb0 bits
// from the top of x and decoder 1's nb1 bits below them (stack order,
// lib.rs:227-234) as bit fields at 32 - nb0 and 32 - nb0 - nb1: from a
// table read back to the next one is four VALU (negate, bfe, add3, shift)
// and no 64-bit shift or window bookkeeping.
template <int NS, uint32_t NBW>
struct RingChain {
    using Tab = RingTab<NBW>;
    int32_t p32;      // bit position - 32
    uint32_t B0, B1;  // states as halved entry addresses
    uint32_t R;       // this chain's ring (LDS byte address)
    __device__ __forceinline__ void init(uint32_t ring, const Tab& T, int32_t p, uint32_t s0, uint32_t s1) {
        p32 = p - 32;
        R = ring;
        B0 = T.H + s0;
        B1 = T.H + s1;
    }
    __device__ __forceinline__ int32_t pos() const { return p32 + 32; }
    __device__ __forceinline__ uint32_t s0(const Tab& T) const { return B0 - T.H; }
    __device__ __forceinline__ uint32_t s1(const Tab& T) const { return B1 - T.H; }
    // the 32 bits [pos - 32, pos); below bit 0 (pos < 32) the low bits are
    // stale ring contents that no step uses
    __device__ __forceinline__ uint32_t window() const {
        // one v_bfe and one v_lshl_add (from ubfe << 2 the compiler makes a
        // shift, a mask and an add: one VALU more per pair, 1.7 % of the
        // sidecar-less decode, profiles/r06/rg/)
        uint32_t wi;
        asm("v_bfe_u32 %0, %1, 5, 7" : "=v"(wi) : "v"(p32));
        const uint32_t a = R + (wi << 2);
        return __builtin_amdgcn_alignbit(lds_u32_at(a + 4u), lds_u32_at(a), (uint32_t)p32);
    }
    // one pair; returns sym0 | sym1 << 8
    __device__ __forceinline__ uint32_t pair(const Tab& T) {
        const uint32_t e0 = T.entry_at(B0), e1 = T.entry_at(B1);
        const uint32_t y0 = T.sym_at(B0), y1 = T.sym_at(B1);
        const uint32_t x = window();
        const uint32_t n0 = T.nbf(e0), n1 = T.nbf(e1);
        const uint32_t o0 = 0u - n0;
        const uint32_t v0 = __builtin_amdgcn_ubfe(x, o0, n0);
        const uint32_t v1 = __builtin_amdgcn_ubfe(x, o0 - n1, n1);
        p32 -= (int32_t)((n0 + n1) & 31u);
        B0 = T.H + T.ns(e0) + v0;
        B1 = T.H + T.ns(e1) + v1;
        return y0 | (y1 << 8);
    }
    // one pair with the symbols deferred: returns the two states (low 16
    // bits of each halved entry address) for sym_map_kernel
    __device__ __forceinline__ uint32_t pair_states(const Tab& T) {
        const uint32_t e0 = T.entry_at(B0), e1 = T.entry_at(B1);
        const uint32_t v = __builtin_amdgcn_perm(B1, B0, 0x05040100u);
        const uint32_t x = window();
        const uint32_t n0 = T.nbf(e0), n1 = T.nbf(e1);
        const uint32_t o0 = 0u - n0;
        const uint32_t v0 = __builtin_amdgcn_ubfe(x, o0, n0);
        const uint32_t v1 = __builtin_amdgcn_ubfe(x, o0 - n1, n1);
        p32 -= (int32_t)((n0 + n1) & 31u);
        B0 = T.H + T.ns(e0) + v0;
        B1 = T.H + T.ns(e1) + v1;
        return v;
    }
    // NS = 1, symbol deferred: advances; returns the state it left (halved address)
    __device__ __forceinline__ uint32_t step_state(const Tab& T) {
        const uint32_t e = T.entry_at(B0);
        const uint32_t b = B0;
        const uint32_t x = window();
        const uint32_t n0 = T.nbf(e);
        p32 -= (int32_t)(n0 & 31u);
        B0 = T.H + T.ns(e) + __builtin_amdgcn_ubfe(x, 0u - n0, n0);
        return b;
    }
    // NS = 1: one symbol; returns it
    __device__ __forceinline__ uint32_t step(const Tab& T) {
        const uint32_t e = T.entry_at(B0);
        const uint32_t y = T.sym_at(B0);
        const uint32_t x = window();
        const uint32_t n0 = T.nbf(e);
        p32 -= (int32_t)(n0 & 31u);
        B0 = T.H + T.ns(e) + __builtin_amdgcn_ubfe(x, 0u - n0, n0);
        return y;
    }
};

template <int LMAX, uint32_t K, int NS, bool DEF = false, uint32_t DW = 1>
__global__ __launch_bounds__(64 * (DW + 1)) void serial_ring_kernel(DecParams P) {
    static_assert(LMAX <= 12, "entry layout ns << 18: e >> 16 is the next entry's byte offset");
    static_assert(K >= 1 && K <= 64, "one decode lane per block");
    static_assert(!DEF || LMAX <= 11, "deferred symbols: L <= 11");
    static_assert(K % DW == 0, "DW decode waves of K / DW lanes each");
    constexpr uint32_t NT = 64u * (DW + 1u), KW = K / DW;
    constexpr uint32_t NBW = LMAX <= 11 ? 5u : 4u;  // nb | newState << NBW fits 16 bits
    constexpr uint32_t TW = 1u << LMAX;
    // u16 entries of the K blocks, then their u8 symbols (DEF: entries only;
    // the symbols are looked up by sym_map_kernel and, for the few end-of-block
    // steps, in the prebuilt u32 table in HBM)
    __shared__ __attribute__((aligned(16))) uint8_t tab_all[K * (DEF ? 2u : 3u) * TW];
    __shared__ uint32_t ring_all[K * RING_STRIDE];
    __shared__ int32_t ctl_all[K][2];  // [0] lowest word landed, [1] highest word the decoder may still read; INT32_MIN = stop
    __shared__ uint32_t any_nb[K];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t gb0 = (uint64_t)blockIdx.x * K;
    if (tid < K) {
        const uint64_t gb = gb0 + tid;
        int32_t nw = 0;
        if (gb < P.n_blocks && P.dtinfo[gb] >= 0) nw = (int32_t)((P.comp_len[gb] + 3u) >> 2);
        ctl_all[tid][0] = nw;  // nothing landed yet
        ctl_all[tid][1] = nw;
        any_nb[tid] = 0;
    }
    __syncthreads();
    for (uint32_t j = 0; j < K; ++j) {  // stage the prebuilt tables (dtable_blocks_kernel)
        const uint64_t gb = gb0 + j;
        if (gb >= P.n_blocks) break;
        const int32_t info = P.dtinfo[gb];
        if (info < 0) continue;
        const uint32_t nv = (1u << ((uint32_t)info >> 16)) >> 2;
        const uint4* t4 = reinterpret_cast<const uint4*>(P.dt + gb * (uint64_t)TW);
        uint8_t* tb = tab_all + j * 2u * TW;         // entries
        uint8_t* sb = tab_all + K * 2u * TW + j * TW;  // symbols
        uint32_t nbor = 0;
        for (uint32_t i = tid; i < nv; i += NT) {
            const uint4 q = t4[i];
            // nb | ns << NBW (ns = e >> 18; bits 16, 17 of e are clear) and the
            // symbols, 4 entries at a time
            auto c16 = [](uint32_t e) { return (e & 0xFu) | ((e >> (18u - NBW)) & ~((1u << NBW) - 1u)); };
            reinterpret_cast<uint2*>(tb)[i] =
                make_uint2(c16(q.x) | (c16(q.y) << 16), c16(q.z) | (c16(q.w) << 16));
            if (!DEF)
                reinterpret_cast<uint32_t*>(sb)[i] =
                    __builtin_amdgcn_perm(__builtin_amdgcn_perm(q.w, q.z, 0x0c0c0501u),
                                          __builtin_amdgcn_perm(q.y, q.x, 0x0c0c0501u), 0x05040100u);
            nbor |= (q.x | q.y | q.z | q.w) & 0xFFu;
        }
        if (nbor) atomicOr(&any_nb[j], 1u);
    }
    __syncthreads();

    if (tid >= 64u * DW) {  // the last wave: the loader, for all K rings (wave-uniform control)
        int32_t k[K], nwj[K];
        const uint32_t* wj[K];
        uint32_t act = 0;
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) {
            nwj[j] = ctl_all[j][1];
            k[j] = (nwj[j] - 1) / (int32_t)RING_CHUNK;
            wj[j] = reinterpret_cast<const uint32_t*>(P.in + (gb0 + j) * P.slot_bytes);
            if (nwj[j] > 0) act |= 1u << j;
        }
        // one sweep: every ring's chunk loads are issued before the first
        // ring write waits on them (a sweep that waited ring by ring took
        // ~K load latencies, near a chunk's decode time at K = 8)
        constexpr uint32_t NQ = RING_WORDS / RING_CHUNK;
        while (act) {
            uint32_t v[K][NQ];
            int32_t k1s[K];
            uint32_t mv = 0;
#pragma unroll
            for (uint32_t j = 0; j < K; ++j) {
                k1s[j] = k[j];
                if (!(act & (1u << j))) continue;
                const int32_t need = lds_load_volatile(&ctl_all[j][1]);
                if (need == INT32_MIN) {  // the decoder is done (or failed)
                    act &= ~(1u << j);
                    continue;
                }
                // chunk c may overwrite the slots of words 64c + RING_WORDS..: dead once above `need`
                int32_t k1 = k[j];
                while (k1 >= 0 && k1 > k[j] - (int32_t)NQ && k1 * (int32_t)RING_CHUNK + (int32_t)RING_WORDS > need)
                    --k1;
                if (k1 == k[j]) continue;
                k1s[j] = k1;
#pragma unroll
                for (int32_t q = 0; q < (int32_t)NQ; ++q) {
                    const int32_t wi = (k[j] - q) * (int32_t)RING_CHUNK + (int32_t)lane;
                    v[j][q] = (k[j] - q > k1 && wi < nwj[j]) ? wj[j][wi] : 0u;
                }
                mv |= 1u << j;
            }
#pragma unroll
            for (uint32_t j = 0; j < K; ++j) {
                if (!(mv & (1u << j))) continue;
                const int32_t k1 = k1s[j];
#pragma unroll
                for (int32_t q = 0; q < (int32_t)NQ; ++q)
                    if (k[j] - q > k1) {
                        const uint32_t slot = (uint32_t)((k[j] - q) * (int32_t)RING_CHUNK + (int32_t)lane) & RING_MASK;
                        ring_all[j * RING_STRIDE + slot] = v[j][q];
                        if (slot == 0u) ring_all[j * RING_STRIDE + RING_WORDS] = v[j][q];  // the mirror
                    }
                k[j] = k1;
                if (lane == 0) lds_store_release(&ctl_all[j][0], (k1 + 1) * (int32_t)RING_CHUNK);
                if (k1 < 0) act &= ~(1u << j);
            }
            if (!mv) __builtin_amdgcn_s_sleep(2);
        }
        return;
    }
    const uint32_t jc = (tid >> 6) * KW + lane;  // this lane's chain
    const uint64_t gb = gb0 + jc;
    if (lane >= KW || gb >= P.n_blocks) return;

    // wave 0, lane j < K: the decoder of block gb0 + j
    const uint32_t tab0 = lds_addr(tab_all);  // even (16-byte aligned)
    const RingTab<NBW> T{(tab0 >> 1) + jc * TW, K * 2u * TW + (tab0 >> 1)};
    const uint32_t* const ring = ring_all + jc * RING_STRIDE;
    int32_t* const ctl = ctl_all[jc];
    const int32_t info = P.dtinfo[gb];
    const uint32_t* const dtg = P.dt + gb * (uint64_t)TW;
    auto sym = [&](uint32_t s) -> uint32_t {  // symbol of state s (end-of-block steps)
        if constexpr (DEF) return dte_sym(dtg[s]);
        else return T.symbol(s);
    };
    const uint8_t* in = P.in + gb * P.slot_bytes;
    const uint32_t clen = info >= 0 ? P.comp_len[gb] : 0u;
    const int32_t nw = (int32_t)((clen + 3u) >> 2);
    const bool single = any_nb[jc] == 0u;
    const bool known = P.n_total != 0;
    const uint64_t ooff = gb * (uint64_t)P.block_size;
    const uint32_t n = known ? (uint32_t)min((uint64_t)P.block_size, P.n_total - ooff) : 0u;
    const uint32_t lim = known ? n : P.out_cap;
    uint8_t* out = P.out + ooff;
    int32_t err = info < 0 ? info : FSE_OK;
    if (NS == 2 && err == FSE_OK && known && n < 2) err = FSE_ERR_LENGTH_MISMATCH;
    // 2-state: a single-symbol table never ends in the reference (refused up
    // front); 1-state: as decode1_serial_kernel, at the capacity
    if (NS == 2 && err == FSE_OK && !known && single) err = FSE_ERR_SINGLE_SYMBOL;
    const int32_t hdr_bits = (info & 0xFFFF) * 8;
    const uint32_t L = (uint32_t)info >> 16;
    uint32_t o = 0, o_bulk = 0;
    // DEF: pair p's states at st_out[p], i.e. 2 bytes per output byte
    uint32_t* const st_out = DEF ? P.states + gb * (uint64_t)P.block_size / 2u : nullptr;
    int32_t top = 0;
    if (err == FSE_OK) {
        top = (int32_t)(clen - 1u) * 8 + (int32_t)ilog2u(in[clen - 1]);  // marker (BitStackReader::new)
        if (top - NS * (int32_t)L < hdr_bits) err = FSE_ERR_TOO_SHORT;  // lib.rs:197 / 224-225 unwrap
    }
    if (err == FSE_OK) {
        int32_t avail = nw;
        auto wait_words = [&](int32_t wlow) {  // words >= max(wlow, 0) have landed
            wlow = max(wlow, 0);
            while (avail > wlow) {
                avail = lds_load_acquire(&ctl[0]);
                if (avail > wlow) __builtin_amdgcn_s_sleep(1);
            }
        };
        // bits [p, p + 32) via the ring (end-of-block steps)
        auto bits_at = [&](int32_t p) -> uint32_t {
            const uint32_t wi = (uint32_t)p >> 5;
            return __builtin_amdgcn_alignbit(ring[(wi + 1u) & RING_MASK], ring[wi & RING_MASK], (uint32_t)p);
        };
        wait_words((top - NS * (int32_t)L) >> 5);
        const uint32_t s0i = bits_at(top - (int32_t)L) & ((1u << L) - 1u);
        const uint32_t s1i = NS == 2 ? bits_at(top - 2 * (int32_t)L) & ((1u << L) - 1u) : 0u;
        RingChain<NS, NBW> c;
        c.init(lds_addr(ring), T, top - NS * (int32_t)L, s0i, s1i);
        const uint32_t I = P.ckpt_interval;
        uint64_t* rec = (P.sidecar_out && I) ? P.sidecar_out + gb * P.ckpt_per_block : nullptr;
        // checkpoint before pair (NS = 2) / symbol (NS = 1) pidx: bit position
        // and the states, as the encoder records them
        uint32_t pidx = 0, next_ck = rec && P.ckpt_per_block ? 0u : 0xFFFFFFFFu, ck = 0;
        auto record_at = [&](int32_t p, uint32_t s0, uint32_t s1) {  // one compare per step when idle
            if (pidx == next_ck) {
                rec[ck++] = (uint64_t)(uint32_t)(p - hdr_bits) | ((uint64_t)s0 << 32) |
                            (NS == 2 ? (uint64_t)s1 << 48 : 0ull);
                next_ck = ck < P.ckpt_per_block ? next_ck + I : 0xFFFFFFFFu;
            }
        };
        // bulk: 2GS output bytes (GS pairs / 2GS symbols, <= 2GS L bits) without
        // end checks; the checkpoint compare is compiled in only when recording.
        // GS = RING_GROUP with the symbols deferred, RING_GROUP_SYM otherwise
        // (both 32: the loop's control is paid once per 32 pairs)
        constexpr uint32_t GS = DEF ? RING_GROUP : RING_GROUP_SYM;
        auto bulk = [&](auto rec_on) {
            constexpr bool REC = decltype(rec_on)::value;
            auto record = [&]() {
                if (REC) record_at(c.pos(), c.s0(T), c.s1(T));
            };
            while (o + 2u * GS + 2u < lim && c.pos() - hdr_bits >= 2 * (int32_t)GS * (int32_t)L) {
                wait_words((c.pos() - 32 - 2 * (int32_t)GS * (int32_t)L) >> 5);
                // DEF: the states of 2GS symbols, 2 bytes per output byte; else
                // the 2GS symbols themselves
                uint32_t v[DEF ? GS : GS / 2u];
                if constexpr (DEF) {
#pragma unroll
                    for (uint32_t j = 0; j < GS; ++j) {
                        if constexpr (NS == 2) {
                            v[j] = c.pair_states(T);
                        } else {
                            const uint32_t a = c.step_state(T);
                            v[j] = __builtin_amdgcn_perm(c.step_state(T), a, 0x05040100u);
                        }
                    }
                } else if constexpr (NS == 2) {
#pragma unroll
                    for (uint32_t j = 0; j < GS; j += 2u) {
                        record();
                        const uint32_t lo = c.pair(T);
                        ++pidx;
                        record();
                        const uint32_t hi = c.pair(T);
                        ++pidx;
                        v[j >> 1] = lo | (hi << 16);
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < GS / 2u; ++j) {
                        uint32_t y = 0;
#pragma unroll
                        for (uint32_t q = 0; q < 4u; ++q) {
                            record();
                            y |= c.step(T) << (8u * q);
                            ++pidx;
                        }
                        v[j] = y;
                    }
                }
                uint4* sp = DEF ? reinterpret_cast<uint4*>(st_out + (o >> 1)) : reinterpret_cast<uint4*>(out + o);
#pragma unroll
                for (uint32_t q = 0; q < (DEF ? GS : GS / 2u) / 4u; ++q)
                    sp[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
                o += 2u * GS;
                lds_store_volatile(&ctl[1], c.pos() >> 5);  // the highest word a later step reads
            }
        };
        if (DEF) bulk(std::false_type{});  // (never with a sidecar to record)
        else if (rec) bulk(std::true_type{});
        else bulk(std::false_type{});
        o_bulk = o;
        // the tail reads words <= pos/32 + 1, and it ends within 2GS L bits
        // (bulk stopped by the position) or within 2GS + 2 symbols (stopped by
        // the output limit): wait for just those words, the loader cannot pass
        // the ring's words above what the decoder still reads
        lds_store_volatile(&ctl[1], (c.pos() >> 5) + 1);
        wait_words(max(hdr_bits, c.pos() - (2 * (int32_t)GS + 4) * (int32_t)L) >> 5);
        uint32_t s0 = c.s0(T), s1 = c.s1(T);
        int32_t pos = c.pos();
        auto pop = [&](uint32_t nb) -> uint32_t {
            pos -= (int32_t)nb;
            return bits_at(pos) & ((1u << nb) - 1u);
        };
        if constexpr (NS == 2) {
            // tail: pair by pair with the reference's end checks (lib.rs:227-244)
            const int32_t full = known ? FSE_ERR_LENGTH_MISMATCH : FSE_ERR_DST_TOO_SMALL;
            for (;; ++pidx) {
                record_at(pos, s0, s1);
                if (known && o + 2u >= n) {
                    if (o < n) out[o++] = (uint8_t)sym(s0);
                    if (o < n) out[o++] = (uint8_t)sym(s1);
                    break;
                }
                uint32_t nb = T.nb(s0);
                if (pos - (int32_t)nb < hdr_bits) {  // decoder 0 cannot read: lib.rs:242-243
                    if (o + 2u > lim) { err = full; break; }
                    out[o++] = (uint8_t)sym(s0);
                    out[o++] = (uint8_t)sym(s1);
                    break;
                }
                const uint32_t y0 = sym(s0);
                s0 = T.next_base(s0) + pop(nb);
                if (o >= lim) { err = full; break; }
                out[o++] = (uint8_t)y0;
                nb = T.nb(s1);
                if (pos - (int32_t)nb < hdr_bits) {  // decoder 1 cannot read: lib.rs:235-239
                    if (o + 2u > lim) { err = full; break; }
                    out[o++] = (uint8_t)sym(s1);
                    out[o++] = (uint8_t)sym(s0);
                    break;
                }
                const uint32_t y1 = sym(s1);
                s1 = T.next_base(s1) + pop(nb);
                if (o >= lim) { err = full; break; }
                out[o++] = (uint8_t)y1;
            }
            if (err == FSE_OK && known && o != n) err = FSE_ERR_LENGTH_MISMATCH;
        } else {
            // tail: symbol by symbol (lib.rs:198-208), then Decoder::finish.  A
            // single-symbol table never fails a read (the reference loops
            // forever); with the raw length known it ends at n - 1 symbols.
            for (;; ++pidx) {
                if (known && single && o + 1u >= n) break;
                record_at(pos, s0, 0u);
                const uint32_t nb = T.nb(s0);
                if (pos - (int32_t)nb < hdr_bits) break;  // decode_symbol -> None
                if (o >= lim) {  // a single-symbol table never ends in the reference (the oracle
                                 // refuses it up front); any other stream simply needs more room
                    err = single ? FSE_ERR_SINGLE_SYMBOL : FSE_ERR_DST_TOO_SMALL;
                    break;
                }
                const uint32_t y = sym(s0);
                s0 = T.next_base(s0) + pop(nb);
                out[o++] = (uint8_t)y;
            }
            if (err == FSE_OK) {
                if (o >= lim) err = FSE_ERR_DST_TOO_SMALL;
                else out[o++] = (uint8_t)sym(s0);  // Decoder::finish (lib.rs:208)
            }
            if (known && (err == FSE_ERR_DST_TOO_SMALL || (err == FSE_OK && o != n))) err = FSE_ERR_LENGTH_MISMATCH;
        }
    }
    lds_store_volatile(&ctl[1], INT32_MIN);  // release the loader
    if (DEF)  // every block, so sym_map_kernel never reads a stale length
        reinterpret_cast<uint2*>(P.bulk)[gb] = make_uint2(err == FSE_OK ? o_bulk : 0u, T.H & (TW - 1u));
    P.status[gb] = err;
    if (P.out_len) P.out_len[gb] = err ? 0u : o;
}

// ------------------------------------------------------------------------
// Deferred symbols (serial_ring_kernel<..., DEF = true>): the chains wrote the
// state pair of each pair (low 16 bits of the halved entry addresses) instead
// of its two symbols, so their LDS holds u16 entries only (4 KiB per chain at
// L <= 11: 8 chains per 37 KB workgroup, 32 per CU instead of 24).  Here one
// workgroup per block stages the block's symbol column (dte_sym of the
// prebuilt u32 table) in LDS and maps the bulk's states to bytes: 2 bytes
// read and 1 written per output byte, fully parallel.  The chains' end-of-
// block steps wrote their bytes directly, above the bulk length.
// ------------------------------------------------------------------------
template <int LMAX>
__global__ __launch_bounds__(256) void sym_map_kernel(DecParams P) {
    constexpr uint32_t TW = 1u << LMAX, M = TW - 1u;
    __shared__ uint8_t sy[TW];
    const uint64_t gb = blockIdx.x;
    if (gb >= P.n_blocks) return;
    const uint2 bk = reinterpret_cast<const uint2*>(P.bulk)[gb];
    const int32_t info = P.dtinfo[gb];
    const uint64_t ooff = gb * (uint64_t)P.block_size;
    const uint32_t lim = P.n_total ? (uint32_t)min((uint64_t)P.block_size, P.n_total - ooff) : P.out_cap;
    const uint32_t ob = min(bk.x, lim) & ~15u;  // the bulk is whole 16-byte groups
    if (info < 0 || ob == 0) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t nst = 1u << min((uint32_t)info >> 16, (uint32_t)LMAX);
    const uint32_t* dtg = P.dt + gb * (uint64_t)TW;
    for (uint32_t i = tid; i < nst; i += 256u) sy[i] = (uint8_t)dte_sym(dtg[i]);
    __syncthreads();
    const uint32_t h = bk.y;
    auto two = [&](uint32_t w) { return (uint32_t)sy[(w - h) & M] | ((uint32_t)sy[((w >> 16) - h) & M] << 8); };
    const uint4* src = reinterpret_cast<const uint4*>(P.states + ooff / 2u);
    uint4* dst = reinterpret_cast<uint4*>(P.out + ooff);
    const uint32_t ng = ob >> 4;  // 16 output bytes = 8 pairs = 2 x uint4 of states
#pragma unroll 2
    for (uint32_t i = tid; i < ng; i += 256u) {
        const uint4 a = src[2u * i], b = src[2u * i + 1u];
        dst[i] = make_uint4(two(a.x) | (two(a.y) << 16), two(a.z) | (two(a.w) << 16), two(b.x) | (two(b.y) << 16),
                            two(b.z) | (two(b.w) << 16));
    }
}

// ------------------------------------------------------------------------
// launch wrapper
// ------------------------------------------------------------------------
hipError_t launch_decode_serial(const DecParams& P, uint32_t lmax, hipStream_t stream) {
    // the ring kernel: k blocks per workgroup, the decode wave and the loader wave
    auto ring = [&](auto kern, uint32_t k) {
        hipLaunchKernelGGL(kern, dim3((P.n_blocks + k - 1u) / k), dim3(128), 0, stream, P);
    };
    auto go = [&](auto NSc) {
        constexpr int NS = decltype(NSc)::value;
        if (lmax <= 11 && P.states && P.bulk && !P.sidecar_out) {
            // symbols deferred: 8 blocks per workgroup, 32 chains per CU, then the map
            ring(serial_ring_kernel<11, 8, NS, true>, 8);
            hipLaunchKernelGGL((sym_map_kernel<11>), dim3(P.n_blocks), dim3(256), 0, stream, P);
            return;
        }
        with_lmax(lmax, [&](auto Lc) {
            constexpr int L = decltype(Lc)::value;
            // 6 (L <= 11) or 3 (L = 12) blocks per workgroup: 24 / 12 chains per CU (LDS-bound)
            if constexpr (L == 11) ring(serial_ring_kernel<11, 6, NS>, 6);
            else if constexpr (L == 12) ring(serial_ring_kernel<12, 3, NS>, 3);
            else if constexpr (NS == 1) hipLaunchKernelGGL((decode1_serial_kernel<L>), dim3(P.n_blocks), dim3(64), 0, stream, P);
            else hipLaunchKernelGGL((serial2_decode_kernel<L>), dim3(P.n_blocks), dim3(64), 0, stream, P);
        });
    };
    if (P.nstates == 1) go(std::integral_constant<int, 1>{});
    else go(std::integral_constant<int, 2>{});
    return hipGetLastError();
}

int occupancy_lines_serial(char* buf, int len, int cap) {
    len = occupancy_line(buf, len, cap, "serial_ring<11,6,2>", reinterpret_cast<const void*>(serial_ring_kernel<11, 6, 2>),
                         128);
    len = occupancy_line(buf, len, cap, "serial_ring<11,8,2,defer>",
                         reinterpret_cast<const void*>(serial_ring_kernel<11, 8, 2, true>), 128);
    return occupancy_line(buf, len, cap, "sym_map<11>", reinterpret_cast<const void*>(sym_map_kernel<11>));
}

}  // namespace fsehip
