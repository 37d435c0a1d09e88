// fse_decode_single.hip -- one stream, latency first, gfx950: the host
// fse_decompress2 / fse_decompress in the reference's own termination, table
// logs <= 11, on a prebuilt table (fse_decode_tables.hip).
//
//   single_ftab_kernel    the stream's u32 table fused into 64-bit entries
//                         shaped for the scalar unit (into DecParams::states)
//   single_decode_kernel  one wave per stream, 2-state or 1-state: the chain
//                         runs on the scalar unit with hand-issued scalar
//                         loads of the fused entries (fent_issue* / fent_wait*
//                         / fstep; tests/test_isa_single_decode.py checks the
//                         register allocation around them)
#include <type_traits>
#include <utility>

#include "fse_decode_dev.hpp"
#include "fse_kernels.h"

namespace fsehip {

// ------------------------------------------------------------------------
// One stream, as fast as one serial chain goes: the host fse_decompress2 /
// fse_decompress (lib.rs:187-248) in the reference's own termination.  A
// lone 2-state stream is a single dependency chain (no
// speculative split), so this kernel minimises the latency of one step
// instead of running many chains per CU:
//   - one wave; the chain is wave-uniform, so it runs on the scalar unit
//     (SGPRs) and never waits on a VGPR round trip;
//   - the bulk reads the table through the scalar cache: fused 64-bit
//     entries (single_ftab_kernel) whose low word is at once the s_bfe_u64
//     operand of the state's bits and the window update, both entries of a
//     pair loaded at an SGPR byte offset and awaited together;
//   - the payload is read from global memory 64 words at a time (one per
//     lane), the next chunk in flight while the current one is consumed; the
//     64-bit window refills from a word taken (v_readlane) one refill ahead,
//     so neither an LDS nor a memory latency is on the chain, and there is no
//     staging phase and no size limit;
//   - the bulk runs 32 pairs (64 symbols) between end checks; each step's
//     entry is parked in a VGPR lane (v_writelane at a constant lane) while
//     the next pair's loads are in flight, and the 64 lanes then store their
//     symbols at once;
//   - the checked tail and the single-symbol test read the table from VGPRs
//     (32 registers: entry s is lane s & 63 of register s >> 6).
// Measured per 64 KiB call (tools/host_latency.py): 3.0-3.6 ms with the
// table in VGPRs (a dependent v_readlane lookup, ~41 cycles) and the payload
// staged in LDS; 2.8 ms with plain scalar loads of the u32 entries; 2.1 ms
// with the fused entries (profiles/r04/single_stream/).
// ------------------------------------------------------------------------

// The table in registers: entry of state s (wave-uniform s)
template <uint32_t NV>
__device__ __forceinline__ uint32_t vtab_at(const uint32_t (&vt)[NV], uint32_t s) {
    return (uint32_t)__builtin_amdgcn_readlane((int)vt[(s >> 6) & (NV - 1u)], (int)(s & 63u));
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <class F, int... I>
__device__ __forceinline__ void unroll_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void unroll(F&& f) {
    unroll_impl(f, std::make_integer_sequence<int, N>{});
}
// v = lane J of `buf` (a constant lane: no index register)
template <int J>
__device__ __forceinline__ void park(uint32_t& buf, uint32_t v) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(buf) : "s"(v), "i"(J));
}
// lanes J and J + 1 (one asm block: no wait state between the two)
template <int J>
__device__ __forceinline__ void park2(uint32_t& buf, uint32_t a, uint32_t b) {
    asm volatile(
        "v_writelane_b32 %0, %1, %3\n\t"
        "v_writelane_b32 %0, %2, %4"
        : "+v"(buf)
        : "s"(a), "s"(b), "i"(J), "i"(J + 1));
}

// Fused entry of one state, shaped for the scalar unit:
//   lo = nb * 0xFFFF | sym << 24, hi = new_state * 8 (the byte offset of the
//   next entry before its bits: offset = bits * 8 + hi, one s_lshl3_add).
// With `av` the window bits below pos, op = av + lo = (nb << 16) | (av - nb)
// (av >= nb) is at once the s_bfe_u64 operand of the state's bits (offset
// av - nb, width nb; bits 23.. are ignored) and, masked to 16 bits, the new
// av.  Built per call into DecParams::states (2 words per entry).
__global__ __launch_bounds__(256) void single_ftab_kernel(const uint32_t* __restrict__ dt, uint32_t* __restrict__ ft,
                                                           uint32_t tw) {
    dt += (uint64_t)blockIdx.x * tw;  // one workgroup per stream
    ft += (uint64_t)blockIdx.x * 2u * tw;
    for (uint32_t i = threadIdx.x; i < tw; i += blockDim.x) {
        const uint32_t e = dt[i];
        ft[2u * i] = dte_nb(e) * 0xFFFFu | dte_sym(e) << 24;
        ft[2u * i + 1u] = Dte<11>::ns(e) << 3;
    }
}
// One fused step's next offset: bfe(W, op) * 8 + hi (W >> (op & 63) masked
// to (op >> 16) & 127 bits), as two scalar instructions in one asm block
// (the bits go through a fixed register pair: separate asm statements get a
// wait state between them, and the compiler emits a shift and an add for
// the second).  s_bfe and s_lshl3_add write SCC.
__device__ __forceinline__ uint32_t fstep(uint64_t W, uint32_t op, uint32_t hi) {
    uint32_t r;
    asm("s_bfe_u64 s[98:99], %1, %2\n\t"
        "s_lshl3_add_u32 %0, s98, %3"
        : "=s"(r)
        : "s"(W), "s"(op), "s"(hi)
        : "s98", "s99", "scc");
    return r;
}
// The bulk's software pipeline: a step computes its pair's next offsets,
// issues the scalar loads of those entries (fent_issue*: SGPR byte offsets
// into ft, no 64-bit address arithmetic) and parks its own entries in VGPR
// lanes in the same asm block, then refills the window while the loads are
// in flight; the next step starts with fent_wait*.  The compiler does not
// track these loads: the registers they write stay live until the wait that
// names them (so nothing else is put there meanwhile), and `av` is tied to
// the issue and `W`, `av` to the wait so that the refill stays between them.
template <int J>
__device__ __forceinline__ void fent_issue2(uint64_t ft, uint32_t o0, uint32_t o1, uint64_t& f0, uint64_t& f1,
                                            uint32_t& buf, uint32_t a, uint32_t b, uint32_t& av) {
    asm volatile(
        "s_load_dwordx2 %0, %4, %5\n\t"
        "s_load_dwordx2 %1, %4, %6\n\t"
        "v_writelane_b32 %2, %7, %9\n\t"
        "v_writelane_b32 %2, %8, %10"
        : "=&s"(f0), "=&s"(f1), "+v"(buf), "+s"(av)
        : "s"(ft), "s"(o0), "s"(o1), "s"(a), "s"(b), "i"(J), "i"(J + 1));
}
__device__ __forceinline__ void fent_issue2n(uint64_t ft, uint32_t o0, uint32_t o1, uint64_t& f0, uint64_t& f1,
                                             uint32_t& av) {  // no entries to park (the bulk's first pair)
    asm volatile(
        "s_load_dwordx2 %0, %3, %4\n\t"
        "s_load_dwordx2 %1, %3, %5"
        : "=&s"(f0), "=&s"(f1), "+s"(av)
        : "s"(ft), "s"(o0), "s"(o1));
}
__device__ __forceinline__ void fent_wait2(uint64_t& f0, uint64_t& f1, uint64_t& W, uint32_t& av) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(f0), "+s"(f1), "+s"(W), "+s"(av));
}
template <int J>
__device__ __forceinline__ void fent_issue1(uint64_t ft, uint32_t o, uint64_t& f, uint32_t& buf, uint32_t a,
                                            uint32_t& av) {
    asm volatile(
        "s_load_dwordx2 %0, %3, %4\n\t"
        "v_writelane_b32 %1, %5, %6"
        : "=&s"(f), "+v"(buf), "+s"(av)
        : "s"(ft), "s"(o), "s"(a), "i"(J));
}
__device__ __forceinline__ void fent_issue1n(uint64_t ft, uint32_t o, uint64_t& f, uint32_t& av) {
    asm volatile("s_load_dwordx2 %0, %2, %3" : "=&s"(f), "+s"(av) : "s"(ft), "s"(o));
}
__device__ __forceinline__ void fent_wait1(uint64_t& f, uint64_t& W, uint32_t& av) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(f), "+s"(W), "+s"(av));
}

template <int NS>
__global__ __launch_bounds__(64) void single_decode_kernel(DecParams P) {
    constexpr uint32_t LMAX = 11, TW = 1u << LMAX, NV = TW / 64u;
    const uint32_t lane = threadIdx.x;
    // one wave per stream: stream gb at P.in + gb * slot_bytes, its table at
    // P.dt + gb * 2^11 words, fused at P.states + gb * 2^12 words, its output
    // at P.out + gb * block_size
    const uint64_t gb = blockIdx.x;
    if (gb >= P.n_blocks) return;
    const int32_t info = P.dtinfo[gb];
    const uint32_t clen = P.comp_len[gb];
    int32_t err = info < 0 ? info : FSE_OK;
    const uint32_t L = err == FSE_OK ? (uint32_t)info >> 16 : 0u;
    // table into VGPRs; OR of the valid entries' nb: 0 = single-symbol table
    uint32_t vt[NV];
    uint32_t nbor = 0;
    {
        const uint32_t size = 1u << L;
#pragma unroll
        for (uint32_t k = 0; k < NV; ++k) {
            vt[k] = P.dt[gb * TW + k * 64u + lane];
            if (k * 64u + lane < size) nbor |= vt[k] & 0xFFu;
        }
    }
    const bool single = __ballot(nbor != 0u) == 0ull;
    uint8_t* out = P.out + gb * P.block_size;
    const uint32_t cap = P.out_cap;
    if (err == FSE_OK && single) err = FSE_ERR_SINGLE_SYMBOL;  // the reference never ends such a stream
    if (err != FSE_OK) {
        if (lane == 0) {
            P.status[gb] = err;
            if (P.out_len) P.out_len[gb] = 0;
        }
        return;
    }
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(P.in + gb * P.slot_bytes);
    const int32_t last = (int32_t)((clen - 1u) >> 2);  // the payload's last word
    // 64 payload words from word c on, one per lane.  Words below word 0 are
    // never consumed (bits below the header are not read), so the index is
    // only clamped into the buffer: an unconditional load straight into its
    // register, awaited only when the chunk is used.
    auto chunk = [&](int32_t c) -> uint32_t { return in32[min(max(c + (int32_t)lane, 0), last)]; };
    const int32_t hdr_bits = (info & 0xFFFF) * 8;
    const uint32_t lastw = (uint32_t)__builtin_amdgcn_readfirstlane((int)in32[last]);
    const uint32_t lastb = (lastw >> (8u * ((clen - 1u) & 3u))) & 0xFFu;  // non-zero: checked by the table build
    const int32_t pos0 = (int32_t)(clen - 1u) * 8 + (int32_t)(31u - (uint32_t)__builtin_clz(lastb));  // the marker
    // window W: bits [base, base + 64) of the stream, base = 32 * (cb + li + 1);
    // av = pos - base bits below pos.  cur holds words [cb, cb + 64), pre the
    // 64 below (in flight); nxt = word cb + li, the next one into the window.
    const int32_t wb = (((pos0 + 31) & ~31) - 64) >> 5;  // the window's low word (>= -2)
    int32_t cb = wb + 1 - 63;
    uint32_t cur = chunk(cb);
    uint32_t pre = chunk(cb - 64);
    int32_t li = wb - 1 - cb;
    auto lane_word = [&](int32_t l) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)cur, l); };
    uint64_t W = (uint64_t)lane_word(wb - cb) | ((uint64_t)lane_word(wb + 1 - cb) << 32);
    uint32_t nxt = lane_word(li);
    uint32_t av = (uint32_t)(pos0 - 32 * wb);
    auto bitpos = [&]() -> int32_t { return 32 * (cb + li + 1) + (int32_t)av; };
    auto shift_in = [&]() {  // one word into the window (av < 32 before)
        W = (W << 32) | nxt;
        av += 32u;
        if (li == 0) {  // the chunk below becomes current; the next one is requested
            // the copy first, then the load into the register pre frees (a load
            // into a temporary would be copied, and awaited, at once)
            asm volatile("v_mov_b32 %0, %1" : "=&v"(cur) : "v"(pre) : "memory");
            cb -= 64;
            pre = chunk(cb - 64);
            li = 64;
        }
        --li;
        nxt = lane_word(li);
    };
    auto refill = [&]() {  // keep >= 32 bits below pos in the window
        if (av < 32u) shift_in();
    };
    auto pop = [&](uint32_t nb) -> uint32_t {
        av -= nb;
        return (uint32_t)(W >> av) & ((1u << nb) - 1u);
    };
    const uint64_t ft = (uint64_t)(P.states + gb * 2u * TW);
    uint32_t o = 0;  // bytes decoded
    uint32_t eb = 0;  // the round's 64 entries, one per lane
    auto put64 = [&]() {  // the round's symbols (fused entries: sym in bits 24..31)
        out[o + lane] = (uint8_t)(eb >> 24);
        o += 64u;
    };
    auto put1 = [&](uint32_t sym) {  // one byte (the checked tail)
        if (lane == 0) out[o] = (uint8_t)sym;
        ++o;
    };
    const int32_t full = FSE_ERR_DST_TOO_SMALL;
    if (NS == 2) {
        if (bitpos() - 2 * (int32_t)L < hdr_bits) {
            err = FSE_ERR_TOO_SHORT;  // lib.rs:224-225 unwrap
        } else {
            uint32_t s0 = pop(L);
            refill();
            uint32_t s1 = pop(L);
            refill();
            // bulk: rounds of 32 pairs that can neither run out of bits (<= 2L
            // a pair) nor reach the capacity: no end checks
            for (;;) {
                const uint32_t by_bits = (uint32_t)(bitpos() - hdr_bits) / (64u * L);
                const uint32_t by_cap = cap > o + 66u ? (cap - o - 2u) / 64u : 0u;
                uint32_t g = min(by_bits, by_cap);
                if (g == 0u) break;
                uint32_t x0 = s0 << 3, x1 = s1 << 3;  // the states as byte offsets into ft
                uint64_t fa0, fa1, fb0, fb1;  // entries of even / odd steps
                fent_issue2n(ft, x0, x1, fa0, fa1, av);
                for (; g; --g) {
                    auto step = [&](auto J) {
                        constexpr int j = decltype(J)::value;
                        uint64_t& c0 = (j & 1) ? fb0 : fa0;
                        uint64_t& c1 = (j & 1) ? fb1 : fa1;
                        uint64_t& n0 = (j & 1) ? fa0 : fb0;
                        uint64_t& n1 = (j & 1) ? fa1 : fb1;
                        fent_wait2(c0, c1, W, av);
                        uint32_t op = av + (uint32_t)c0;
                        x0 = fstep(W, op, (uint32_t)(c0 >> 32));
                        op = (op & 0xFFFFu) + (uint32_t)c1;
                        x1 = fstep(W, op, (uint32_t)(c1 >> 32));
                        av = op & 0xFFFFu;
                        fent_issue2<2 * j>(ft, x0, x1, n0, n1, eb, (uint32_t)c0, (uint32_t)c1, av);
                        refill();  // a pair takes <= 2L = 22 bits, a refill leaves >= 32
                    };
                    unroll<32>(step);
                    put64();
                }
                fent_wait2(fa0, fa1, W, av);  // the loads issued after the last pair
                s0 = x0 >> 3;
                s1 = x1 >> 3;
            }
            // tail: pair by pair with the reference's end checks (lib.rs:227-243)
            for (;;) {
                const uint32_t e0 = vtab_at(vt, s0);
                uint32_t nb = dte_nb(e0);
                if (bitpos() - (int32_t)nb < hdr_bits) {  // decoder 0 cannot read
                    if (o + 2u > cap) { err = full; break; }
                    put1(dte_sym(e0));
                    put1(dte_sym(vtab_at(vt, s1)));
                    break;
                }
                s0 = Dte<LMAX>::ns(e0) + pop(nb);
                refill();
                if (o >= cap) { err = full; break; }
                put1(dte_sym(e0));
                const uint32_t e1 = vtab_at(vt, s1);
                nb = dte_nb(e1);
                if (bitpos() - (int32_t)nb < hdr_bits) {  // decoder 1 cannot read
                    if (o + 2u > cap) { err = full; break; }
                    put1(dte_sym(e1));
                    put1(dte_sym(vtab_at(vt, s0)));
                    break;
                }
                s1 = Dte<LMAX>::ns(e1) + pop(nb);
                refill();
                if (o >= cap) { err = full; break; }
                put1(dte_sym(e1));
            }
        }
    } else {
        if (bitpos() - (int32_t)L < hdr_bits) {
            err = FSE_ERR_TOO_SHORT;  // lib.rs:197 unwrap
        } else {
            uint32_t s = pop(L);
            refill();
            for (;;) {  // bulk: rounds of 64 symbols, no end checks
                const uint32_t by_bits = (uint32_t)(bitpos() - hdr_bits) / (64u * L);
                const uint32_t by_cap = cap > o + 65u ? (cap - o - 1u) / 64u : 0u;
                uint32_t g = min(by_bits, by_cap);
                if (g == 0u) break;
                uint32_t x = s << 3;
                uint64_t fa, fb;  // entries of even / odd steps
                fent_issue1n(ft, x, fa, av);
                for (; g; --g) {
                    auto step = [&](auto J) {
                        constexpr int j = decltype(J)::value;
                        uint64_t& c = (j & 1) ? fb : fa;
                        uint64_t& nx = (j & 1) ? fa : fb;
                        fent_wait1(c, W, av);
                        const uint32_t op = av + (uint32_t)c;
                        x = fstep(W, op, (uint32_t)(c >> 32));
                        av = op & 0xFFFFu;
                        fent_issue1<j>(ft, x, nx, eb, (uint32_t)c, av);
                        if (j & 1) refill();  // two symbols take <= 2L = 22 bits
                    };
                    unroll<64>(step);
                    put64();
                }
                fent_wait1(fa, W, av);
                s = x >> 3;
            }
            for (;;) {  // lib.rs:198-207 with the read check, then finish (208)
                const uint32_t e = vtab_at(vt, s);
                const uint32_t nb = dte_nb(e);
                if (bitpos() - (int32_t)nb < hdr_bits) break;
                if (o >= cap) { err = full; break; }
                s = Dte<LMAX>::ns(e) + pop(nb);
                refill();
                put1(dte_sym(e));
            }
            if (err == FSE_OK) {
                if (o >= cap) err = full;
                else put1(dte_sym(vtab_at(vt, s)));
            }
        }
    }
    if (lane == 0) {
        P.status[gb] = err;
        if (P.out_len) P.out_len[gb] = err ? 0u : o;
    }
}

// P.n_blocks streams, one wave each (P.states: 2^12 words of fused table per stream)
hipError_t launch_single(const DecParams& P, uint32_t lmax, hipStream_t stream) {
    if (!P.dt || !P.dtinfo || !P.states || P.n_total || P.sidecar || P.sidecar_out || P.n_blocks == 0 || lmax > 11)
        return hipErrorInvalidValue;
    const dim3 g(P.n_blocks);
    hipLaunchKernelGGL(single_ftab_kernel, g, dim3(256), 0, stream, P.dt, P.states, 2048u);
    if (P.nstates == 1) hipLaunchKernelGGL((single_decode_kernel<1>), g, dim3(64), 0, stream, P);
    else hipLaunchKernelGGL((single_decode_kernel<2>), g, dim3(64), 0, stream, P);
    return hipGetLastError();
}

}  // namespace fsehip
