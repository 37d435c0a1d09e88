// fse_shared.hip -- shared-table coding: many small messages against one
// caller's table (fsehip.h section 2c).
//
//   shared_build_kernel   EncodeTable::new + DecodeTable::new (fse.rs:88-189,
//                         269-338) of one NormHistogram into one device image
//                         (one wave, wave_build_spread with checked ranks)
//   shared_encode_kernel  the payload of fse_compress2 (lib.rs:151-182) or of
//                         the headerless 1-state stream (fse.rs:394-421 =
//                         lib.rs:118-142), no header in front
//   shared_decode_kernel  the loops of lib.rs:222-247 / 187-211 over it
//
// The coders run one lane per message with the table once per workgroup in
// LDS (10 KiB encode, 16 KiB decode at L = 12): a short message costs one
// lane's serial chain and no table build, where fsehip_compress_streams spends
// a wave and a build on it.  Lanes of a wave end at different times; messages
// are not sorted.
#include "fse_device.hpp"
#include "fse_kernels.h"

namespace fsehip {

// The image (SHARED_BYTES, 16-byte aligned): header words {valid, table_log,
// table_len, single}, the 256-bit present mask, the symbol transforms, the
// stateTable and the decode table (dte layout: nb | sym << 8 | newState << 18).
constexpr uint32_t SH_VALID = 0x54455346u;  // "FSET": only a build that succeeded writes it
constexpr uint32_t SH_MASK_OFF = 16, SH_TT_OFF = 64, SH_ST_OFF = SH_TT_OFF + 256u * 8u,
                   SH_DT_OFF = SH_ST_OFF + (2u << SHARED_LMAX), SH_BYTES = SH_DT_OFF + (4u << SHARED_LMAX);
static_assert(SH_BYTES == SHARED_BYTES, "image layout");
static_assert(SH_ST_OFF % 16u == 0 && SH_DT_OFF % 16u == 0, "16-byte copies");
constexpr uint32_t SH_THREADS = 256;
constexpr uint32_t SH_MAX_SRC = 65536;  // longer messages belong on fsehip_compress_streams

// Images whose atomic ranks failed their check and were rebuilt with the
// peer-mask ranks (wave_build_spread); per device, reported with the table
// calls' count by fsehip_rank_fallbacks.
__device__ uint32_t g_rank_fb_shared;
hipError_t rank_fallbacks_shared(uint32_t* out, bool reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rank_fb_shared), 4, 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) {
        const uint32_t z = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_rank_fb_shared), &z, 4, 0, hipMemcpyHostToDevice);
    }
    return e;
}

// ------------------------------------------------------------------------
// The build: both tables from one spread.  The ranks come on top of
// cumul[s], the stateTable order (fse.rs:157-162); the decode entry's
// symbol_next is the symbol's count plus the same rank (fse.rs:329-331).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void shared_build_kernel(const fse_norm_histogram* nh, uint8_t* image, int32_t* status,
                                                          uint32_t peer_ranks) {
    constexpr uint32_t SMAX = 1u << SHARED_LMAX;
    __shared__ __attribute__((aligned(16))) uint8_t sym_at[SMAX];
    __shared__ __attribute__((aligned(16))) uint8_t occ[SMAX];
    __shared__ int32_t norm[256];
    __shared__ uint16_t cumul[256];
    __shared__ uint32_t cnt[256];
    const uint32_t lane = lane_id();
    const uint32_t L = nh->log2, tl = nh->table_len;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(image);
    for (uint32_t s = lane; s < 256u; s += WAVE) norm[s] = s < tl ? nh->norm[s] : 0;
    wave_sync();
    int rc = FSE_OK;
    if (L < LOG_MIN || L > LOG_MAX_REF) rc = FSE_ERR_TABLELOG_RANGE;  // TABLE_LOG_RANGE assert (fse.rs:103-106)
    else if (L > SHARED_LMAX) rc = FSE_ERR_UNSUPPORTED;
    else if (tl == 0 || tl > 256u) rc = FSE_ERR_BAD_TABLE;
    const uint32_t size = 1u << (L & 15u);
    uint32_t single = 0;
    if (rc == FSE_OK) {
        // counts are -1 or >= 0 and fill the table exactly
        uint32_t sum = 0, bad = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            const int32_t v = norm[k * WAVE + lane];
            bad |= v < -1 ? 1u : 0u;
            sum += v == -1 ? 1u : v > 0 ? (uint32_t)v : 0u;
            single |= v == (int32_t)size ? 1u : 0u;
            const uint64_t m = __ballot(v != 0);
            if (lane == 0) {
                hdr[SH_MASK_OFF / 4u + 2u * k] = (uint32_t)m;
                hdr[SH_MASK_OFF / 4u + 2u * k + 1u] = (uint32_t)(m >> 32);
            }
        }
        single = wave_max(single);
        if (wave_max(bad) || wave_sum(sum) != size) rc = FSE_ERR_BAD_TABLE;
    }
    if (rc == FSE_OK) {
        uint16_t* st = reinterpret_cast<uint16_t*>(image + SH_ST_OFF);
        uint32_t* dt = reinterpret_cast<uint32_t*>(image + SH_DT_OFF);
        rc = wave_build_spread<64, true>(
            norm, L, tl, sym_at, occ, cumul, cnt,
            [&](uint32_t i, uint32_t s, uint32_t r) {
                st[r] = (uint16_t)(size + i);  // fse.rs:157-162 (r = cumul[s] + rank)
                const int32_t v = norm[s];
                const uint32_t nx = (v < 0 ? 1u : (uint32_t)v) + r - (uint32_t)cumul[s];  // fse.rs:296-308, 329-331
                const uint32_t nb = L - ilog2u(nx);
                dt[i] = nb | (s << 8) | (((nx << nb) - size) << 18);
            },
            [&](uint32_t s) { return (uint32_t)cumul[s]; },
            RankAtomic{peer_ranks == 0u, occ, nullptr, 0u, &g_rank_fb_shared, 0u});
    }
    if (rc == FSE_OK) {
        // symbol transforms (fse.rs:165-188).  A symbol without slots, at or
        // past table_len too, gets the zero-count transform: its bit count
        // comes out as L + 1, which no symbol of the table reaches, and the
        // encoder reads that as "not in the table".
        uint2* tt = reinterpret_cast<uint2*>(image + SH_TT_OFF);
        for (uint32_t s = lane; s < 256u; s += WAVE) {
            const int32_t x = norm[s];
            uint32_t bits = ((L + 1u) << 16) - size;
            int32_t fs = 0;
            if (x == -1 || x == 1) {
                bits = (L << 16) - size;
                fs = (int32_t)cumul[s] - 1;
            } else if (x > 1) {
                const uint32_t mb = L - ilog2u((uint32_t)(x - 1));
                bits = (mb << 16) - ((uint32_t)x << mb);
                fs = (int32_t)cumul[s] - x;
            }
            tt[s] = make_uint2(bits, (uint32_t)fs);
        }
    }
    if (lane == 0) {
        hdr[1] = L;
        hdr[2] = tl;
        hdr[3] = single;
        hdr[0] = rc == FSE_OK ? SH_VALID : 0u;
        *status = rc;
    }
}

// ------------------------------------------------------------------------
// What the two coders share.
// ------------------------------------------------------------------------
// 1..16 bytes of the group {w0, w1, w2, w3} (the ends of a region or message)
__device__ __forceinline__ void store_bytes(uint8_t* p, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t n) {
#pragma unroll
    for (uint32_t b = 0; b < 16u; ++b)
        if (b < n) p[b] = (uint8_t)((b < 4u ? w0 : b < 8u ? w1 : b < 12u ? w2 : w3) >> (8u * (b & 3u)));
}

// The image's header: usable only when a build wrote it (nothing is indexed
// with the contents of any other image).
__device__ __forceinline__ bool shared_image_ok(const uint32_t* hdr, uint32_t* L) {
    *L = hdr[1];
    return hdr[0] == SH_VALID && *L >= LOG_MIN && *L <= SHARED_LMAX;
}

// `bytes` (a multiple of 16) from the image into LDS, by the whole workgroup
__device__ __forceinline__ void stage(void* lds, const uint8_t* g, uint32_t bytes) {
    for (uint32_t i = threadIdx.x; i < bytes / 16u; i += SH_THREADS)
        static_cast<uint4*>(lds)[i] = reinterpret_cast<const uint4*>(g)[i];
}

// ------------------------------------------------------------------------
// Encode.  The lane walks its message backwards: state by the parity of the
// byte's index at two states (lib.rs:151-177: the last two bytes seed the
// states, then index n - 3 down to 0), one state otherwise (lib.rs:118-139).
// Source reads: exactly the message's bytes, 16-byte loads for the aligned
// chunks below the first bytes walked.  Bits go into a 64-bit accumulator and
// leave it as whole dwords, four of them per 16-byte store; nothing is stored
// at or past out_cap.
// ------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(SH_THREADS) void shared_encode_kernel(SharedParams P) {
    __shared__ __attribute__((aligned(16))) uint2 tt[256];
    __shared__ __attribute__((aligned(16))) uint16_t st[1u << SHARED_LMAX];
    __shared__ uint32_t pres[8];
    uint32_t L;
    const bool ok = shared_image_ok(reinterpret_cast<const uint32_t*>(P.table), &L);
    if (ok) {
        stage(tt, P.table + SH_TT_OFF, sizeof tt);
        stage(st, P.table + SH_ST_OFF, 2u << L);
        if (threadIdx.x < 8u) pres[threadIdx.x] = reinterpret_cast<const uint32_t*>(P.table + SH_MASK_OFF)[threadIdx.x];
    }
    __syncthreads();
    const uint32_t msg = blockIdx.x * SH_THREADS + threadIdx.x;
    if (msg >= P.n) return;
    const fsehip_stream_desc d = P.desc[msg];
    const uint32_t n = d.src_len, cap = d.out_cap;
    int32_t err = FSE_OK;
    uint32_t bits = 0;
    if (!ok) err = FSE_ERR_BAD_TABLE;
    else if ((d.src_off | d.out_off) & 15u) err = FSE_ERR_BAD_ARG;
    else if (n == 0) err = FSE_ERR_EMPTY;
    else if (NS == 2 && n == 1) err = FSE_ERR_TOO_SHORT;  // chunks unwrap (lib.rs:154-156)
    else if (n > SH_MAX_SRC) err = FSE_ERR_UNSUPPORTED;
    if (err == FSE_OK) {
        const uint8_t* src = P.in + d.src_off;
        uint8_t* out = P.out + d.out_off;
        const uint32_t smask = (1u << L) - 1u;
        uint64_t acc = 0;
        uint32_t nacc = 0, nd = 0, w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        auto push = [&](uint32_t w) {  // one more dword of the payload
            w0 = w1, w1 = w2, w2 = w3, w3 = w;
            if ((++nd & 3u) == 0) {
                const uint32_t off = 4u * nd - 16u;
                if (off + 16u <= cap) *reinterpret_cast<uint4*>(out + off) = make_uint4(w0, w1, w2, w3);
                else if (off < cap) store_bytes(out + off, w0, w1, w2, w3, cap - off);
            }
        };
        auto put = [&](uint32_t v, uint32_t nb) {  // v < 2^nb
            acc |= (uint64_t)v << nacc;
            nacc += nb;
            if (nacc >= 32u) {
                push((uint32_t)acc);
                acc >>= 32;
                nacc -= 32u;
            }
        };
        bool bad = false;  // a byte the table has no slot for
        auto first = [&](uint32_t s) {  // Encoder::new_first_symbol (fse.rs:210-218)
            bad |= ((pres[s >> 5] >> (s & 31u)) & 1u) == 0;
            const uint2 t = tt[s];
            const uint32_t bo = (t.x + (1u << 15)) >> 16;
            return (uint32_t)st[((((bo << 16) - t.x) >> bo) + t.y) & smask];
        };
        auto step = [&](uint32_t& x, uint32_t s) {  // Encoder::encode (fse.rs:231-238)
            const uint2 t = tt[s];
            const uint32_t bo = (t.x + x) >> 16;
            bad |= bo > L;  // the zero-count transform (shared_build_kernel)
            put(x & ((1u << bo) - 1u), bo);
            x = st[((x >> bo) + t.y) & smask];
        };
        uint32_t x0, x1 = 0;
        int32_t i;
        if (NS == 2) {
            const uint32_t a = first(src[n - 1]), b = first(src[n - 2]);
            x0 = (n & 1u) ? a : b;  // the state of the even indices
            x1 = (n & 1u) ? b : a;
            i = (int32_t)n - 3;
        } else {
            x0 = first(src[n - 1]);
            i = (int32_t)n - 2;
        }
        for (; i >= 0 && ((i + 1) & 15); --i) step((NS == 2 && (i & 1)) ? x1 : x0, src[i]);
        // bytes 0..i: whole chunks, the next one loaded under this one's steps
        const uint4* src4 = reinterpret_cast<const uint4*>(src);
        int32_t c = (i + 1) / 16 - 1;
        uint4 nxt = c >= 0 ? src4[c] : make_uint4(0, 0, 0, 0);
        for (; c >= 0 && !bad; --c) {
            const uint32_t w[4] = {nxt.x, nxt.y, nxt.z, nxt.w};
            if (c > 0) nxt = src4[c - 1];
#pragma unroll
            for (int j = 15; j >= 0; --j) step((NS == 2 && (j & 1)) ? x1 : x0, (w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        }
        if (bad) {
            err = FSE_ERR_SYMBOL_NOT_IN_TABLE;
        } else {
            if (NS == 2) put(x1 & smask, L);  // Encoder::finish (lib.rs:178-179 / 140)
            put(x0 & smask, L);
            put(1u, 1u);  // the marker
            bits = 32u * nd + nacc;
            const uint32_t clen = (bits + 7u) >> 3;
            if (nacc) push((uint32_t)acc);
            if (const uint32_t k = nd & 3u) {  // the last, partial group
                for (uint32_t r = k; r < 4u; ++r) w0 = w1, w1 = w2, w2 = w3, w3 = 0;
                const uint32_t off = 4u * (nd - k), end = min(clen, cap);
                if (off < end) store_bytes(out + off, w0, w1, w2, w3, end - off);
            }
            if (clen > cap) err = FSE_ERR_DST_TOO_SMALL;
        }
    }
    P.status[msg] = err;
    P.len[msg] = err ? 0u : (bits + 7u) >> 3;
    if (P.bits) P.bits[msg] = err ? 0u : bits;
}

// ------------------------------------------------------------------------
// Decode.  The lane reads its payload from the end: the last partial dword
// bytewise, then whole dwords downwards, never below the payload's first
// byte.  `acc` holds the unread bits that have been loaded in its low `nb`
// bits, the next to be read on top; after every read it is refilled, so
// nb >= 32 or no dword is left and "nb >= k" is the reader's "k bits remain"
// (stack_reader.rs:176-215).  Output: 16-byte groups, the last one bytewise.
// The end rules are the serial decoders' (fse_decode_serial.hip, known / lim), but
// that with a known length at two states the payload must end there too: the
// block decoders stop at the raw length whatever follows.
// ------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(SH_THREADS) void shared_decode_kernel(SharedParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t dt[1u << SHARED_LMAX];
    uint32_t L;
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(P.table);
    const bool ok = shared_image_ok(hdr, &L);
    if (ok) stage(dt, P.table + SH_DT_OFF, 4u << L);
    __syncthreads();
    const uint32_t msg = blockIdx.x * SH_THREADS + threadIdx.x;
    if (msg >= P.n) return;
    const fsehip_stream_desc d = P.desc[msg];
    const uint32_t n = d.src_len;
    const bool known = P.raw_len != nullptr;
    const uint32_t lim = known ? P.raw_len[msg] : d.out_cap;  // bytes the message may produce
    const bool single = ok && hdr[3] != 0u;
    const uint8_t* in = P.in + d.src_off;
    uint8_t* out = P.out + d.out_off;
    int32_t err = FSE_OK;
    uint32_t last = 0;
    if (!ok) err = FSE_ERR_BAD_TABLE;
    else if ((d.src_off | d.out_off) & 15u) err = FSE_ERR_BAD_ARG;
    else if (n == 0) err = FSE_ERR_EMPTY;  // BitStackReader::new of an empty slice is None as well; as the block decoders
    else if ((last = in[n - 1]) == 0) err = FSE_ERR_NO_MARKER;  // stack_reader.rs:77-83
    else if (lim > d.out_cap) err = FSE_ERR_DST_TOO_SMALL;  // a known length the region cannot hold
    else if (NS == 2 && known && lim < 2u) err = FSE_ERR_LENGTH_MISMATCH;
    else if (!known && single) err = FSE_ERR_SINGLE_SYMBOL;  // the reference never ends such a stream
    uint32_t o = 0;
    if (err == FSE_OK) {
        const uint32_t* in4 = reinterpret_cast<const uint32_t*>(in);
        uint32_t nd = n >> 2, nb;
        uint64_t acc = 0;
        if (const uint32_t t = n & 3u) {
            for (uint32_t k = 0; k < t; ++k) acc |= (uint64_t)in[4u * nd + k] << (8u * k);
            nb = 8u * (t - 1u) + ilog2u(last);
        } else {
            acc = in4[--nd];
            nb = 24u + ilog2u(last);
        }
        auto refill = [&]() {
            if (nb < 32u && nd) {
                acc = (acc << 32) | in4[--nd];
                nb += 32u;
            }
        };
        auto pop = [&](uint32_t k) {  // k <= nb
            nb -= k;
            const uint32_t v = (uint32_t)(acc >> nb) & ((1u << k) - 1u);
            refill();
            return v;
        };
        refill();
        uint32_t cur = 0, w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        auto emit = [&](uint32_t y) {  // o < lim
            cur |= y << (8u * (o & 3u));
            if ((++o & 3u) == 0) {
                w0 = w1, w1 = w2, w2 = w3, w3 = cur, cur = 0;
                if ((o & 15u) == 0) *reinterpret_cast<uint4*>(out + o - 16u) = make_uint4(w0, w1, w2, w3);
            }
        };
        auto sym = [](uint32_t e) { return (e >> 8) & 0xFFu; };
        uint32_t s0 = 0, s1 = 0;
        if (nb < NS * L) {
            err = FSE_ERR_TOO_SHORT;  // the state reads' unwrap (lib.rs:197 / 224-225)
        } else {
            s0 = pop(L);
            if (NS == 2) s1 = pop(L);
        }
        if (err != FSE_OK) {
        } else if (NS == 2) {
            // pair by pair with the reference's end checks (lib.rs:227-244)
            const int32_t full = known ? FSE_ERR_LENGTH_MISMATCH : FSE_ERR_DST_TOO_SMALL;
            uint32_t nb1 = 0;  // bits of decoder 1's last read
            for (;;) {
                if (known && o + 2u >= lim) {
                    // The raw length ends the message (o is even here) -- if
                    // the payload ends too: no bit is left, and where one byte
                    // is missing decoder 1's last read took none (an odd
                    // length ends by a failed read, lib.rs:235-239, unless
                    // that read needs no bit; one that took bits undid a step
                    // of the encoder, so the message is longer).
                    if (nb != 0u || (o + 2u != lim && nb1 != 0u)) { err = FSE_ERR_LENGTH_MISMATCH; break; }
                    emit(sym(dt[s0]));
                    if (o < lim) emit(sym(dt[s1]));
                    break;
                }
                const uint32_t e0 = dt[s0];
                if (nb < (e0 & 0xFFu)) {  // decoder 0 cannot read: lib.rs:242-243
                    if (o + 2u > lim) { err = full; break; }
                    emit(sym(e0));
                    emit(sym(dt[s1]));
                    break;
                }
                s0 = (e0 >> 18) + pop(e0 & 0xFFu);
                if (o >= lim) { err = full; break; }
                emit(sym(e0));
                const uint32_t e1 = dt[s1];
                if (nb < (e1 & 0xFFu)) {  // decoder 1 cannot read: lib.rs:235-239
                    if (o + 2u > lim) { err = full; break; }
                    emit(sym(e1));
                    emit(sym(dt[s0]));
                    break;
                }
                nb1 = e1 & 0xFFu;
                s1 = (e1 >> 18) + pop(nb1);
                if (o >= lim) { err = full; break; }
                emit(sym(e1));
            }
            if (err == FSE_OK && known && o != lim) err = FSE_ERR_LENGTH_MISMATCH;
        } else {
            // symbol by symbol (lib.rs:198-208), then Decoder::finish; a
            // single-symbol table never fails a read and ends by its length
            for (;;) {
                if (known && single && o + 1u >= lim) break;
                const uint32_t e = dt[s0];
                if (nb < (e & 0xFFu)) break;  // decode_symbol -> None
                if (o >= lim) { err = FSE_ERR_DST_TOO_SMALL; break; }
                s0 = (e >> 18) + pop(e & 0xFFu);
                emit(sym(e));
            }
            if (err == FSE_OK) {
                if (o >= lim) err = FSE_ERR_DST_TOO_SMALL;
                else emit(sym(dt[s0]));  // Decoder::finish (lib.rs:208)
            }
            if (known && (err == FSE_ERR_DST_TOO_SMALL || (err == FSE_OK && o != lim))) err = FSE_ERR_LENGTH_MISMATCH;
        }
        if (const uint32_t r = o & 15u) {  // the last, partial group
            uint32_t k = r >> 2;
            if (r & 3u) w0 = w1, w1 = w2, w2 = w3, w3 = cur, ++k;
            for (; k < 4u; ++k) w0 = w1, w1 = w2, w2 = w3, w3 = 0;
            store_bytes(out + (o & ~15u), w0, w1, w2, w3, r);
        }
    }
    P.status[msg] = err;
    P.len[msg] = err ? 0u : o;
}

// ------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------
hipError_t launch_shared_build(const fse_norm_histogram* nh, uint8_t* image, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(shared_build_kernel, dim3(1), dim3(64), 0, s, nh, image, status, atomic_ranks_on() ? 0u : 1u);
    return hipGetLastError();
}

hipError_t launch_shared_encode(const SharedParams& P, hipStream_t s) {
    const dim3 grid((P.n + SH_THREADS - 1u) / SH_THREADS);
    if (P.nstates == 1) hipLaunchKernelGGL(shared_encode_kernel<1>, grid, dim3(SH_THREADS), 0, s, P);
    else hipLaunchKernelGGL(shared_encode_kernel<2>, grid, dim3(SH_THREADS), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_shared_decode(const SharedParams& P, hipStream_t s) {
    const dim3 grid((P.n + SH_THREADS - 1u) / SH_THREADS);
    if (P.nstates == 1) hipLaunchKernelGGL(shared_decode_kernel<1>, grid, dim3(SH_THREADS), 0, s, P);
    else hipLaunchKernelGGL(shared_decode_kernel<2>, grid, dim3(SH_THREADS), 0, s, P);
    return hipGetLastError();
}

}  // namespace fsehip
