// fse_decode_tables.hip -- header parse and decode tables for a batch of
// blocks, gfx950: the first step of every block decode (launch_dtables).
//
//   hdr_parse_kernel      NormHistogram::read (histogram.rs:436-505), one lane
//                         per block over headers staged in LDS rows (L <= 12,
//                         with the optional scratch), counts to the scratch
//   dtable_blocks_kernel  DecodeTable (fse.rs:280-338), one wave per block,
//                         from those counts or its own scalar-unit parse;
//                         the table goes to HBM in the decoders' entry layout
//                         (Dte, fse_decode_dev.hpp)
//
// Kernels are instantiated at LMAX = 11, 12, 13, 14 and 15 (the table's
// stride in HBM is 4 << LMAX bytes per block).
#include "fse_decode_dev.hpp"
#include "fse_decode_host.h"

namespace fsehip {

// Tables of this file's kernels whose atomic ranks failed their check and
// were rebuilt with the peer-mask ranks (wave_build_spread); per device.
__device__ uint32_t g_rank_fb_dec;
hipError_t rank_fallbacks_dec(uint32_t* out, bool reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rank_fb_dec), 4, 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) {
        const uint32_t z = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_rank_fb_dec), &z, 4, 0, hipMemcpyHostToDevice);
    }
    return e;
}

// ------------------------------------------------------------------------
// NormHistogram::read (histogram.rs:436-505) for 16 blocks per wave, one lane
// per block.  Parsed on the scalar unit inside dtable_blocks_kernel a header
// costs ~2,200 scalar instructions, and at full occupancy the CU's one scalar
// unit is shared by all its waves (the parse took 29.8K of the kernel's 68.4K
// cycles per block, profiles/r04/probe1/stamps_T64.log).  Here the headers
// are staged into LDS rows (the same 512 bytes the wave parse holds, coalesced
// per block, 16 blocks' loads in flight at once) and each lane runs the same
// parse (header_read_core) on its own row; the counts and the header length /
// L / table_len go to the scratch that dtable_blocks_kernel then reads.
// ------------------------------------------------------------------------
constexpr uint32_t HP_BLOCKS = 16;  // headers per workgroup: 1,024 workgroups at C2 (8 measured no faster: the parse latency is the floor)
template <int LMAX>
__global__ __launch_bounds__(64) void hdr_parse_kernel(DtParams P) {
    static_assert(LMAX <= 12, "headers of L <= 12 fit the 512 staged bytes");
    constexpr uint32_t NB = HP_BLOCKS;
    // block j's header words and counts, rotated by j words (row j, word i at
    // (i + j) % 128): lanes at the same word index hit different banks
    __shared__ uint32_t rows[NB][128];
    __shared__ uint32_t nrm[NB][128];  // 256 x int16 per block
    const uint32_t lane = threadIdx.x;
    const uint64_t gb0 = (uint64_t)blockIdx.x * NB;
    const uint64_t gl = gb0 + lane;
    const bool mine = lane < NB && gl < P.n_blocks;
    const uint32_t clen_l = mine ? P.comp_len[gl] : 0u;
    // the words header_read_wave holds: min(clen, 512) bytes, within the slot
    const uint32_t nw_l = (uint32_t)min((uint64_t)min(clen_l, HDR_MAX) + 3u, P.slot_bytes) >> 2;
    for (uint32_t i = lane; i < NB * 128u; i += 64u) (&nrm[0][0])[i] = 0u;
    // stage: block j's words across the lanes, every block's loads in flight at once
    uint32_t a[NB], b[NB];
#pragma unroll
    for (uint32_t j = 0; j < NB; ++j) {
        const uint32_t nw = (uint32_t)__builtin_amdgcn_readlane((int)nw_l, (int)j);  // 0 past the batch
        const uint32_t* w = reinterpret_cast<const uint32_t*>(P.in + (gb0 + j) * P.slot_bytes);
        a[j] = lane < nw ? w[lane] : 0u;
        b[j] = lane + 64u < nw ? w[lane + 64u] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < NB; ++j) {
        rows[j][(lane + j) & 127u] = a[j];
        rows[j][(lane + 64u + j) & 127u] = b[j];
    }
    __syncthreads();
    if (mine) {
        uint32_t L = 0, tl = 0;
        typedef __attribute__((address_space(3))) int16_t lds_i16;
        const int hl = header_read_row((const lds_u32*)&rows[lane][0], lane, nw_l, clen_l, (uint32_t)LMAX,
                                       (lds_i16*)&nrm[lane][0], &L, &tl);
        P.hdr_meta[gl] = make_int2(hl, (int)(L | (tl << 8)));
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < NB; ++j) {  // counts out, unrotated: word k of block j
        const uint64_t g = gb0 + j;
        if (g >= P.n_blocks) break;
        P.hdr_norm[g * 128u + lane] = nrm[j][(lane + j) & 127u];
        P.hdr_norm[g * 128u + 64u + lane] = nrm[j][(lane + 64u + j) & 127u];
    }
}

// ------------------------------------------------------------------------
// Decode tables for a batch of blocks (C3's "pre-built dtables"; also the
// first kernel of the two-kernel decode): NormHistogram::read on the scalar
// unit + DecodeTable (fse.rs:280-338) by one wave per block, written to HBM
// in the decoder's entry layout.  Small LDS footprint at L <= 12, so many
// blocks are in flight per CU and the serial header parse is overlapped
// across blocks.
// ------------------------------------------------------------------------
template <int LMAX>
__global__ __launch_bounds__(64) void dtable_blocks_kernel(DtParams P) {
    constexpr uint32_t SIZE = 1u << LMAX;
    __shared__ int32_t norm[256];
    __shared__ __attribute__((aligned(16))) uint8_t sym_at[SIZE];
    // the two-pass rank table (2^L u16) reuses the occurrence owners, the
    // counters and cumul: all three are dead once the spread walk is done
    // (the decoder's visit reads norm only); 7 KB per workgroup at L = 11.
    // L >= 13 never takes the two-pass ranks, so the array only has to hold
    // occ, cnt and cumul: 2^L + 1.5 KiB instead of 2^(L+1) bytes (L = 15: 2
    // workgroups per CU instead of 1)
    constexpr uint32_t RKN = LMAX <= 12 ? SIZE : SIZE / 2u + 768u;
    __shared__ __attribute__((aligned(16))) uint16_t rk[RKN];
    static_assert(SIZE + 256 * 4 + 256 * 2 <= RKN * 2, "rank table must cover occ, cnt and cumul");
    // (no LDS peer masks: the peer-mask ranks run only when an atomic-rank
    // table fails its check, and then match keys by ballot; the 512 B they
    // took kept the kernel at 21 workgroups per CU instead of 22)
    uint8_t* occ = reinterpret_cast<uint8_t*>(rk);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(rk) + SIZE);
    uint16_t* cumul = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(rk) + SIZE + 1024);
    const uint32_t lane = lane_id();
    const uint64_t gb = blockIdx.x;
    if (gb >= P.n_blocks) return;
    FSE_STAMP(P, 0);
    const uint8_t* in = P.in + gb * P.slot_bytes;
    const uint32_t clen = P.comp_len[gb];
    const uint32_t last = (clen && clen <= P.slot_bytes) ? in[clen - 1u] : 0u;
    uint32_t L = 0, tl = 0;
    int hl;
    if (LMAX <= 12 && P.hdr_meta) {  // parsed by hdr_parse_kernel: counts from the scratch
        const int2 m = P.hdr_meta[gb];
        const uint32_t q0 = P.hdr_norm[gb * 128u + lane], q1 = P.hdr_norm[gb * 128u + 64u + lane];
        norm[2u * lane] = (int32_t)(int16_t)(q0 & 0xFFFFu);
        norm[2u * lane + 1u] = (int32_t)(int16_t)(q0 >> 16);
        norm[128u + 2u * lane] = (int32_t)(int16_t)(q1 & 0xFFFFu);
        norm[128u + 2u * lane + 1u] = (int32_t)(int16_t)(q1 >> 16);
        hl = m.x;
        L = (uint32_t)m.y & 0xFFu;
        tl = (uint32_t)m.y >> 8;
        wave_sync();
        FSE_STAMP(P, 1);
        FSE_STAMP(P, 2);
    } else {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(in);
        // The header words are loaded before the length arrives when the slot
        // holds HDR_MAX bytes (always, for encoder slots), so the two loads and
        // the marker byte's load overlap instead of following one another;
        // words past the block are zeroed once the length is known.
        uint32_t r0, r1;
        if (P.slot_bytes >= HDR_MAX) {
            r0 = w[lane];
            r1 = w[lane + 64u];
        }
        const uint32_t nw = (uint32_t)min((uint64_t)min(clen, HDR_MAX) + 3u, P.slot_bytes) >> 2;
        if (P.slot_bytes < HDR_MAX) {
            r0 = lane < nw ? w[lane] : 0u;
            r1 = lane + 64u < nw ? w[lane + 64u] : 0u;
        }
        r0 = lane < nw ? r0 : 0u;
        r1 = lane + 64u < nw ? r1 : 0u;
        for (uint32_t s = lane; s < 256u; s += WAVE) norm[s] = 0;
        wave_sync();
        FSE_STAMP(P, 1);
        hl = header_read_wave(r0, r1, clen, (uint32_t)LMAX, norm, &L, &tl);
        FSE_STAMP(P, 2);
    }
    int rc = hl < 0 ? hl : FSE_OK;
    if (rc == FSE_OK && ((uint32_t)hl >= clen || last == 0)) rc = FSE_ERR_NO_MARKER;  // lib.rs:222
    if (rc == FSE_OK && clen > (1u << 28)) rc = FSE_ERR_UNSUPPORTED;  // bit positions are 32-bit in the decoders
    wave_sync();
    if (rc == FSE_OK) {
        const uint32_t size = 1u << L;
        uint32_t* dt = P.dt + gb * (uint64_t)SIZE;
        auto visit = [&](uint32_t i, uint32_t s, uint32_t nx) {  // nx = the symbol's first x + rank
            const uint32_t nb = L - ilog2u(nx);
            dt[i] = Dte<LMAX>::make(nb, s, (nx << nb) - size);
        };
        auto first_x = [&](uint32_t s) {  // symbol_next (fse.rs:296-308): 1 for a -1 count
            const int32_t v = norm[s];
            return v < 0 ? 1u : (uint32_t)v;
        };
        // two-pass ranks need 2^L / 64 per-chunk registers: up to L = 12
        const RankAtomic ra{P.peer_ranks == 0u, occ, nullptr, 0u, &g_rank_fb_dec, P.rank_inject};
        if (LMAX <= 12)
            rc = wave_build_spread<SIZE / 64u, true>(norm, L, tl, sym_at, occ, cumul, cnt, visit, first_x, ra, rk,
                                                     nullptr, &P);
        else rc = wave_build_spread<64, true>(norm, L, tl, sym_at, occ, cumul, cnt, visit, first_x, ra);
    }
    FSE_STAMP(P, 8);
    if (lane == 0) P.dtinfo[gb] = rc == FSE_OK ? (int32_t)((uint32_t)hl | (L << 16)) : rc;
}

hipError_t launch_dtables(const DtParams& P0, uint32_t lmax, hipStream_t stream) {
    DtParams P = P0;
    P.peer_ranks = atomic_ranks_on() ? 0u : 1u;
    // the staged rows hold headers up to L = 12; without the whole scratch the table kernel parses
    const bool parse = lmax <= 12 && P.hdr_meta && P.hdr_norm;
    if (!parse) P.hdr_meta = nullptr;
    with_lmax(lmax, [&](auto Lc) {
        constexpr int L = decltype(Lc)::value;
        if constexpr (L <= 12) {
            const dim3 gp((P.n_blocks + HP_BLOCKS - 1u) / HP_BLOCKS);
            if (parse) hipLaunchKernelGGL((hdr_parse_kernel<L>), gp, dim3(64), 0, stream, P);
        }
        hipLaunchKernelGGL((dtable_blocks_kernel<L>), dim3(P.n_blocks), dim3(64), P.xlds, stream, P);
    });
    return hipGetLastError();
}

}  // namespace fsehip
