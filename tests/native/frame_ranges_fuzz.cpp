// frame_ranges_fuzz.cpp -- the range planner of fsehip_frame_decompress_ranges
// (entropy_coders_amd/csrc/fse_frame.cpp, fse_frame_plan.h) against a
// brute-force per-byte model, built with g++ -fsanitize=address,undefined
// (tests/test_frame_ranges_plan.py).  Seeded random headers and range sets;
// prints "ok <cases>" or the first violated property.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../entropy_coders_amd/csrc/fse_frame_plan.h"

using fsehip::RangePiece;
using fsehip::RangePlan;
using fsehip::RangeRun;

static int g_case = 0;
static long g_runs = 0, g_bounced = 0, g_chunks = 0, g_both = 0;  // what the random cases reached
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        if (!(c)) {                                                                     \
            printf("FAIL case %d line %d: %s\n", g_case, __LINE__, #c);                 \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

static fsehip_frame_info make_info(uint64_t n_total, uint32_t bs) {
    fsehip_frame_info f{};
    f.version = 1;
    f.nstates = 2;
    f.max_table_log = 11;
    f.flags = 1;
    f.block_size = bs;
    f.ckpt_interval = 64;
    f.n_total = n_total;
    f.n_blocks = (uint32_t)(n_total / bs + (n_total % bs ? 1 : 0));
    f.records_off = 32 + 4ull * f.n_blocks;
    return f;
}

static uint64_t raw_len(const fsehip_frame_info& f, uint64_t b) {
    return std::min<uint64_t>(f.block_size, f.n_total - b * f.block_size);
}

static void check_plan(const fsehip_frame_info& f, uint32_t cb_cap, uint64_t out_addr,
                       const std::vector<fsehip_frame_range>& rg, const RangePlan& P) {
    const uint64_t bs = f.block_size;
    const uint32_t n = (uint32_t)rg.size();
    // the unique block list: ascending, and exactly the blocks a byte of some range lies in
    std::vector<uint8_t> covered(f.n_blocks, 0);
    for (const auto& g : rg)
        for (uint64_t k = 0; k < g.len; ++k) covered[(g.src_off + k) / bs] = 1;
    std::vector<uint32_t> want;
    for (uint32_t b = 0; b < f.n_blocks; ++b)
        if (covered[b]) want.push_back(b);
    REQUIRE(P.blocks == want);
    // every (range, byte) is served exactly once, by a piece inside its block or by the range's run,
    // from the right source byte
    REQUIRE(P.piece_start.size() == (size_t)n + 1 && P.piece_start[0] == 0 && P.piece_start[n] == P.pieces.size());
    REQUIRE(P.range_slot.size() == n && P.range_blocks.size() == n);
    std::vector<uint8_t> needs_bounce(P.blocks.size(), 0);
    std::vector<int> runs_of(n, 0);
    for (uint32_t r = 0; r < n; ++r) {
        const auto& g = rg[r];
        std::vector<uint8_t> served(g.len, 0);
        if (g.len) {
            REQUIRE(P.range_slot[r] < P.blocks.size() && P.blocks[P.range_slot[r]] == g.src_off / bs);
            REQUIRE(P.range_blocks[r] == (g.src_off + g.len - 1) / bs - g.src_off / bs + 1);
        } else {
            REQUIRE(P.range_blocks[r] == 0);
        }
        REQUIRE(P.piece_start[r] <= P.piece_start[r + 1]);
        for (uint64_t i = P.piece_start[r]; i < P.piece_start[r + 1]; ++i) {
            const RangePiece& pc = P.pieces[i];
            REQUIRE(pc.range == r && pc.slot < P.blocks.size() && pc.len > 0);
            if (i > P.piece_start[r]) REQUIRE(pc.slot > P.pieces[i - 1].slot);  // block order
            REQUIRE(pc.slot >= P.range_slot[r] && pc.slot - P.range_slot[r] < P.range_blocks[r]);
            const uint64_t b = P.blocks[pc.slot];
            REQUIRE((uint64_t)pc.in_off + pc.len <= raw_len(f, b));
            REQUIRE(pc.dst_off >= g.dst_off);
            const uint64_t k0 = pc.dst_off - g.dst_off;
            REQUIRE(k0 + pc.len <= g.len);
            REQUIRE(b * bs + pc.in_off == g.src_off + k0);
            for (uint64_t k = 0; k < pc.len; ++k) {
                REQUIRE(!served[k0 + k]);
                served[k0 + k] = 1;
            }
            needs_bounce[pc.slot] = 1;
        }
        // direct runs: whole blocks of their range, aligned destinations, long enough, one per range
        for (const RangeRun& run : P.runs) {
            if (run.range != r) continue;
            REQUIRE(++runs_of[r] == 1 && run.n_blocks >= fsehip::kDirectMinBlocks);
            const uint64_t lo = (uint64_t)run.first_block * bs, last = (uint64_t)run.first_block + run.n_blocks - 1;
            REQUIRE(last < f.n_blocks);
            const uint64_t hi = last * bs + raw_len(f, last);
            REQUIRE(lo >= g.src_off && hi <= g.src_off + g.len);
            REQUIRE(run.dst_off == g.dst_off + (lo - g.src_off));
            REQUIRE(((out_addr + run.dst_off) & 15u) == 0 && (bs & 15u) == 0);
            REQUIRE(run.slot + (uint64_t)run.n_blocks <= P.blocks.size());
            for (uint32_t i = 0; i < run.n_blocks; ++i) REQUIRE(P.blocks[run.slot + i] == run.first_block + i);
            for (uint64_t k = lo - g.src_off; k < hi - g.src_off; ++k) {
                REQUIRE(!served[k]);
                served[k] = 1;
            }
        }
        for (uint8_t s : served) REQUIRE(s);
    }
    for (const RangeRun& run : P.runs) REQUIRE(run.range < n);
    // the bounce list: exactly the slots with a piece, ascending; its pieces in list order
    std::vector<uint32_t> want_bounce;
    for (uint32_t s = 0; s < P.blocks.size(); ++s)
        if (needs_bounce[s]) want_bounce.push_back(s);
    REQUIRE(P.bounce == want_bounce);
    REQUIRE(P.bounce_piece.size() == P.pieces.size());
    std::vector<uint8_t> listed(P.pieces.size(), 0);
    for (size_t k = 0; k < P.bounce_piece.size(); ++k) {
        REQUIRE(P.bounce_piece[k] < P.pieces.size());
        const RangePiece& pc = P.pieces[P.bounce_piece[k]];
        REQUIRE(pc.bounce < P.bounce.size() && P.bounce[pc.bounce] == pc.slot);
        if (k) REQUIRE(P.pieces[P.bounce_piece[k - 1]].bounce <= pc.bounce);
        REQUIRE(!listed[P.bounce_piece[k]]);
        listed[P.bounce_piece[k]] = 1;
    }
    // chunks: at most cb_cap blocks, full but the last, pieces split alike; the short last block ends its chunk
    const size_t nc = P.chunk_start.size();
    REQUIRE(nc >= 1 && P.chunk_piece.size() == nc && P.chunk_start[0] == 0 && P.chunk_piece[0] == 0);
    REQUIRE(P.chunk_start[nc - 1] == P.bounce.size() && P.chunk_piece[nc - 1] == P.bounce_piece.size());
    for (size_t c = 0; c + 1 < nc; ++c) {
        const uint32_t j0 = P.chunk_start[c], j1 = P.chunk_start[c + 1];
        REQUIRE(j1 > j0 && j1 - j0 <= cb_cap && (c + 2 == nc || j1 - j0 == cb_cap));
        REQUIRE(P.chunk_piece[c] <= P.chunk_piece[c + 1]);
        for (uint64_t k = P.chunk_piece[c]; k < P.chunk_piece[c + 1]; ++k) {
            const uint32_t j = P.pieces[P.bounce_piece[k]].bounce;
            REQUIRE(j >= j0 && j < j1);
        }
        for (uint32_t j = j0; j < j1; ++j) {
            const uint64_t b = P.blocks[P.bounce[j]];
            if (raw_len(f, b) != bs) REQUIRE(j == j1 - 1);
        }
    }
}

static int plan(const fsehip_frame_info& f, uint32_t cb_cap, uint64_t out_addr, uint64_t out_cap,
                const std::vector<fsehip_frame_range>& rg, RangePlan* P) {
    // an exact-size heap copy: a read past the caller's array is a sanitizer error
    fsehip_frame_range* a = rg.empty() ? nullptr : new fsehip_frame_range[rg.size()];
    std::copy(rg.begin(), rg.end(), a);
    const int rc = fsehip::frame_plan_ranges(&f, cb_cap, out_addr, out_cap, a, (uint32_t)rg.size(), P);
    delete[] a;
    return rc;
}

static void rejections() {
    const fsehip_frame_info f = make_info(8 * 4096 + 1000, 4096);
    const uint64_t cap = 1u << 20, top = ~0ull;
    RangePlan P;
    auto rc = [&](std::vector<fsehip_frame_range> rg, uint64_t out_cap) { return plan(f, 4, 0, out_cap, rg, &P); };
    REQUIRE(rc({{0, f.n_total, 0}}, cap) == FSE_OK);
    REQUIRE(rc({{f.n_total, 0, 0}}, 0) == FSE_OK);                 // an empty range at the end
    REQUIRE(rc({{top, 2, 0}}, cap) == FSE_ERR_BAD_ARG);            // src_off + len overflows u64
    REQUIRE(rc({{2, top, 0}}, cap) == FSE_ERR_BAD_ARG);
    REQUIRE(rc({{f.n_total, 1, 0}}, cap) == FSE_ERR_BAD_ARG);      // past n_total
    REQUIRE(rc({{f.n_total - 1, 2, 0}}, cap) == FSE_ERR_BAD_ARG);
    REQUIRE(rc({{0, 2, top}}, cap) == FSE_ERR_BAD_ARG);            // dst_off + len overflows
    REQUIRE(rc({{0, 10, 0}, {100, 10, 9}}, cap) == FSE_ERR_BAD_ARG);   // destinations overlap
    REQUIRE(rc({{0, 10, 5}, {100, 10, 0}}, cap) == FSE_ERR_BAD_ARG);
    REQUIRE(rc({{0, 10, 0}, {0, 10, 10}}, cap) == FSE_OK);         // the same source twice, touching destinations
    REQUIRE(rc({{0, 10, 0}, {5, 0, 3}}, cap) == FSE_OK);           // an empty range overlaps nothing
    REQUIRE(rc({{0, 10, 0}}, 9) == FSE_ERR_DST_TOO_SMALL);         // past out_cap
    REQUIRE(rc({{0, 10, cap - 9}}, cap) == FSE_ERR_DST_TOO_SMALL);
    REQUIRE(rc({{0, 10, cap - 10}}, cap) == FSE_OK);
    REQUIRE(rc({{0, 0, cap}}, cap) == FSE_OK);
    REQUIRE(rc({{0, 0, cap + 1}}, cap) == FSE_ERR_DST_TOO_SMALL);  // an empty range's place counts too
    REQUIRE(fsehip::frame_plan_ranges(nullptr, 4, 0, cap, nullptr, 0, &P) == FSE_ERR_BAD_ARG);
    REQUIRE(fsehip::frame_plan_ranges(&f, 4, 0, cap, nullptr, 1, &P) == FSE_ERR_BAD_ARG);
    fsehip_frame_info bad = f;
    bad.n_blocks += 1;
    REQUIRE(plan(bad, 4, 0, cap, {{0, 1, 0}}, &P) == FSE_ERR_BAD_ARG);  // an info read_header would reject
    bad = f;
    bad.reserved = 1;
    REQUIRE(plan(bad, 4, 0, cap, {}, &P) == FSE_ERR_BAD_ARG);
    // the empty frame: empty ranges only
    const fsehip_frame_info e = make_info(0, 4096);
    REQUIRE(plan(e, 1, 0, 0, {}, &P) == FSE_OK && P.blocks.empty() && P.chunk_start.size() == 1);
    REQUIRE(plan(e, 1, 0, 0, {{0, 0, 0}}, &P) == FSE_OK && P.pieces.empty());
    REQUIRE(plan(e, 1, 0, cap, {{0, 1, 0}}, &P) == FSE_ERR_BAD_ARG);
    // the largest frame the header can describe: the planner works in u64 and in covered blocks only
    const uint64_t big_bs = 1u << 28;
    const fsehip_frame_info big = make_info(0xFFFFFFFFull * big_bs - 7, (uint32_t)big_bs);
    REQUIRE(big.n_blocks == 0xFFFFFFFFu);
    REQUIRE(plan(big, 4096, 0, ~0ull, {{big.n_total - 100, 100, 1ull << 40}, {big_bs - 1, 2, 0}}, &P) == FSE_OK);
    REQUIRE(P.blocks.size() == 3 && P.blocks[0] == 0 && P.blocks[1] == 1 && P.blocks[2] == 0xFFFFFFFEu);
    REQUIRE(P.pieces.size() == 3 && P.pieces[0].slot == 2 && P.pieces[0].in_off == big_bs - 7 - 100);
    REQUIRE(P.range_slot[0] == 2 && P.range_blocks[0] == 1 && P.range_slot[1] == 0 && P.range_blocks[1] == 2);
    REQUIRE(plan(big, 4096, 0, ~0ull, {{big.n_total, 1, 0}}, &P) == FSE_ERR_BAD_ARG);
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    rejections();
    std::mt19937_64 rng(0xF5EF0002ull);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    for (g_case = 0; g_case < cases; ++g_case) {
        // 0..12 blocks of 16..160 bytes (or one block of any size), a ragged tail most of the time
        const bool one = below(8) == 0;
        const uint32_t bs = one ? 1 + (uint32_t)below(200) : 16u * (1 + (uint32_t)below(10));
        const uint64_t n_total = one ? below(bs + 1) : below(4) ? below(12ull * bs + 1) : bs * below(13);
        const fsehip_frame_info f = make_info(n_total, bs);
        const uint32_t cb_cap = 1 + (uint32_t)below(6);
        const uint64_t out_addr = 0x7000 + (below(3) ? 0 : below(16));
        // ranges laid out in destination order with random gaps, then shuffled
        const uint32_t n = (uint32_t)below(7);
        std::vector<fsehip_frame_range> rg;
        uint64_t at = 0;
        for (uint32_t r = 0; r < n; ++r) {
            fsehip_frame_range g{};
            const int shape = (int)below(6);
            if (shape == 0 || n_total == 0) {
                g.src_off = below(n_total + 1);
                g.len = 0;
            } else if (shape == 1) {  // whole blocks, often up to the frame's end
                const uint64_t b0 = below(f.n_blocks), b1 = b0 + 1 + below(f.n_blocks - b0);
                g.src_off = b0 * bs;
                g.len = std::min<uint64_t>(b1 * bs, n_total) - g.src_off;
            } else if (shape == 2) {  // ends with the frame
                g.src_off = below(n_total);
                g.len = n_total - g.src_off;
            } else {
                g.src_off = below(n_total);
                g.len = 1 + below(n_total - g.src_off);
            }
            at += below(3) ? 0 : below(40);
            if (below(2)) at = (at + 15) & ~15ull;
            g.dst_off = at;
            at += g.len;
            rg.push_back(g);
        }
        std::shuffle(rg.begin(), rg.end(), rng);
        RangePlan P;
        REQUIRE(plan(f, cb_cap, out_addr, at, rg, &P) == FSE_OK);
        check_plan(f, cb_cap, out_addr, rg, P);
        g_runs += (long)P.runs.size();
        g_bounced += (long)P.bounce.size();
        g_chunks += (long)P.chunk_start.size() - 1;
        g_both += !P.runs.empty() && !P.bounce.empty();
        REQUIRE(plan(f, cb_cap, out_addr, at, rg, nullptr) == FSE_OK);  // validation alone
        const bool ends_at_cap = std::any_of(rg.begin(), rg.end(), [&](const fsehip_frame_range& g) {
            return g.len != 0 && g.dst_off + g.len == at;
        });
        if (ends_at_cap) REQUIRE(plan(f, cb_cap, out_addr, at - 1, rg, &P) == FSE_ERR_DST_TOO_SMALL);
    }
    // the generator must reach both routes, several chunks per call and calls that mix the routes
    REQUIRE(cases < 1000 || (g_runs > 100 && g_bounced > 1000 && g_chunks > 1000 && g_both > 100));
    printf("ok %d cases, %ld runs, %ld bounced blocks, %ld chunks, %ld mixed\n", cases, g_runs, g_bounced, g_chunks, g_both);
    return 0;
}
