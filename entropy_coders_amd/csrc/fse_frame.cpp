// fse_frame.cpp -- the frame's header and the range planner, host side
// (fsehip.h section 2b).
//
// Plain C++ with no HIP include: the same source builds into libfsehip.so
// and, with g++ alone, into the sanitizer fuzz of tests/native/frame_fuzz.cpp.
// The device side (directory, records) is fse_frame.hip.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/fsehip.h"
#include "fse_frame_plan.h"

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

// ------------------------------------------------------------------------
// The planner of fsehip_frame_decompress_ranges (fse_frame_plan.h)
// ------------------------------------------------------------------------
namespace fsehip {

namespace {
// covered blocks [first, last] whose slots start at `slot`
struct Span {
    uint64_t first, last, slot;
};
}  // namespace

int frame_plan_ranges(const fsehip_frame_info* info, uint32_t cb_cap, uint64_t out_addr, uint64_t out_cap,
                      const fsehip_frame_range* ranges, uint32_t n_ranges, RangePlan* plan) {
    if (!info || (n_ranges && !ranges) || cb_cap == 0u || !fields_ok(*info)) return FSE_ERR_BAD_ARG;
    const uint64_t bs = info->block_size, n_total = info->n_total, nb = info->n_blocks;
    // block sizes are powers of two in practice: a shift, not a 64-bit division, per lookup
    const bool pow2 = (bs & (bs - 1u)) == 0u;
    uint32_t sh = 0;
    while (pow2 && (1ull << sh) < bs) ++sh;
    const auto blk = [&](uint64_t x) { return pow2 ? x >> sh : x / bs; };
    std::vector<std::pair<uint64_t, uint64_t>> dst;  // non-empty destinations [lo, hi)
    dst.reserve(n_ranges);
    uint64_t dst_end = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_frame_range& g = ranges[r];
        if (g.src_off + g.len < g.src_off || g.src_off + g.len > n_total) return FSE_ERR_BAD_ARG;
        if (g.dst_off + g.len < g.dst_off) return FSE_ERR_BAD_ARG;
        if (g.len) dst.emplace_back(g.dst_off, g.dst_off + g.len);
        dst_end = std::max(dst_end, g.dst_off + g.len);
    }
    // callers mostly pass ranges in order: sort only what is not sorted
    if (!std::is_sorted(dst.begin(), dst.end())) std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); ++i)
        if (dst[i].first < dst[i - 1].second) return FSE_ERR_BAD_ARG;
    if (dst_end > out_cap) return FSE_ERR_DST_TOO_SMALL;  // an empty range's place counts too
    if (!plan) return FSE_OK;
    *plan = RangePlan();
    RangePlan& P = *plan;

    // the covered blocks: the ranges' block intervals, merged
    std::vector<Span> spans;
    spans.reserve(dst.size());
    for (uint32_t r = 0; r < n_ranges; ++r)
        if (ranges[r].len)
            spans.push_back({blk(ranges[r].src_off), blk(ranges[r].src_off + ranges[r].len - 1u), 0u});
    const auto by_first = [](const Span& a, const Span& b) { return a.first < b.first; };
    if (!std::is_sorted(spans.begin(), spans.end(), by_first)) std::sort(spans.begin(), spans.end(), by_first);
    size_t ns = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        if (ns && spans[i].first <= spans[ns - 1].last + 1u)
            spans[ns - 1].last = std::max(spans[ns - 1].last, spans[i].last);
        else
            spans[ns++] = spans[i];
    }
    spans.resize(ns);
    uint64_t n_cov = 0;
    for (Span& s : spans) {
        s.slot = n_cov;
        n_cov += s.last - s.first + 1u;
    }
    P.blocks.resize(n_cov);
    for (const Span& s : spans)
        for (uint64_t b = s.first; b <= s.last; ++b) P.blocks[s.slot + (b - s.first)] = (uint32_t)b;
    size_t hint = 0;  // the span of the last lookup: ranges in order find theirs there or next to it
    auto slot_of = [&](uint64_t b) {
        if (!(spans[hint].first <= b && b <= spans[hint].last)) {
            if (hint + 1u < spans.size() && spans[hint + 1u].first <= b && b <= spans[hint + 1u].last) {
                ++hint;
            } else {
                size_t lo = 0, hi = spans.size();  // the last span with first <= b
                while (hi - lo > 1u) {
                    const size_t mid = (lo + hi) / 2u;
                    if (spans[mid].first <= b) lo = mid; else hi = mid;
                }
                hint = lo;
            }
        }
        return (uint32_t)(spans[hint].slot + (b - spans[hint].first));
    };

    // direct runs and bounce pieces, range by range
    std::vector<uint8_t> bounced(n_cov, 0);
    P.piece_start.assign((size_t)n_ranges + 1u, 0u);
    P.range_slot.assign(n_ranges, 0u);
    P.range_blocks.assign(n_ranges, 0u);
    P.pieces.reserve(2u * (size_t)n_ranges);
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const fsehip_frame_range& g = ranges[r];
        P.piece_start[r] = P.pieces.size();
        if (!g.len) continue;
        const uint64_t end = g.src_off + g.len;
        const uint64_t b0 = blk(g.src_off), b1 = blk(end - 1u);
        const uint32_t s0 = slot_of(b0);  // the range's blocks are consecutive slots from here
        P.range_slot[r] = s0;
        P.range_blocks[r] = (uint32_t)(b1 - b0 + 1u);
        // whole blocks [w0, w1): the frame's last block counts when the range ends with the frame
        uint64_t w0 = b0 + (g.src_off != b0 * bs ? 1u : 0u);
        uint64_t w1 = end == n_total ? nb : blk(end);
        bool run = false;
        if (w1 > w0 && w1 - w0 >= kDirectMinBlocks && !(bs & 15u)) {
            const uint64_t d0 = g.dst_off + (w0 * bs - g.src_off);
            if (((out_addr + d0) & 15u) == 0u) {
                run = true;
                P.runs.push_back({r, (uint32_t)w0, (uint32_t)(w1 - w0), s0 + (uint32_t)(w0 - b0), d0});
            }
        }
        if (!run) w0 = w1 = b1 + 1u;
        for (uint64_t b = b0; b <= b1; ++b) {
            if (b == w0) {  // the run serves [w0, w1)
                b = w1 - 1u;
                continue;
            }
            const uint64_t lo = std::max(g.src_off, b * bs), hi = std::min(end, (b + 1u) * bs);
            RangePiece pc{};
            pc.range = r;
            pc.slot = s0 + (uint32_t)(b - b0);
            pc.in_off = (uint32_t)(lo - b * bs);
            pc.len = (uint32_t)(hi - lo);
            pc.dst_off = g.dst_off + (lo - g.src_off);
            bounced[pc.slot] = 1;
            P.pieces.push_back(pc);
        }
    }
    P.piece_start[n_ranges] = P.pieces.size();

    // the bounce list, its pieces in list order (a counting sort), the chunks
    std::vector<uint32_t> bidx(n_cov, 0);
    for (uint64_t s = 0; s < n_cov; ++s)
        if (bounced[s]) {
            bidx[s] = (uint32_t)P.bounce.size();
            P.bounce.push_back((uint32_t)s);
        }
    std::vector<uint64_t> first(P.bounce.size() + 1u, 0u);
    for (RangePiece& pc : P.pieces) {
        pc.bounce = bidx[pc.slot];
        ++first[pc.bounce + 1u];
    }
    for (size_t j = 0; j < P.bounce.size(); ++j) first[j + 1u] += first[j];
    P.bounce_piece.resize(P.pieces.size());
    {
        std::vector<uint64_t> at(first.begin(), first.end() - 1);
        for (size_t i = 0; i < P.pieces.size(); ++i) P.bounce_piece[at[P.pieces[i].bounce]++] = i;
    }
    for (uint64_t j = 0; j < P.bounce.size(); j += cb_cap) {
        P.chunk_start.push_back((uint32_t)j);
        P.chunk_piece.push_back(first[j]);
    }
    P.chunk_start.push_back((uint32_t)P.bounce.size());
    P.chunk_piece.push_back(first[P.bounce.size()]);
    return FSE_OK;
}

}  // namespace fsehip
