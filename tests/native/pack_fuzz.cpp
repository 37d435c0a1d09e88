// Fuzz of the pack frame's host code (entropy_coders_amd/csrc/fse_pack.cpp
// over fse_frame.cpp, include/fsehip.h section 2j), built by
// tests/test_pack_sanitized.py with AddressSanitizer + UBSan: valid, random,
// truncated and damaged heads (header, member table, inner frame header) and
// tables whose sums overflow are parsed from heap buffers allocated to their
// exact size, so a read past `len` or an undefined shift stops the run.  Every
// result must be FSE_OK with all fields inside their ranges (and then the
// writer reproduces the head, the size formulas agree, the planner's plane
// offsets are fsehip_pack_plane_offset's and tile the image exactly, and
// random selections plan inside the scratch they are promised), or
// FSE_ERR_BAD_FRAME with the outputs zeroed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../entropy_coders_amd/csrc/fse_pack_host.h"
#include "../../include/fsehip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "FAIL %s:%d case %d: %s\n", __FILE__, __LINE__, cs, #c); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// a member list that passes every rule; `huge`: element counts up to 2^40
static std::vector<fsehip_pack_member> valid_members(bool huge) {
    std::vector<fsehip_pack_member> v((size_t)(next_u64() % 40u));
    for (fsehip_pack_member& m : v) {
        m.d_ptr = nullptr;
        m.kind = 1u + (uint32_t)(next_u64() % 2u);
        m.elem_bytes = 1u << (next_u64() % 4u);
        const uint32_t bits = (uint32_t)(next_u64() % (huge ? 41u : 14u));
        m.n_elems = bits ? next_u64() % (1ull << bits) : 0u;
    }
    return v;
}

// the head of a valid list and a matching inner frame header
static std::vector<uint8_t> valid_head(const std::vector<fsehip_pack_member>& v) {
    const uint32_t n = (uint32_t)v.size();
    std::vector<uint8_t> out(32u + 16u * n + 32u);
    if (fsehip_pack_write_header(v.data(), n, out.data()) != FSE_OK) std::abort();
    fsehip_frame_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.nstates = 1 + (uint32_t)(next_u64() % 2u);
    f.max_table_log = 11 + (uint32_t)(next_u64() % 5u);
    f.flags = (uint32_t)(next_u64() % 2u);
    f.ckpt_interval = f.flags ? 1u << (4 + next_u64() % 10u) : 0u;
    f.n_total = fsehip_pack_image_bytes(v.data(), n);
    f.block_size = 16u << (12 + next_u64() % 13u);  // 64 KiB .. 256 MiB: n_blocks fits 32 bits
    f.n_blocks = (uint32_t)(f.n_total / f.block_size + (f.n_total % f.block_size != 0));
    if (fsehip_frame_write_header(&f, out.data() + 32u + 16u * n) != FSE_OK) std::abort();
    return out;
}

static void put_u64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int accepted = 0;
    for (int cs = 0; cs < cases; ++cs) {
        const uint32_t mode = (uint32_t)(next_u64() % 7u);
        const std::vector<fsehip_pack_member> v = valid_members(next_u64() % 2u);
        const uint32_t n = (uint32_t)v.size();
        std::vector<uint8_t> h = valid_head(v);
        const size_t full = h.size();
        size_t len = full + (size_t)(next_u64() % 17u);
        h.resize(len);
        for (size_t i = full; i < len; ++i) h[i] = (uint8_t)next_u64();
        if (mode == 0) {  // random bytes, half of them behind a good magic
            for (size_t i = 0; i < len; ++i) h[i] = (uint8_t)next_u64();
            if (next_u64() % 2u) std::memcpy(h.data(), "FSEM\x01\0\0\0", 8);
            if (next_u64() % 2u) h[10] = h[11] = 0;  // a member count that may fit the buffer
        }
        if (mode == 2) len = (size_t)(next_u64() % full);  // truncated: header, table or inner header
        if (mode == 3)  // one to three flipped bits
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[next_u64() % full] ^= (uint8_t)(1u << (next_u64() % 8u));
        if (mode == 4) h[next_u64() % full] = (uint8_t)next_u64();  // one replaced byte
        if (mode == 5 && n) {  // a count that overflows its stride, its image or the sum
            const uint32_t m = (uint32_t)(next_u64() % n);
            const uint64_t big[4] = {UINT64_MAX - (next_u64() % 15u), UINT64_MAX / (h[32 + 16 * m + 1] + 1u) + 1u,
                                     (UINT64_MAX >> 1) + 1u, UINT64_MAX - 15u};
            put_u64(&h[32 + 16 * m + 8], big[next_u64() % 4u]);
            if (n > 1) put_u64(&h[32 + 16 * ((m + 1) % n) + 8], big[2]);
        }
        if (mode == 6) {  // a member count beyond the table that is there
            const uint32_t more = n + 1u + (uint32_t)(next_u64() % (next_u64() % 2u ? 4u : 1u << 21));
            for (int i = 0; i < 4; ++i) h[8 + i] = (uint8_t)(more >> (8 * i));
        }
        uint8_t* buf = new uint8_t[len ? len : 1];  // exact size: ASan sees a read past len
        std::memcpy(buf, h.data(), len);
        fsehip_pack_info p, p2;
        fsehip_frame_info f;
        std::memset(&p, 0xEE, sizeof(p));
        std::memset(&p2, 0xEE, sizeof(p2));
        std::memset(&f, 0xEE, sizeof(f));
        const int rc0 = fsehip_pack_read_header(len ? buf : nullptr, len, &p2);
        CHECK(rc0 == FSE_OK || rc0 == FSE_ERR_BAD_FRAME);
        if (rc0 != FSE_OK) CHECK(p2.n_members == 0 && p2.image_bytes == 0 && p2.version == 0);
        else CHECK(p2.version == 1 && p2.n_members <= FSEHIP_PACK_MAX_MEMBERS);
        // the member array is exact too: a write past members_cap is seen
        const uint32_t cap = rc0 == FSE_OK && len >= 64u && p2.n_members <= (len - 64u) / 16u ? p2.n_members : n;
        fsehip_pack_member* got = new fsehip_pack_member[cap ? cap : 1];
        const int rc = fsehip_pack_read_members(len ? buf : nullptr, len, got, cap, &p, &f);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME || (rc == FSE_ERR_DST_TOO_SMALL && mode != 1));
        if (mode == 1) CHECK(rc == FSE_OK);
        if (mode == 2 || mode == 5 || mode == 6) CHECK(rc != FSE_OK || (mode == 5 && n == 0));
        if (rc0 != FSE_OK) CHECK(rc == FSE_ERR_BAD_FRAME);
        if (rc == FSE_OK) {
            const uint32_t k = p.n_members;
            CHECK(p.version == 1 && k <= cap && len >= 64u + 16u * (size_t)k);
            uint64_t image = 0, content = 0;
            for (uint32_t m = 0; m < k; ++m) {
                CHECK(got[m].d_ptr == nullptr && (got[m].kind == 1 || got[m].kind == 2));
                CHECK(got[m].elem_bytes == 1 || got[m].elem_bytes == 2 || got[m].elem_bytes == 4 || got[m].elem_bytes == 8);
                CHECK(got[m].n_elems <= UINT64_MAX - 15u);
                const uint64_t stride = (got[m].n_elems + 15u) & ~15ull;
                CHECK(stride <= (UINT64_MAX - image) / got[m].elem_bytes);
                image += stride * got[m].elem_bytes;
                content += got[m].n_elems * got[m].elem_bytes;
            }
            CHECK(p.image_bytes == image && p.content_bytes == content && f.n_total == image);
            std::vector<uint8_t> back(32u + 16u * (size_t)k + 32u);
            CHECK(fsehip_pack_write_header(got, k, back.data()) == FSE_OK);
            CHECK(fsehip_frame_write_header(&f, back.data() + 32u + 16u * (size_t)k) == FSE_OK);
            CHECK(std::memcmp(back.data(), buf, back.size()) == 0);
            CHECK(fsehip_pack_image_bytes(got, k) == image);
            const uint64_t inner = fsehip_frame_bound(image, f.block_size), head = 32u + 16u * (uint64_t)k;
            CHECK(fsehip_pack_bound(got, k, f.block_size) == (inner >= image && inner <= UINT64_MAX - head ? head + inner : 0));
            const uint64_t scratch = fsehip_pack_scratch_bytes(got, k);
            CHECK(scratch % 16u == 0 && scratch >= image + sizeof(fsehip::PackDesc) * k + head);
            // the planner: offsets are the exported ones, multiples of 16, and the planes tile the image
            std::vector<fsehip::PackDesc> d(k ? k : 1);
            const uint64_t tiles = fsehip::pack_plan(got, k, d.data());
            uint64_t want_tiles = 0, covered = 0;
            std::vector<std::pair<uint64_t, uint64_t>> spans;
            for (uint32_t m = 0; m < k; ++m) {
                CHECK(d[m].first_tile == want_tiles && d[m].w == got[m].elem_bytes && d[m].kind == got[m].kind);
                CHECK(d[m].n_elems == got[m].n_elems);
                want_tiles += (got[m].n_elems + 4095u) / 4096u;
                const uint64_t stride = (got[m].n_elems + 15u) & ~15ull;
                for (uint32_t b = 0; b < got[m].elem_bytes; ++b) {
                    CHECK(d[m].plane[b] == fsehip_pack_plane_offset(got, k, m, b) && d[m].plane[b] % 16u == 0);
                    CHECK(d[m].plane[b] <= image && stride <= image - d[m].plane[b]);
                    if (stride) spans.emplace_back(d[m].plane[b], stride);
                    covered += stride;
                }
                CHECK(fsehip_pack_plane_offset(got, k, m, got[m].elem_bytes) == UINT64_MAX);
            }
            CHECK(tiles == want_tiles && covered == image);
            std::sort(spans.begin(), spans.end());
            uint64_t at = 0;
            for (const auto& s : spans) {
                CHECK(s.first == at);
                at += s.second;
            }
            CHECK(fsehip_pack_plane_offset(got, k, k, 0) == UINT64_MAX);
            // random selections: valid ones plan inside their scratch, others are refused
            std::vector<uint32_t> sel((size_t)(next_u64() % 6u));
            bool valid = true;
            for (uint32_t& s : sel) s = (uint32_t)(next_u64() % (k + 2u));
            for (size_t i = 0; i < sel.size(); ++i) {
                valid = valid && sel[i] < k;
                for (size_t j = 0; j < i; ++j) valid = valid && sel[i] != sel[j];
            }
            std::vector<fsehip::PackDesc> sd;
            std::vector<fsehip_frame_range> fr;
            uint64_t planes_bytes = 0, sel_tiles = 0;
            const int src = fsehip::pack_plan_selected(got, k, sel.data(), (uint32_t)sel.size(), &sd, &fr, &planes_bytes,
                                                       &sel_tiles);
            CHECK(src == (valid ? FSE_OK : FSE_ERR_BAD_ARG));
            const uint64_t need = fsehip_pack_members_scratch_bytes(got, k, sel.data(), (uint32_t)sel.size());
            bool in_range = true;
            for (uint32_t s : sel) in_range = in_range && s < k;
            CHECK((need != 0) == in_range);
            if (valid) {
                CHECK(sd.size() == sel.size() && planes_bytes % 16u == 0);
                CHECK(need >= planes_bytes + 4u * fr.size() + sizeof(fsehip::PackDesc) * sel.size() + head);
                uint64_t dst = 0;
                size_t r = 0;
                for (size_t i = 0; i < sel.size(); ++i) {
                    const fsehip_pack_member& mb = got[sel[i]];
                    const uint64_t stride = (mb.n_elems + 15u) & ~15ull;
                    CHECK(sd[i].status0 == r && sd[i].w == mb.elem_bytes && sd[i].n_elems == mb.n_elems);
                    for (uint32_t b = 0; b < mb.elem_bytes; ++b) {
                        CHECK(sd[i].plane[b] == dst);
                        if (stride) {
                            CHECK(r < fr.size() && fr[r].src_off == d[sel[i]].plane[b] && fr[r].len == stride &&
                                  fr[r].dst_off == dst);
                            ++r;
                        }
                        dst += stride;
                    }
                }
                CHECK(r == fr.size() && dst == planes_bytes);
            }
            ++accepted;
        } else {
            CHECK(p.n_members == 0 && p.image_bytes == 0 && p.content_bytes == 0 && f.n_total == 0);  // outputs zeroed
        }
        delete[] got;
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases) {
        std::fprintf(stderr, "FAIL: %d of %d heads accepted\n", accepted, cases);
        return 1;
    }
    std::printf("ok %d cases, %d accepted\n", cases, accepted);
    return 0;
}
