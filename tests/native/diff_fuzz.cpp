// Fuzz of the diff frame's host code (entropy_coders_amd/csrc/fse_elem.cpp
// over fse_frame.cpp, include/fsehip.h section 2h), built by
// tests/test_diff_sanitized.py with AddressSanitizer + UBSan: valid, random,
// truncated and bit-flipped 48-byte heads are parsed from heap buffers
// allocated to their exact size, so a read past `len` or an undefined shift
// stops the run.  Every result must be FSE_OK with all fields inside their
// ranges (and then the writers reproduce the 48 bytes, the size formulas
// agree and the plane and delta readers refuse the same bytes), or
// FSE_ERR_BAD_FRAME.  Range lists, from exact-size heap arrays, go through
// the range-scratch formula and the range checks of the new kind against a
// plain restatement of both.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../entropy_coders_amd/csrc/fse_elem_host.h"
#include "../../include/fsehip.h"

static uint64_t rng_state = 0xD1FFD1FFD1FFD1FFull;
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

static bool width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// a head that passes every rule: the diff header and an inner frame header of w * stride bytes
static void valid_head(uint8_t out[48]) {
    fsehip_diff_info p;
    std::memset(&p, 0, sizeof(p));
    p.version = 1;
    p.elem_bytes = 1u << (next_u64() % 4u);
    const uint32_t bits = (uint32_t)(next_u64() % 41u);  // up to 2^40 elements: 2^43 bytes at most
    p.n_elems = bits ? next_u64() % (1ull << bits) : 0u;
    if (fsehip_diff_write_header(&p, out) != FSE_OK) std::abort();
    const uint64_t stride = (p.n_elems + 15u) & ~15ull;
    fsehip_frame_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.nstates = 1 + (uint32_t)(next_u64() % 2u);
    f.max_table_log = 11 + (uint32_t)(next_u64() % 5u);
    f.flags = (uint32_t)(next_u64() % 2u);
    f.ckpt_interval = f.flags ? 1u << (4 + next_u64() % 10u) : 0u;
    f.n_total = stride * p.elem_bytes;
    f.block_size = 16u << (12 + next_u64() % 13u);  // 64 KiB .. 256 MiB: n_blocks fits 32 bits
    f.n_blocks = (uint32_t)(f.n_total / f.block_size + (f.n_total % f.block_size != 0));
    if (fsehip_frame_write_header(&f, out + 16) != FSE_OK) std::abort();
}

// a size that is often small, sometimes near a multiple of 4096 and sometimes huge
static uint64_t some_u64() {
    switch (next_u64() % 4u) {
        case 0: return next_u64() % 64u;
        case 1: return 4096u * (next_u64() % 8u) + next_u64() % 3u - 1u;
        case 2: return next_u64() % (1ull << 20);
        default: return next_u64() >> (next_u64() % 64u);
    }
}

// the range rules and the scratch formula once more, in 128-bit arithmetic:
// a diff range's pieces are its n_elems bytes of each plane, back to back
static int ranges_model(const fsehip_planes_range* r, uint32_t n, uint64_t n_elems, uint32_t w, uint64_t out_cap,
                        uint64_t* scratch) {
    typedef unsigned __int128 u128;
    u128 at = 0, dst_end = 0;
    int rc = FSE_OK;
    for (uint32_t i = 0; i < n; ++i) {
        at += ((u128)r[i].n_elems * w + 15u) / 16u * 16u;
        if ((u128)r[i].elem_off + r[i].n_elems > n_elems) rc = FSE_ERR_BAD_ARG;
        if ((u128)r[i].dst_elem_off + r[i].n_elems > UINT64_MAX) rc = FSE_ERR_BAD_ARG;
    }
    at += ((u128)4u * w * n + 15u) / 16u * 16u;
    *scratch = at > UINT64_MAX ? 0 : (uint64_t)at;
    if (rc != FSE_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const u128 end = (u128)r[i].dst_elem_off + r[i].n_elems;
        dst_end = end > dst_end ? end : dst_end;
        for (uint32_t j = 0; j < i; ++j)
            if (r[i].n_elems && r[j].n_elems && r[i].dst_elem_off < r[j].dst_elem_off + r[j].n_elems &&
                r[j].dst_elem_off < r[i].dst_elem_off + r[i].n_elems)
                return FSE_ERR_BAD_ARG;
    }
    return dst_end * w > out_cap ? FSE_ERR_DST_TOO_SMALL : FSE_OK;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int accepted = 0, ranges_ok = 0;
    for (int cs = 0; cs < cases; ++cs) {
        uint8_t h[64];
        for (size_t i = 0; i < sizeof(h); ++i) h[i] = (uint8_t)next_u64();
        const uint32_t mode = (uint32_t)(next_u64() % 5u);
        size_t len = 48 + (size_t)(next_u64() % 17u);
        if (mode != 0) valid_head(h);  // mode 0: random bytes
        if (mode == 0 && next_u64() % 2u) std::memcpy(h, "FSEB\x01", 5);  // random bytes behind a good magic
        if (mode == 2) len = (size_t)(next_u64() % 48u);  // truncated
        if (mode == 3) {  // one to three flipped bits
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[next_u64() % 48u] ^= (uint8_t)(1u << (next_u64() % 8u));
        }
        if (mode == 4) h[next_u64() % 48u] = (uint8_t)next_u64();  // one replaced byte
        uint8_t* buf = new uint8_t[len ? len : 1];  // exact size: ASan sees a read past len
        std::memcpy(buf, h, len);
        fsehip_diff_info p;
        fsehip_frame_info f;
        std::memset(&p, 0xEE, sizeof(p));
        std::memset(&f, 0xEE, sizeof(f));
        const int rc = fsehip_diff_read_header(len ? buf : nullptr, len, &p, &f);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (mode == 1) CHECK(rc == FSE_OK);
        if (mode == 2) CHECK(rc == FSE_ERR_BAD_FRAME);
        if (rc == FSE_OK) {
            CHECK(p.version == 1 && width_ok(p.elem_bytes) && p.reserved == 0);
            CHECK(p.stride >= p.n_elems && p.stride - p.n_elems < 16 && p.stride % 16 == 0);
            CHECK(p.stride <= UINT64_MAX / p.elem_bytes && f.n_total == p.stride * p.elem_bytes);
            uint8_t back[48];
            CHECK(fsehip_diff_write_header(&p, back) == FSE_OK);
            CHECK(fsehip_frame_write_header(&f, back + 16) == FSE_OK);
            CHECK(std::memcmp(back, buf, 48) == 0);
            CHECK(fsehip_diff_scratch_bytes(p.n_elems, p.elem_bytes) == f.n_total);
            CHECK(fsehip::elem_check(fsehip::kDiff, &p, &f) == FSE_OK);
            const uint64_t inner = fsehip_frame_bound(f.n_total, f.block_size);
            const uint64_t bound = fsehip_diff_bound(p.n_elems, p.elem_bytes, f.block_size);
            CHECK(bound == (inner >= f.n_total && inner <= UINT64_MAX - 16 ? 16 + inner : 0 /* u64 wrap */));
            // the same bytes are no plane frame and no delta frame, and with their magic no diff frame
            fsehip_planes_info q;
            fsehip_frame_info g;
            CHECK(fsehip_planes_read_header(buf, len, &q, &g) == FSE_ERR_BAD_FRAME);
            CHECK(fsehip_delta_read_header(buf, len, &q, &g) == FSE_ERR_BAD_FRAME);
            buf[3] = "PDF"[next_u64() % 3u];
            CHECK(fsehip_diff_read_header(buf, len, &q, &g) == FSE_ERR_BAD_FRAME);
            ++accepted;
        } else {
            CHECK(p.n_elems == 0 && p.elem_bytes == 0 && p.stride == 0 && f.n_total == 0);  // outputs zeroed
        }
        delete[] buf;

        // a range list against the model
        fsehip_diff_info q;
        std::memset(&q, 0, sizeof(q));
        q.version = 1;
        q.elem_bytes = next_u64() % 8u ? 1u << (next_u64() % 4u) : (uint32_t)(next_u64() % 20u);
        q.n_elems = some_u64();
        const uint32_t n = (uint32_t)(next_u64() % 6u);
        fsehip_planes_range* r = new fsehip_planes_range[n ? n : 1];  // exact size again
        uint64_t at = next_u64() % 8u;
        for (uint32_t i = 0; i < n; ++i) {
            const bool tame = next_u64() % 4u != 0 && q.n_elems != UINT64_MAX;  // mostly inside the tensor, destinations mostly in order
            r[i].n_elems = tame && q.n_elems ? some_u64() % (q.n_elems + 1u) : some_u64();
            r[i].elem_off = tame && q.n_elems >= r[i].n_elems ? next_u64() % (q.n_elems - r[i].n_elems + 1u) : some_u64();
            r[i].dst_elem_off = next_u64() % 8u ? at : some_u64();
            at += r[i].n_elems + next_u64() % 2u;
        }
        const uint64_t out_cap = next_u64() % 2u ? UINT64_MAX : some_u64();
        const uint64_t got_scratch = fsehip_diff_ranges_scratch_bytes(q.elem_bytes, r, n);
        const int got = fsehip::elem_check_ranges(fsehip::kDiff, &q, out_cap, r, n);
        if (!width_ok(q.elem_bytes)) {
            CHECK(got_scratch == 0 && got == FSE_ERR_BAD_ARG);
        } else {
            uint64_t want_scratch;
            const int want = ranges_model(r, n, q.n_elems, q.elem_bytes, out_cap, &want_scratch);
            CHECK(got == want);
            CHECK(got_scratch == want_scratch);
            ranges_ok += got == FSE_OK;
        }
        delete[] r;
    }
    if (accepted == 0 || accepted == cases || ranges_ok == 0 || ranges_ok == cases) {
        std::fprintf(stderr, "FAIL: %d of %d heads accepted, %d range lists\n", accepted, cases, ranges_ok);
        return 1;
    }
    std::printf("ok %d cases, %d heads and %d range lists accepted\n", cases, accepted, ranges_ok);
    return 0;
}
