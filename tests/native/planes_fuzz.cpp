// Fuzz of the plane frame's host code (entropy_coders_amd/csrc/fse_elem.cpp
// over fse_frame.cpp, include/fsehip.h section 2d), built by
// tests/test_planes_sanitized.py with AddressSanitizer + UBSan: valid, random,
// truncated and bit-flipped 48-byte heads are parsed from heap buffers
// allocated to their exact size, so a read past `len` or an undefined shift
// stops the run.  Every result must be FSE_OK with all fields inside their
// ranges (and then the writers reproduce the 48 bytes and the size formulas
// agree), or FSE_ERR_BAD_FRAME.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// a head that passes every rule: the planes header and an inner frame header of w * stride bytes
static void valid_head(uint8_t out[48]) {
    fsehip_planes_info p;
    std::memset(&p, 0, sizeof(p));
    p.version = 1;
    p.elem_bytes = 2u << (next_u64() % 3u);
    const uint32_t bits = (uint32_t)(next_u64() % 41u);  // up to 2^40 elements: 2^43 bytes at most
    p.n_elems = bits ? next_u64() % (1ull << bits) : 0u;
    if (fsehip_planes_write_header(&p, out) != FSE_OK) std::abort();
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

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int accepted = 0;
    for (int cs = 0; cs < cases; ++cs) {
        uint8_t h[64];
        for (size_t i = 0; i < sizeof(h); ++i) h[i] = (uint8_t)next_u64();
        const uint32_t mode = (uint32_t)(next_u64() % 5u);
        size_t len = 48 + (size_t)(next_u64() % 17u);
        if (mode != 0) valid_head(h);  // mode 0: random bytes
        if (mode == 0 && next_u64() % 2u) std::memcpy(h, "FSEP\x01", 5);  // random bytes behind a good magic
        if (mode == 2) len = (size_t)(next_u64() % 48u);  // truncated
        if (mode == 3) {  // one to three flipped bits
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[next_u64() % 48u] ^= (uint8_t)(1u << (next_u64() % 8u));
        }
        if (mode == 4) h[next_u64() % 48u] = (uint8_t)next_u64();  // one replaced byte
        uint8_t* buf = new uint8_t[len ? len : 1];  // exact size: ASan sees a read past len
        std::memcpy(buf, h, len);
        fsehip_planes_info p;
        fsehip_frame_info f;
        std::memset(&p, 0xEE, sizeof(p));
        std::memset(&f, 0xEE, sizeof(f));
        const int rc = fsehip_planes_read_header(len ? buf : nullptr, len, &p, &f);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (mode == 1) CHECK(rc == FSE_OK);
        if (mode == 2) CHECK(rc == FSE_ERR_BAD_FRAME);
        if (rc == FSE_OK) {
            CHECK(p.version == 1 && (p.elem_bytes == 2 || p.elem_bytes == 4 || p.elem_bytes == 8) && p.reserved == 0);
            CHECK(p.stride >= p.n_elems && p.stride - p.n_elems < 16 && p.stride % 16 == 0);
            CHECK(p.stride <= UINT64_MAX / p.elem_bytes && f.n_total == p.stride * p.elem_bytes);
            uint8_t back[48];
            CHECK(fsehip_planes_write_header(&p, back) == FSE_OK);
            CHECK(fsehip_frame_write_header(&f, back + 16) == FSE_OK);
            CHECK(std::memcmp(back, buf, 48) == 0);
            CHECK(fsehip_planes_scratch_bytes(p.n_elems, p.elem_bytes) == f.n_total);
            const uint64_t inner = fsehip_frame_bound(f.n_total, f.block_size);
            const uint64_t bound = fsehip_planes_bound(p.n_elems, p.elem_bytes, f.block_size);
            CHECK(bound == (inner >= f.n_total && inner <= UINT64_MAX - 16 ? 16 + inner : 0 /* u64 wrap */));
            const fsehip_planes_range r[2] = {{next_u64(), next_u64(), next_u64()}, {0, p.n_elems % 1000u, 3}};
            const uint64_t rs = fsehip_planes_ranges_scratch_bytes(p.elem_bytes, r, 2);
            CHECK(rs == 0 || rs >= r[0].n_elems * p.elem_bytes + r[1].n_elems * p.elem_bytes + 8u * p.elem_bytes);
            ++accepted;
        } else {
            CHECK(p.n_elems == 0 && p.elem_bytes == 0 && f.n_total == 0);  // outputs zeroed
        }
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases) {
        std::fprintf(stderr, "FAIL: %d of %d heads accepted\n", accepted, cases);
        return 1;
    }
    std::printf("ok %d cases, %d accepted\n", cases, accepted);
    return 0;
}
