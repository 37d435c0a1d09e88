// Fuzz of the check record's host code (entropy_coders_amd/csrc/fse_check.cpp
// alone, include/fsehip.h section 2f), built by tests/test_check_sanitized.py
// with AddressSanitizer + UBSan.
//   heads    valid, random, truncated and bit-flipped record heads and sealed
//            heads, parsed from heap buffers of their exact size: FSE_OK with
//            every field in range (and the writer reproduces the bytes), or
//            FSE_ERR_BAD_FRAME with the outputs zeroed;
//   crc      fsehip_crc32 at every alignment 0..15 and length 0..70 against a
//            bitwise CRC-32 written here, in one call and in two;
//   combine  fsehip_crc32_combine against the CRC of the concatenation;
//   ranges   fsehip_check_ranges_verified_bytes against a per-byte model.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

// CRC-32, one bit at a time
static uint32_t crc_bitwise(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

static void put64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// a record header that passes every rule
static fsehip_check_info valid_info() {
    fsehip_check_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.algorithm = FSEHIP_CHECK_CRC32;
    f.check_log = 8 + (uint32_t)(next_u64() % 9u);
    const uint32_t bits = (uint32_t)(next_u64() % (32u + f.check_log));  // n_cb fits 32 bits
    f.n_content = bits ? next_u64() % (1ull << bits) : 0u;
    f.n_cb = (uint32_t)((f.n_content >> f.check_log) + ((f.n_content & ((1ull << f.check_log) - 1u)) ? 1u : 0u));
    f.content_crc = f.n_content ? (uint32_t)next_u64() : 0u;
    return f;
}

static int heads(int cases) {
    int accepted = 0;
    for (int cs = 0; cs < cases; ++cs) {
        uint8_t h[48];
        for (size_t i = 0; i < sizeof(h); ++i) h[i] = (uint8_t)next_u64();
        const uint32_t mode = (uint32_t)(next_u64() % 5u);
        size_t len = 32 + (size_t)(next_u64() % 17u);
        if (mode != 0) {  // mode 0: random bytes
            const fsehip_check_info f = valid_info();
            if (fsehip_check_write_header(&f, h) != FSE_OK) std::abort();
        }
        if (mode == 0 && next_u64() % 2u) std::memcpy(h, "FSEK\x01\x01", 6);  // random bytes behind a good start
        if (mode == 2) len = (size_t)(next_u64() % 32u);                        // truncated
        if (mode == 3) {  // one to three flipped bits, in different bytes
            const uint32_t at = (uint32_t)(next_u64() % 32u);
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[(at + 11u * k) % 32u] ^= (uint8_t)(1u << (next_u64() % 8u));
        }
        if (mode == 4) h[next_u64() % 32u] ^= (uint8_t)(1u + next_u64() % 255u);  // one changed byte
        uint8_t* buf = new uint8_t[len ? len : 1];  // exact size: ASan sees a read past len
        std::memcpy(buf, h, len);
        fsehip_check_info f;
        std::memset(&f, 0xEE, sizeof(f));
        const int rc = fsehip_check_read_header(len ? buf : nullptr, len, &f);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (mode == 1) CHECK(rc == FSE_OK);
        if (mode == 2 || mode == 3 || mode == 4) CHECK(rc == FSE_ERR_BAD_FRAME);  // header_crc sees every change
        if (rc == FSE_OK) {
            CHECK(f.version == 1 && f.algorithm == 1 && f.check_log >= 8 && f.check_log <= 16 && f.reserved == 0);
            CHECK(((uint64_t)f.n_cb << f.check_log) >= f.n_content);
            CHECK(f.n_cb == 0 || ((uint64_t)(f.n_cb - 1u) << f.check_log) < f.n_content);
            CHECK(f.header_crc == crc_bitwise(buf, 28));
            CHECK(fsehip_check_bytes(f.n_content, f.check_log) == 32u + 4ull * f.n_cb);
            uint8_t back[32];
            CHECK(fsehip_check_write_header(&f, back) == FSE_OK && std::memcmp(back, buf, 32) == 0);
            ++accepted;
        } else {
            CHECK(f.version == 0 && f.check_log == 0 && f.n_content == 0 && f.n_cb == 0 && f.header_crc == 0);
        }
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases) {
        std::fprintf(stderr, "FAIL: %d of %d heads accepted\n", accepted, cases);
        return 1;
    }
    return 0;
}

// sealed heads: a small record (n_cb <= 8) and the first bytes of a container
static int sealed(int cases) {
    int accepted = 0;
    for (int cs = 0; cs < cases; ++cs) {
        fsehip_check_info f;
        std::memset(&f, 0, sizeof(f));
        f.version = 1;
        f.algorithm = FSEHIP_CHECK_CRC32;
        f.check_log = 8 + (uint32_t)(next_u64() % 9u);
        const uint32_t kind = (uint32_t)(next_u64() % 3u);
        const uint32_t w = kind == 0 ? 1u : 1u << (next_u64() % 4u);
        const uint64_t n_elems = next_u64() % ((8ull << f.check_log) / w);
        f.n_content = n_elems * w;
        f.n_cb = (uint32_t)((f.n_content >> f.check_log) + ((f.n_content & ((1ull << f.check_log) - 1u)) ? 1u : 0u));
        f.content_crc = f.n_content ? (uint32_t)next_u64() : 0u;
        const size_t off = 32u + 4u * f.n_cb, inner = kind == 0 ? 32u : 48u;
        std::vector<uint8_t> h(off + inner);
        for (auto& b : h) b = (uint8_t)next_u64();
        if (fsehip_check_write_header(&f, h.data()) != FSE_OK) std::abort();
        uint8_t* in = h.data() + off;
        std::memcpy(in, kind == 0 ? "FSEF" : kind == 1 ? "FSEP" : "FSED", 4);
        if (kind == 0) {
            put64(in + 16, f.n_content);
        } else {
            in[5] = (uint8_t)w;
            put64(in + 8, n_elems);
        }
        const uint32_t mode = (uint32_t)(next_u64() % 4u);
        size_t len = h.size();
        if (mode == 1) len = (size_t)(next_u64() % h.size());                               // truncated
        if (mode == 2) h[next_u64() % h.size()] ^= (uint8_t)(1u << (next_u64() % 8u));      // one flipped bit
        if (mode == 3) put64(kind == 0 ? in + 16 : in + 8, (kind == 0 ? f.n_content : n_elems) + 1u);  // another length
        uint8_t* buf = new uint8_t[len ? len : 1];
        std::memcpy(buf, h.data(), len);
        fsehip_check_info g;
        uint32_t k = 77;
        uint64_t o = 77;
        std::memset(&g, 0xEE, sizeof(g));
        const int rc = fsehip_sealed_read_header(len ? buf : nullptr, len, &g, &k, &o);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (mode == 0) CHECK(rc == FSE_OK);
        if (mode == 1 || mode == 3) CHECK(rc == FSE_ERR_BAD_FRAME);
        if (rc == FSE_OK) {
            CHECK(k == kind && o == off && g.n_content == f.n_content && g.n_cb == f.n_cb);
            ++accepted;
        } else {
            CHECK(k == 0 && o == 0 && g.n_content == 0 && g.version == 0);
        }
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases) {
        std::fprintf(stderr, "FAIL: %d of %d sealed heads accepted\n", accepted, cases);
        return 1;
    }
    return 0;
}

static int crcs() {
    int cs = 0;
    CHECK(fsehip_crc32(0, nullptr, 0) == 0);
    for (size_t align = 0; align < 16; ++align)
        for (size_t n = 0; n <= 70; ++n, ++cs) {
            uint8_t* buf = new uint8_t[align + n ? align + n : 1];  // the data ends where the allocation ends
            for (size_t i = 0; i < align + n; ++i) buf[i] = (uint8_t)next_u64();
            if (next_u64() % 8u == 0) std::memset(buf, next_u64() % 2u ? 0xFF : 0, align + n);
            const uint8_t* p = buf + align;
            const uint32_t want = crc_bitwise(p, n);
            CHECK(fsehip_crc32(0, p, n) == want);
            const size_t cut = n ? (size_t)(next_u64() % (n + 1)) : 0;
            const uint32_t first = fsehip_crc32(0, p, cut), second = crc_bitwise(p + cut, n - cut);
            CHECK(fsehip_crc32(first, p + cut, n - cut) == want);
            CHECK(fsehip_crc32_combine(first, second, n - cut) == want);
            delete[] buf;
        }
    // the combine over lengths no buffer has: against itself in two steps
    for (cs = 0; cs < 200; ++cs) {
        const uint32_t a = (uint32_t)next_u64(), b = (uint32_t)next_u64(), c = (uint32_t)next_u64();
        const uint64_t lb = next_u64() >> (next_u64() % 64u), lc = next_u64() >> (1 + next_u64() % 63u);
        if (lb > UINT64_MAX - lc) continue;
        // (a || b) || c == a || (b || c)
        CHECK(fsehip_crc32_combine(fsehip_crc32_combine(a, b, lb), c, lc) ==
              fsehip_crc32_combine(a, fsehip_crc32_combine(b, c, lc), lb + lc));
    }
    return 0;
}

static int ranges(int cases) {
    for (int cs = 0; cs < cases; ++cs) {
        fsehip_check_info f;
        std::memset(&f, 0, sizeof(f));
        f.version = 1;
        f.algorithm = FSEHIP_CHECK_CRC32;
        f.check_log = 8 + (uint32_t)(next_u64() % 3u);
        f.n_content = next_u64() % 3000u;
        const uint64_t B = 1ull << f.check_log;
        f.n_cb = (uint32_t)((f.n_content + B - 1u) / B);
        f.content_crc = f.n_content ? 7u : 0u;
        uint8_t h[32];
        if (fsehip_check_write_header(&f, h) != FSE_OK || fsehip_check_read_header(h, 32, &f) != FSE_OK) std::abort();
        const uint32_t n_ranges = (uint32_t)(next_u64() % 5u);
        fsehip_frame_range* r = new fsehip_frame_range[n_ranges ? n_ranges : 1];  // exact size
        uint64_t want = 0;
        for (uint32_t i = 0; i < n_ranges; ++i) {
            uint64_t s = next_u64() % (f.n_content + 1u), e = next_u64() % (f.n_content + 1u);
            if (next_u64() % 3u == 0) s = s / B * B;  // on a block's edge, or one off it
            if (next_u64() % 3u == 0) e = e / B * B + (next_u64() % 3u) - 1u;
            if (next_u64() % 4u == 0) e = f.n_content;
            if (e > f.n_content) e = f.n_content;
            if (e < s) { const uint64_t t = s; s = e; e = t; }
            r[i] = fsehip_frame_range{s, e - s, next_u64()};
            // per byte: a block counts when the range holds every one of its content bytes
            for (uint64_t b = 0; b < f.n_cb; ++b) {
                const uint64_t lo = b * B, hi = (b + 1u) * B < f.n_content ? (b + 1u) * B : f.n_content;
                bool all = e > s;
                for (uint64_t x = lo; x < hi; ++x) all = all && x >= s && x < e;
                if (all) want += hi - lo;
            }
        }
        uint64_t got = 77;
        CHECK(fsehip_check_ranges_verified_bytes(&f, n_ranges ? r : nullptr, n_ranges, &got) == FSE_OK);
        CHECK(got == want);
        if (n_ranges) {
            r[0].len = f.n_content - r[0].src_off + 1u;  // one byte past the end
            CHECK(fsehip_check_ranges_verified_bytes(&f, r, n_ranges, &got) == FSE_ERR_BAD_ARG && got == 0);
            r[0].src_off = UINT64_MAX;
            r[0].len = 2;
            CHECK(fsehip_check_ranges_verified_bytes(&f, r, n_ranges, &got) == FSE_ERR_BAD_ARG);
        }
        delete[] r;
    }
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    if (heads(cases) || sealed(cases / 4) || crcs() || ranges(cases / 4)) return 1;
    std::printf("ok %d cases\n", cases);
    return 0;
}
