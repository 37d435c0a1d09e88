// Fuzz of the size estimate's host code (entropy_coders_amd/csrc/
// fse_estimate.cpp, include/fsehip.h section 2g), built alone by
// tests/test_estimate_sanitized.py with AddressSanitizer + UBSan.  Count and
// table arrays, the estimates and the magics are read from heap buffers
// allocated to their exact size, so a read past them or an undefined shift
// stops the run.  fsehip_log2q8 is held against a 128-bit restatement and
// against log2 itself for every count; fsehip_estimate_block_host against the
// rule written out again on random and degenerate tables; the choice, the
// kind and the sizes against plain restatements.
#include <cmath>
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

typedef unsigned __int128 u128;

static uint32_t ref_log2q8(uint32_t c) {
    uint32_t hb = 0;
    while ((c >> (hb + 1)) != 0) ++hb;
    u128 x = (u128)c << (31 - hb);
    uint32_t y = hb;
    for (int i = 0; i < 8; ++i) {
        x = (x * x) >> 31;
        y <<= 1;
        if (x >> 32) {
            x >>= 1;
            y |= 1;
        }
    }
    return y;
}

static uint32_t kernel_class(uint32_t table_log, uint32_t max_table_log) {
    uint32_t m = max_table_log ? max_table_log : (table_log == 0 || table_log < 11 ? 11 : table_log);
    return m <= 11 ? 11 : m >= 15 ? 15 : m;
}

static bool width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }

static u128 image_bytes(uint32_t kind, uint64_t n, uint32_t w) {
    if (kind == 0) return (u128)n * w;
    return (((u128)n + 15) / 16 * 16) * w;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int cs = -1;

    // ---- the logarithm, every count
    for (uint32_t c = 1; c <= 32768; ++c) {
        const uint32_t y = fsehip_log2q8(c);
        CHECK(y == ref_log2q8(c));
        CHECK(std::fabs((double)y - 256.0 * std::log2((double)c)) <= 1.01);
        if ((c & (c - 1)) == 0) CHECK(y == 256u * (uint32_t)std::lround(std::log2((double)c)));
    }
    CHECK(fsehip_log2q8(0) == 0 && fsehip_log2q8(32769) == 0 && fsehip_log2q8(0xFFFFFFFFu) == 0);

    for (cs = 0; cs < cases; ++cs) {
        // ---- the choice
        {
            uint64_t* est = (uint64_t*)std::malloc(3 * sizeof(uint64_t));
            int want = -1;
            for (int k = 0; k < 3; ++k) {
                const uint64_t r = next_u64();
                est[k] = r % 4 == 0 ? FSEHIP_EST_NONE : r % 4 == 1 ? 1000 + (r >> 8) % 3 : r >> (r % 60);
            }
            for (int k = 0; k < 3; ++k)
                if (est[k] != FSEHIP_EST_NONE && (want < 0 || est[k] < est[want])) want = k;
            CHECK(fsehip_estimate_choose(est) == want);
            std::free(est);
        }
        // ---- the kind, from buffers of 0..8 bytes
        {
            const size_t len = next_u64() % 9;
            uint8_t* b = (uint8_t*)std::malloc(len ? len : 1);
            for (size_t i = 0; i < len; ++i) b[i] = (uint8_t)next_u64();
            if (len >= 4 && next_u64() % 2) {
                std::memcpy(b, "FSE", 3);
                b[3] = "FPDKX\0f"[next_u64() % 7];
            }
            const int k = fsehip_container_kind(len ? b : nullptr, len);
            int want = FSE_ERR_BAD_FRAME;
            if (len >= 4 && b[0] == 'F' && b[1] == 'S' && b[2] == 'E')
                want = b[3] == 'F' ? 0 : b[3] == 'P' ? 1 : b[3] == 'D' ? 2 : b[3] == 'K' ? 3 : FSE_ERR_BAD_FRAME;
            CHECK(k == want);
            std::free(b);
        }
        // ---- the sizes
        {
            const uint32_t w = next_u64() % 8 ? 1u << (next_u64() % 4) : (uint32_t)(next_u64() % 20);
            const uint32_t bits = (uint32_t)(next_u64() % 65);
            const uint64_t n = bits == 0 ? 0 : bits == 64 ? next_u64() : next_u64() % (1ull << bits);
            const uint32_t mask = (uint32_t)(next_u64() % 10);
            const uint32_t bs = next_u64() % 4 ? 16u << (next_u64() % 24) : (uint32_t)(next_u64() % 5000);
            const uint64_t b = bs ? bs : 65536;
            u128 most = 0;
            bool bad = mask == 0 || mask > 7 || !width_ok(w);
            for (uint32_t k = 0; k < 3 && !bad; ++k) {
                const u128 img = image_bytes(k, n, w);
                const bool none = k == 1 && w == 1;
                const uint64_t got = fsehip_estimate_image_bytes(k, n, w);
                if (none || img > UINT64_MAX || (k && (u128)n + 15 > UINT64_MAX)) {
                    CHECK(got == 0);
                    if (!none && (mask >> k & 1)) bad = true;
                    continue;
                }
                CHECK(got == (uint64_t)img);
                if (mask >> k & 1) {
                    const u128 nb = (img + b - 1) / b;
                    most = nb > most ? nb : most;
                }
            }
            const uint64_t got = fsehip_estimate_scratch_bytes(n, w, mask, bs);
            if (bad || most * 1024 > UINT64_MAX) CHECK(got == 0);
            else CHECK(got == (uint64_t)(most * 1024));
            CHECK(fsehip_estimate_image_bytes(3 + (uint32_t)(next_u64() % 100), n, w) == 0);
        }
        // ---- one block against the rule written out again
        {
            uint32_t* counts = (uint32_t*)std::calloc(256, sizeof(uint32_t));
            int32_t* norm = (int32_t*)std::calloc(256, sizeof(int32_t));
            const uint32_t L = 5 + (uint32_t)(next_u64() % 11);
            const uint32_t nsym = 1 + (uint32_t)(next_u64() % (next_u64() % 2 ? 4 : 256));
            const uint32_t top = next_u64() % 3 == 0 ? 1u << 28 : 1u << (next_u64() % 18);
            uint64_t raw = 0;
            for (uint32_t i = 0; i < nsym; ++i) {
                const uint32_t s = next_u64() % 4 == 0 ? i : (uint32_t)(next_u64() % 256);
                const uint32_t c = 1 + (uint32_t)(next_u64() % top);
                if (raw + c > (1u << 28)) break;
                raw = raw - counts[s] + c;
                counts[s] = c;
                norm[s] = next_u64() % 5 == 0 ? -1 : 1 + (int32_t)(next_u64() % (1u << L));
            }
            const int mode = (int)(next_u64() % 8);  // 0: all zeros (RLE), 1: a bad table entry, 2: no table
            if (mode == 0) {
                std::memset(counts, 0, 1024);
                counts[0] = (uint32_t)raw;
            }
            int bad_sym = -1;
            if (mode == 1)
                for (int s = 255; s >= 1; --s)
                    if (counts[s]) {
                        bad_sym = s;
                        norm[s] = next_u64() % 3 == 0 ? 0 : next_u64() % 2 ? (int32_t)(1u << L) + 1 : -2;
                        break;
                    }
            fsehip_frame_params p;
            std::memset(&p, 0, sizeof(p));
            p.table_log = next_u64() % 2 ? 0 : (uint32_t)(next_u64() % 17);
            p.max_table_log = next_u64() % 2 ? 0 : (uint32_t)(next_u64() % 17);
            p.ckpt_interval = next_u64() % 2 ? 0 : 8u << (next_u64() % 8);
            p.nstates = (uint32_t)(next_u64() % 4);
            const uint32_t hdr = (uint32_t)(next_u64() % 513);
            fsehip_block_estimate e;
            std::memset(&e, 0xEE, sizeof(e));
            const int32_t* table = mode == 2 ? nullptr : norm;
            const int rc = fsehip_estimate_block_host(counts, (uint32_t)raw, table, L, hdr, &p, &e);
            const uint32_t ns = p.nstates == 1 ? 1 : 2;
            const bool rle = raw && counts[0] == raw;
            if (p.nstates > 2) {
                CHECK(rc == FSE_ERR_BAD_ARG);
            } else if (rle) {
                CHECK(rc == FSE_OK && e.type == FSEHIP_EST_RLE && e.rec == 1 && e.bits == 0 && e.table_log == 0);
            } else if (mode == 2 || raw < 2) {
                CHECK(rc == FSE_OK && e.type == FSEHIP_EST_RAW && e.rec == raw && e.bits == 0 && e.table_log == 0);
            } else if (bad_sym >= 0) {
                CHECK(rc == FSE_ERR_BAD_ARG);
            } else {
                u128 Q = 0;
                for (int s = 0; s < 256; ++s)
                    if (counts[s]) Q += (u128)counts[s] * (256u * L - ref_log2q8(norm[s] < 1 ? 1 : (uint32_t)norm[s]));
                const u128 bits = ((Q + 255) >> 8) + ns * L + 1;
                const uint32_t spb = p.ckpt_interval == 0 ? 0
                                     : ns == 1           ? (uint32_t)raw / p.ckpt_interval + 2
                                                         : (uint32_t)raw / 2 / p.ckpt_interval + 2;
                const u128 rec = hdr + (bits + 7) / 8 + 8ull * spb;
                CHECK(rc == FSE_OK);
                if (L <= kernel_class(p.table_log, p.max_table_log) && rec < raw) {
                    CHECK(e.type == FSEHIP_EST_FSE && e.table_log == L);
                    CHECK(e.rec == (uint64_t)rec && e.bits == (uint64_t)bits);
                } else {
                    CHECK(e.type == FSEHIP_EST_RAW && e.rec == raw && e.bits == 0 && e.table_log == 0);
                }
            }
            CHECK(fsehip_estimate_block_host(nullptr, 1, norm, L, hdr, &p, &e) == FSE_ERR_BAD_ARG);
            CHECK(fsehip_estimate_block_host(counts, 1, norm, L, hdr, nullptr, &e) == FSE_ERR_BAD_ARG);
            CHECK(fsehip_estimate_block_host(counts, 1, norm, L, hdr, &p, nullptr) == FSE_ERR_BAD_ARG);
            std::free(counts);
            std::free(norm);
        }
    }
    std::printf("ok %d cases\n", cases);
    return 0;
}
