// Fuzz of the frame's host code (entropy_coders_amd/csrc/fse_frame.cpp,
// include/fsehip.h section 2b), built by tests/test_frame_sanitized.py with
// AddressSanitizer + UBSan: valid, random, truncated and bit-flipped headers
// are parsed from heap buffers allocated to their exact size, so a read past
// `len` or an undefined shift stops the run.  Every result must be FSE_OK
// with all fields inside their ranges (and then the writer reproduces the 32
// bytes), or FSE_ERR_BAD_FRAME.
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

static bool in_range(const fsehip_frame_info& f) {
    if (f.version != 1 || f.nstates < 1 || f.nstates > 2 || f.max_table_log < 11 || f.max_table_log > 15) return false;
    if ((f.flags & ~1u) || f.reserved || f.block_size < 1 || f.block_size > (1u << 28)) return false;
    if (f.flags) {
        if (f.ckpt_interval < (f.nstates == 1 ? 16u : 8u) || (f.ckpt_interval & (f.ckpt_interval - 1))) return false;
    } else if (f.ckpt_interval) {
        return false;
    }
    const uint64_t nb = f.n_total / f.block_size + (f.n_total % f.block_size != 0);
    if (nb != f.n_blocks || (f.n_blocks > 1 && (f.block_size & 15u))) return false;
    return f.records_off == 32 + 4ull * f.n_blocks;
}

// a header that passes every rule
static void valid_header(uint8_t out[32]) {
    fsehip_frame_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.nstates = 1 + (uint32_t)(next_u64() % 2u);
    f.max_table_log = 11 + (uint32_t)(next_u64() % 5u);
    f.flags = (uint32_t)(next_u64() % 2u);
    f.ckpt_interval = f.flags ? 1u << (4 + next_u64() % 10u) : 0u;
    const uint32_t shift = (uint32_t)(next_u64() % 25u);
    f.block_size = 16u << shift;
    if (next_u64() % 4u == 0) f.block_size = 1 + (uint32_t)(next_u64() % 70000u);  // odd sizes: one block at most
    const uint64_t max_total = (f.block_size & 15u) ? f.block_size : (uint64_t)f.block_size * 0xFFFFFFFFull;
    f.n_total = next_u64() % 8u == 0 ? max_total : next_u64() % (max_total + 1u);
    if (next_u64() % 3u == 0) f.n_total %= 1u << 20;
    f.n_blocks = (uint32_t)(f.n_total / f.block_size + (f.n_total % f.block_size != 0));
    if (fsehip_frame_write_header(&f, out) != FSE_OK) std::abort();
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int accepted = 0;
    for (int cs = 0; cs < cases; ++cs) {
        uint8_t h[48];
        for (size_t i = 0; i < sizeof(h); ++i) h[i] = (uint8_t)next_u64();
        const uint32_t mode = (uint32_t)(next_u64() % 5u);
        size_t len = 32 + (size_t)(next_u64() % 17u);
        if (mode != 0) valid_header(h);  // mode 0: random bytes
        if (mode == 2) len = (size_t)(next_u64() % 32u);  // truncated
        if (mode == 3) {  // one to three flipped bits
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[next_u64() % 32u] ^= (uint8_t)(1u << (next_u64() % 8u));
        }
        if (mode == 4) h[next_u64() % 32u] = (uint8_t)next_u64();  // one replaced byte
        uint8_t* buf = new uint8_t[len ? len : 1];  // exact size: ASan sees a read past len
        std::memcpy(buf, h, len);
        fsehip_frame_info f;
        std::memset(&f, 0xEE, sizeof(f));
        const int rc = fsehip_frame_read_header(len ? buf : nullptr, len, &f);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (mode == 1) CHECK(rc == FSE_OK);
        if (mode == 2) CHECK(rc == FSE_ERR_BAD_FRAME);
        if (rc == FSE_OK) {
            CHECK(in_range(f));
            uint8_t back[32];
            CHECK(fsehip_frame_write_header(&f, back) == FSE_OK);
            CHECK(std::memcmp(back, buf, 32) == 0);
            const uint64_t bound = fsehip_frame_bound(f.n_total, f.block_size);
            CHECK(bound == f.records_off + f.n_total || bound < f.n_total /* u64 wrap */);
            ++accepted;
        }
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases) {
        std::fprintf(stderr, "FAIL: %d of %d headers accepted\n", accepted, cases);
        return 1;
    }
    std::printf("ok %d cases, %d accepted\n", cases, accepted);
    return 0;
}
