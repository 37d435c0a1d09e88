// Fuzz of the host code of the estimate with a base (entropy_coders_amd/csrc/
// fse_estimate.cpp, include/fsehip.h section 2i), built alone by
// tests/test_estimate_diff_sanitized.py with AddressSanitizer + UBSan.  The
// five estimates are read from a heap buffer of exactly 40 bytes, so a read
// past them stops the run.  fsehip_estimate_choose_base is held against the
// tie rule written out again, fsehip_estimate_base_scratch_bytes against its
// formula in 128-bit integers, on random and degenerate inputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/fsehip.h"

static uint64_t rng_state = 0xD1FFE57100000001ull;
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

static bool width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// frame, planes, delta, diff: the order ties are settled in
static const int ORDER[4] = {0, 1, 2, 4};

static int ref_choose(const uint64_t* est) {
    int best = -1;
    for (int i = 0; i < 4; ++i) {
        const int k = ORDER[i];
        if (est[k] == FSEHIP_EST_NONE) continue;
        if (best < 0 || est[k] < est[best]) best = k;  // strictly: an equal later kind loses
    }
    return best;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    int cs = -1;

    CHECK(fsehip_estimate_choose_base(nullptr) == -1);
    {
        uint64_t* est = (uint64_t*)std::malloc(5 * sizeof(uint64_t));
        for (int k = 0; k < 5; ++k) est[k] = FSEHIP_EST_NONE;
        CHECK(fsehip_estimate_choose_base(est) == -1);
        est[3] = 0;  // a sealed buffer is no choice of container
        CHECK(fsehip_estimate_choose_base(est) == -1);
        est[4] = 7;
        CHECK(fsehip_estimate_choose_base(est) == 4);
        est[2] = 7;
        CHECK(fsehip_estimate_choose_base(est) == 2);
        est[0] = est[1] = 7;
        CHECK(fsehip_estimate_choose_base(est) == 0);
        est[4] = 6;
        CHECK(fsehip_estimate_choose_base(est) == 4);
        std::free(est);
    }

    for (cs = 0; cs < cases; ++cs) {
        // ---- the choice
        {
            uint64_t* est = (uint64_t*)std::malloc(5 * sizeof(uint64_t));
            for (int k = 0; k < 5; ++k) {
                const uint64_t r = next_u64();
                est[k] = r % 4 == 0 ? FSEHIP_EST_NONE : r % 4 == 1 ? 1000 + (r >> 8) % 3 : r >> (r % 60);
            }
            const int got = fsehip_estimate_choose_base(est);
            CHECK(got == ref_choose(est));
            CHECK(got != 3);
            if (est[4] == FSEHIP_EST_NONE) CHECK(got == fsehip_estimate_choose(est));  // the three-entry form's answer
            std::free(est);
        }
        // ---- the scratch
        {
            const uint32_t w = next_u64() % 8 ? 1u << (next_u64() % 4) : (uint32_t)(next_u64() % 20);
            const uint32_t bits = (uint32_t)(next_u64() % 65);
            const uint64_t n = bits == 0 ? 0 : bits == 64 ? next_u64() : next_u64() % (1ull << bits);
            const uint32_t mask = next_u64() % 16 ? (uint32_t)(next_u64() % 40) : (uint32_t)next_u64();
            const uint32_t bs = next_u64() % 4 ? 16u << (next_u64() % 24) : (uint32_t)(next_u64() % 5000);
            const uint64_t b = bs ? bs : 65536;
            const uint64_t got = fsehip_estimate_base_scratch_bytes(n, w, mask, bs);
            if (mask == 0 || (mask & ~23u) || !width_ok(w)) {
                CHECK(got == 0);
                continue;
            }
            const u128 stride = ((u128)n + 15) / 16 * 16;
            u128 most = 0;
            bool overflow = false;
            for (int i = 0; i < 4; ++i) {
                const int k = ORDER[i];
                if (!(mask >> k & 1) || (k == 1 && w == 1)) continue;
                const u128 img = k == 0 ? (u128)n * w : stride * w;
                if (img > UINT64_MAX || (k && (u128)n + 15 > UINT64_MAX)) overflow = true;
                const u128 nb = (img + b - 1) / b;
                most = nb > most ? nb : most;
            }
            if (overflow || most * 1024 > UINT64_MAX) CHECK(got == 0);
            else CHECK(got == (uint64_t)(most * 1024));
            if (!(mask & 16u)) CHECK(got == fsehip_estimate_scratch_bytes(n, w, mask, bs));
        }
    }
    std::printf("ok %d cases\n", cases);
    return 0;
}
