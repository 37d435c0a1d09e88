// Fuzz of the versioned pack's host code (entropy_coders_amd/csrc/fse_pack.cpp
// with both flavours, over fse_frame.cpp; include/fsehip.h sections 2j and
// 2k), built by tests/test_vpack_sanitized.py with AddressSanitizer + UBSan.
//
// Part 1: valid, random, truncated and damaged heads are parsed by the readers
// of BOTH containers from heap buffers allocated to their exact size.  Every
// result is FSE_OK with all fields in range or FSE_ERR_BAD_FRAME with the
// outputs zeroed; at most one of the two readers accepts a buffer; the pack
// frame's reader never returns a diff member; what the versioned reader
// accepts is written back byte for byte, sized consistently and planned with
// the exported plane offsets.
//
// Part 2: the pointer checks of the device calls (pack_bases_ok,
// pack_decode_spans_ok) on random member lists, selections, destinations and
// bases laid out in a small address range so that overlaps are common,
// against a quadratic restatement of the rule: no destination shares a byte
// with another destination or with a decoded diff member's base, except a
// diff member's destination that is its base itself.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../entropy_coders_amd/csrc/fse_pack_host.h"
#include "../../include/fsehip.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

static const uint32_t kKinds[3] = {FSEHIP_KIND_PLANES, FSEHIP_KIND_DELTA, FSEHIP_KIND_DIFF};

// a member list valid for the versioned pack; `diff`: diff members among them
static std::vector<fsehip_pack_member> valid_members(bool diff, bool huge) {
    std::vector<fsehip_pack_member> v((size_t)(next_u64() % 40u));
    for (fsehip_pack_member& m : v) {
        m.d_ptr = nullptr;
        m.kind = kKinds[next_u64() % (diff ? 3u : 2u)];
        m.elem_bytes = 1u << (next_u64() % 4u);
        const uint32_t bits = (uint32_t)(next_u64() % (huge ? 41u : 14u));
        m.n_elems = bits ? next_u64() % (1ull << bits) : 0u;
    }
    return v;
}

static std::vector<uint8_t> valid_head(const std::vector<fsehip_pack_member>& v) {
    const uint32_t n = (uint32_t)v.size();
    std::vector<uint8_t> out(32u + 16u * n + 32u);
    if (fsehip_vpack_write_header(v.data(), n, out.data()) != FSE_OK) std::abort();
    fsehip_frame_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.nstates = 1 + (uint32_t)(next_u64() % 2u);
    f.max_table_log = 11 + (uint32_t)(next_u64() % 5u);
    f.flags = (uint32_t)(next_u64() % 2u);
    f.ckpt_interval = f.flags ? 1u << (4 + next_u64() % 10u) : 0u;
    f.n_total = fsehip_vpack_image_bytes(v.data(), n);
    f.block_size = 16u << (12 + next_u64() % 13u);
    f.n_blocks = (uint32_t)(f.n_total / f.block_size + (f.n_total % f.block_size != 0));
    if (fsehip_frame_write_header(&f, out.data() + 32u + 16u * n) != FSE_OK) std::abort();
    return out;
}

static int fuzz_heads(int cases) {
    int accepted = 0, accepted_pack = 0;
    for (int cs = 0; cs < cases; ++cs) {
        const uint32_t mode = (uint32_t)(next_u64() % 7u);
        const bool diff = next_u64() % 4u != 0;
        const std::vector<fsehip_pack_member> v = valid_members(diff, next_u64() % 2u);
        const uint32_t n = (uint32_t)v.size();
        std::vector<uint8_t> h = valid_head(v);
        const size_t full = h.size();
        size_t len = full + (size_t)(next_u64() % 17u);
        h.resize(len);
        for (size_t i = full; i < len; ++i) h[i] = (uint8_t)next_u64();
        if (mode == 0) {  // random bytes, most of them behind one of the two magics
            for (size_t i = 0; i < len; ++i) h[i] = (uint8_t)next_u64();
            const uint32_t pick = (uint32_t)(next_u64() % 3u);
            if (pick) std::memcpy(h.data(), pick == 1 ? "FSEV\x01\0\0\0" : "FSEM\x01\0\0\0", 8);
            if (next_u64() % 2u) h[10] = h[11] = 0;
        }
        if (mode == 2) len = (size_t)(next_u64() % full);  // truncated
        if (mode == 3)
            for (uint32_t k = 1 + (uint32_t)(next_u64() % 3u); k; --k) h[next_u64() % full] ^= (uint8_t)(1u << (next_u64() % 8u));
        if (mode == 4 && n) h[32 + 16 * (next_u64() % n)] = (uint8_t)(next_u64() % 8u);  // another kind byte
        if (mode == 5) h[3] = 'M';  // the same head under the pack frame's magic
        if (mode == 6) {
            const uint32_t more = n + 1u + (uint32_t)(next_u64() % (next_u64() % 2u ? 4u : 1u << 21));
            for (int i = 0; i < 4; ++i) h[8 + i] = (uint8_t)(more >> (8 * i));
        }
        uint8_t* buf = new uint8_t[len ? len : 1];
        std::memcpy(buf, h.data(), len);
        int rcs[2];
        for (int fl = 0; fl < 2; ++fl) {  // 0: the versioned pack's readers, 1: the pack frame's
            fsehip_pack_info p, p2;
            fsehip_frame_info f;
            std::memset(&p, 0xEE, sizeof(p));
            std::memset(&p2, 0xEE, sizeof(p2));
            std::memset(&f, 0xEE, sizeof(f));
            const int rc0 = fl ? fsehip_pack_read_header(len ? buf : nullptr, len, &p2)
                               : fsehip_vpack_read_header(len ? buf : nullptr, len, &p2);
            CHECK(rc0 == FSE_OK || rc0 == FSE_ERR_BAD_FRAME);
            if (rc0 != FSE_OK) CHECK(p2.n_members == 0 && p2.image_bytes == 0 && p2.version == 0);
            else CHECK(p2.version == 1 && p2.n_members <= FSEHIP_PACK_MAX_MEMBERS);
            const uint32_t cap = rc0 == FSE_OK && len >= 64u && p2.n_members <= (len - 64u) / 16u ? p2.n_members : n;
            fsehip_pack_member* got = new fsehip_pack_member[cap ? cap : 1];
            const int rc = fl ? fsehip_pack_read_members(len ? buf : nullptr, len, got, cap, &p, &f)
                              : fsehip_vpack_read_members(len ? buf : nullptr, len, got, cap, &p, &f);
            rcs[fl] = rc;
            CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME || (rc == FSE_ERR_DST_TOO_SMALL && mode != 1));
            if (mode == 1) CHECK(rc == (fl ? FSE_ERR_BAD_FRAME : FSE_OK));
            if (mode == 2 || mode == 6) CHECK(rc != FSE_OK);
            if (mode == 5) CHECK(fl ? (rc == FSE_OK) == !std::any_of(v.begin(), v.end(), [](const fsehip_pack_member& m) {
                return m.kind == FSEHIP_KIND_DIFF;
            }) : rc == FSE_ERR_BAD_FRAME);
            if (rc0 != FSE_OK) CHECK(rc == FSE_ERR_BAD_FRAME);
            if (rc == FSE_OK) {
                const uint32_t k = p.n_members;
                CHECK(p.version == 1 && k <= cap && len >= 64u + 16u * (size_t)k);
                CHECK(std::memcmp(buf, fl ? "FSEM" : "FSEV", 4) == 0);
                uint64_t image = 0, content = 0;
                for (uint32_t m = 0; m < k; ++m) {
                    CHECK(got[m].d_ptr == nullptr);
                    CHECK(got[m].kind == 1 || got[m].kind == 2 || (!fl && got[m].kind == 4));
                    CHECK(got[m].elem_bytes == 1 || got[m].elem_bytes == 2 || got[m].elem_bytes == 4 || got[m].elem_bytes == 8);
                    CHECK(got[m].n_elems <= UINT64_MAX - 15u);
                    const uint64_t stride = (got[m].n_elems + 15u) & ~15ull;
                    CHECK(stride <= (UINT64_MAX - image) / got[m].elem_bytes);
                    image += stride * got[m].elem_bytes;
                    content += got[m].n_elems * got[m].elem_bytes;
                }
                CHECK(p.image_bytes == image && p.content_bytes == content && f.n_total == image);
                if (!fl) {
                    std::vector<uint8_t> back(32u + 16u * (size_t)k + 32u);
                    CHECK(fsehip_vpack_write_header(got, k, back.data()) == FSE_OK);
                    CHECK(fsehip_frame_write_header(&f, back.data() + 32u + 16u * (size_t)k) == FSE_OK);
                    CHECK(std::memcmp(back.data(), buf, back.size()) == 0);
                    CHECK(fsehip_vpack_image_bytes(got, k) == image);
                    const uint64_t head = 32u + 16u * (uint64_t)k;
                    const uint64_t scratch = fsehip_vpack_scratch_bytes(got, k);
                    CHECK(scratch % 16u == 0 && scratch >= image + (sizeof(fsehip::PackDesc) + 8u) * k + head);
                    std::vector<fsehip::PackDesc> d(k ? k : 1);
                    const uint64_t tiles = fsehip::pack_plan(got, k, d.data());
                    uint64_t want_tiles = 0;
                    for (uint32_t m = 0; m < k; ++m) {
                        CHECK(d[m].first_tile == want_tiles && d[m].kind == got[m].kind && d[m].w == got[m].elem_bytes);
                        want_tiles += (got[m].n_elems + 4095u) / 4096u;
                        for (uint32_t b = 0; b < got[m].elem_bytes; ++b)
                            CHECK(d[m].plane[b] == fsehip_vpack_plane_offset(got, k, m, b) && d[m].plane[b] % 16u == 0);
                    }
                    CHECK(tiles == want_tiles);
                    // a list without diff members: the pack frame's head differs in its magic only
                    const bool any_diff = std::any_of(got, got + k, [](const fsehip_pack_member& m) { return m.kind == 4; });
                    std::vector<uint8_t> as_pack(head ? head : 1);
                    const int wrc = fsehip_pack_write_header(got, k, as_pack.data());
                    CHECK(wrc == (any_diff ? FSE_ERR_BAD_ARG : FSE_OK));
                    if (!any_diff) CHECK(std::memcmp(as_pack.data() + 4, buf + 4, head - 4u) == 0 && as_pack[3] == 'M');
                    // random selections plan inside the scratch they are promised
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
                    const int src = fsehip::pack_plan_selected(got, k, sel.data(), (uint32_t)sel.size(), &sd, &fr,
                                                               &planes_bytes, &sel_tiles);
                    CHECK(src == (valid ? FSE_OK : FSE_ERR_BAD_ARG));
                    const uint64_t need = fsehip_vpack_members_scratch_bytes(got, k, sel.data(), (uint32_t)sel.size());
                    if (valid)
                        CHECK(need >= planes_bytes + 4u * fr.size() + (sizeof(fsehip::PackDesc) + 8u) * sel.size() + head);
                    ++accepted;
                } else {
                    ++accepted_pack;
                }
            } else {
                CHECK(p.n_members == 0 && p.image_bytes == 0 && p.content_bytes == 0 && f.n_total == 0);
            }
            delete[] got;
        }
        CHECK(!(rcs[0] == FSE_OK && rcs[1] == FSE_OK));  // one magic, one reader
        delete[] buf;
    }
    if (accepted == 0 || accepted == cases || accepted_pack == 0) {
        std::fprintf(stderr, "FAIL: %d and %d of %d heads accepted\n", accepted, accepted_pack, cases);
        return 1;
    }
    std::printf("ok heads: %d cases, %d versioned and %d pack heads accepted\n", cases, accepted, accepted_pack);
    return 0;
}

static bool meet(uintptr_t a, uintptr_t an, uintptr_t b, uintptr_t bn) { return a < b + bn && b < a + an; }

static int fuzz_spans(int cases) {
    int refused = 0, passed = 0, in_place_ok = 0;
    for (int cs = 0; cs < cases; ++cs) {
        const uint32_t n = 1u + (uint32_t)(next_u64() % 12u);
        const uintptr_t span = 64u << (next_u64() % 6u);  // a crowded or a roomy address range
        std::vector<fsehip_pack_member> v(n);
        std::vector<const void*> bases(n);
        for (uint32_t m = 0; m < n; ++m) {
            v[m].kind = kKinds[next_u64() % 3u];
            v[m].elem_bytes = 1u << (next_u64() % 4u);
            v[m].n_elems = next_u64() % 4u ? 1u + next_u64() % 6u : 0u;
            const uintptr_t w = v[m].elem_bytes;
            v[m].d_ptr = reinterpret_cast<void*>(0x10000u + (next_u64() % span) / w * w);
            const uint32_t how = (uint32_t)(next_u64() % 8u);
            uintptr_t b = 0x10000u + (next_u64() % span) / w * w;
            if (how < 3) b = reinterpret_cast<uintptr_t>(v[m].d_ptr);  // in place
            if (how == 3) b = 0x80000u + 64u * m;                      // far away
            if (how == 4) b += 1;                                      // maybe misaligned
            if (how == 5) b = 0;                                       // missing
            bases[m] = reinterpret_cast<const void*>(b);
        }
        // spread the destinations in half of the cases, so that passes are common too
        if (next_u64() % 2u)
            for (uint32_t m = 0; m < n; ++m) {
                const bool same = bases[m] == v[m].d_ptr;
                v[m].d_ptr = reinterpret_cast<void*>(0x20000u + 64u * m);
                if (same) bases[m] = v[m].d_ptr;
            }
        std::vector<uint32_t> sel;
        const bool all = next_u64() % 2u;
        if (!all) {
            for (uint32_t m = 0; m < n; ++m)
                if (next_u64() % 2u) sel.push_back(m);
            for (size_t i = sel.size(); i > 1; --i) std::swap(sel[i - 1], sel[next_u64() % i]);
        }
        const uint32_t* idx = all ? nullptr : sel.data();
        const uint32_t cnt = all ? n : (uint32_t)sel.size();
        const bool null_bases = next_u64() % 8u == 0;
        const void* const* bp = null_bases ? nullptr : bases.data();
        // the rule, restated pair by pair
        bool want_bases = true, want_spans = true, any_in_place = false;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t m = idx ? idx[i] : i;
            const bool needs = v[m].kind == FSEHIP_KIND_DIFF && v[m].n_elems;
            CHECK(fsehip::pack_needs_base(v[m]) == needs);
            if (needs && (null_bases || !bases[m] || reinterpret_cast<uintptr_t>(bases[m]) % v[m].elem_bytes))
                want_bases = false;
        }
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t m = idx ? idx[i] : i;
            if (!v[m].n_elems) continue;
            const uintptr_t d = reinterpret_cast<uintptr_t>(v[m].d_ptr), dn = v[m].n_elems * v[m].elem_bytes;
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t o = idx ? idx[j] : j;
                if (!v[o].n_elems) continue;
                if (o != m && meet(d, dn, reinterpret_cast<uintptr_t>(v[o].d_ptr), v[o].n_elems * v[o].elem_bytes))
                    want_spans = false;
                if (null_bases || v[o].kind != FSEHIP_KIND_DIFF) continue;
                const uintptr_t b = reinterpret_cast<uintptr_t>(bases[o]);
                if (o == m && b == d) {
                    any_in_place = true;
                    continue;
                }
                if (meet(d, dn, b, v[o].n_elems * v[o].elem_bytes)) want_spans = false;
            }
        }
        CHECK(fsehip::pack_bases_ok(v.data(), bp, idx, cnt) == want_bases);
        // the device calls ask about the spans only after the bases passed
        if (want_bases) {
            CHECK(fsehip::pack_decode_spans_ok(v.data(), bp, idx, cnt) == want_spans);
            (want_spans ? passed : refused) += 1;
            if (want_spans && any_in_place) ++in_place_ok;
        }
    }
    if (!refused || !passed || !in_place_ok) {
        std::fprintf(stderr, "FAIL: %d refused, %d passed, %d of them in place\n", refused, passed, in_place_ok);
        return 1;
    }
    std::printf("ok spans: %d cases, %d refused, %d passed, %d of them with an in-place member\n", cases, refused, passed,
                in_place_ok);
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    if (fuzz_heads(cases)) return 1;
    return fuzz_spans(4 * cases);
}
