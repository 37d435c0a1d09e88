// Fuzz of the member check record's and the sealed pack's host code
// (entropy_coders_amd/csrc/fse_mcheck.cpp over fse_pack.cpp, fse_check.cpp and
// fse_frame.cpp; include/fsehip.h section 2l), built by
// tests/test_spack_sanitized.py with AddressSanitizer + UBSan.
//
// Part 1: valid, random, truncated and damaged heads are parsed by
// fsehip_mcheck_read_header and fsehip_spack_read_header from heap buffers
// allocated to their exact size.  Every result is FSE_OK with all fields in
// range or FSE_ERR_BAD_FRAME with the outputs zeroed; what is accepted is
// written back byte for byte, and the pack behind it is read by its own
// reader at the offset returned.
//
// Part 2: the planner's descriptors for random member lists, selections and
// pointers, written into exact-size arrays: units numbered without gaps from
// the first on, byte counts and pointers those of the list, bases only for
// diff members with elements, the init shares and x^(8 |last unit|) equal to
// the CRC arithmetic's own values -- checked by combining fsehip_crc32 of the
// units of a small host buffer the way the kernels do; and the scratch layout
// disjoint, 16-byte aligned and inside fsehip_mcheck_scratch_bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../entropy_coders_amd/csrc/fse_mcheck_host.h"
#include "../../include/fsehip.h"

using namespace fsehip;

static uint64_t rng_state = 0x13198A2E03707344ull;
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

static std::vector<fsehip_pack_member> valid_members(bool diff, uint32_t max_bits) {
    std::vector<fsehip_pack_member> v((size_t)(next_u64() % 40u));
    for (fsehip_pack_member& m : v) {
        m.d_ptr = nullptr;
        m.kind = kKinds[next_u64() % (diff ? 3u : 2u)];
        m.elem_bytes = 1u << (next_u64() % 4u);
        const uint32_t bits = (uint32_t)(next_u64() % max_bits);
        m.n_elems = bits ? next_u64() % (1ull << bits) : 0u;
    }
    return v;
}

static bool all_zero(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i)
        if (b[i]) return false;
    return true;
}

// the sealed pack's head: record, pack head, inner frame header
static std::vector<uint8_t> valid_head(const std::vector<fsehip_pack_member>& v, bool versioned, uint32_t flags) {
    const uint32_t n = (uint32_t)v.size();
    const uint64_t rec = fsehip_mcheck_bytes(n);
    std::vector<uint8_t> out((size_t)rec + 32u + 16u * n + 32u);
    fsehip_mcheck_info mi;
    std::memset(&mi, 0, sizeof(mi));
    mi.version = 1;
    mi.algorithm = FSEHIP_CHECK_CRC32;
    mi.flags = flags;
    mi.n_members = n;
    uint64_t content = 0;
    for (const fsehip_pack_member& m : v) content += m.n_elems * m.elem_bytes;
    mi.content_bytes = content;
    if (fsehip_mcheck_write_header(&mi, out.data()) != FSE_OK) std::abort();
    for (size_t i = 32; i < rec; ++i) out[i] = (uint8_t)next_u64();  // any table
    uint8_t* pk = out.data() + rec;
    if ((versioned ? fsehip_vpack_write_header : fsehip_pack_write_header)(v.data(), n, pk) != FSE_OK) std::abort();
    fsehip_frame_info f;
    std::memset(&f, 0, sizeof(f));
    f.version = 1;
    f.nstates = 2;
    f.max_table_log = 11;
    f.n_total = versioned ? fsehip_vpack_image_bytes(v.data(), n) : fsehip_pack_image_bytes(v.data(), n);
    f.block_size = 65536;
    f.n_blocks = (uint32_t)(f.n_total / f.block_size + (f.n_total % f.block_size != 0));
    if (fsehip_frame_write_header(&f, pk + 32u + 16u * n) != FSE_OK) std::abort();
    return out;
}

static int fuzz_heads(int cases) {
    int accepted = 0, accepted_rec = 0;
    for (int cs = 0; cs < cases; ++cs) {
        const bool versioned = next_u64() % 2u;
        const std::vector<fsehip_pack_member> v = valid_members(versioned, 41);
        const uint32_t flags = versioned ? (uint32_t)(next_u64() % 2u) : 0u;
        std::vector<uint8_t> good = valid_head(v, versioned, flags);
        std::vector<uint8_t> buf = good;
        const uint32_t mode = (uint32_t)(next_u64() % 6u);
        if (mode == 1) {  // random bytes behind the magic
            for (size_t i = 4; i < buf.size(); ++i) buf[i] = (uint8_t)next_u64();
        } else if (mode == 2) {  // truncated anywhere
            buf.resize((size_t)(next_u64() % (buf.size() + 1u)));
        } else if (mode == 3) {  // one byte of the heads damaged (the table is free)
            const size_t rec = (size_t)fsehip_mcheck_bytes((uint32_t)v.size());
            size_t at = (size_t)(next_u64() % (32u + buf.size() - rec));
            if (at >= 32u) at += rec - 32u;
            buf[at] ^= (uint8_t)(1u << (next_u64() % 8u));
        } else if (mode == 4) {  // a damaged header with its CRC repaired
            const size_t at = 4u + (size_t)(next_u64() % 24u);
            buf[at] ^= (uint8_t)(1u << (next_u64() % 8u));
            const uint32_t c = fsehip_crc32(0, buf.data(), 28);
            for (int i = 0; i < 4; ++i) buf[28 + i] = (uint8_t)(c >> (8 * i));
        } else if (mode == 5) {  // the other flavour's flag
            buf[6] ^= 1u;
            const uint32_t c = fsehip_crc32(0, buf.data(), 28);
            for (int i = 0; i < 4; ++i) buf[28 + i] = (uint8_t)(c >> (8 * i));
        }
        // exact-size heap copy: a read past the end is an ASan error
        uint8_t* heap = buf.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(buf.size()));
        if (!buf.empty()) std::memcpy(heap, buf.data(), buf.size());
        fsehip_mcheck_info mi, si;
        std::memset(&mi, 0xEE, sizeof(mi));
        std::memset(&si, 0xEE, sizeof(si));
        uint32_t ver = 99;
        uint64_t off = 99;
        const int rc_rec = fsehip_mcheck_read_header(heap, buf.size(), &mi);
        const int rc = fsehip_spack_read_header(heap, buf.size(), &si, &ver, &off);
        CHECK(rc_rec == FSE_OK || rc_rec == FSE_ERR_BAD_FRAME);
        CHECK(rc == FSE_OK || rc == FSE_ERR_BAD_FRAME);
        if (rc_rec != FSE_OK) {
            CHECK(all_zero(&mi, sizeof(mi)) && rc != FSE_OK);
        } else {
            ++accepted_rec;
            CHECK(mi.version == 1 && mi.algorithm == FSEHIP_CHECK_CRC32 && mi.flags <= 1u && mi.reserved == 0u);
            CHECK(mi.n_members <= FSEHIP_PACK_MAX_MEMBERS);
            uint8_t back[32];
            CHECK(fsehip_mcheck_write_header(&mi, back) == FSE_OK && std::memcmp(back, heap, 32) == 0);
        }
        if (rc != FSE_OK) {
            CHECK(all_zero(&si, sizeof(si)) && ver == 0u && off == 0u);
        } else {
            ++accepted;
            CHECK(std::memcmp(&si, &mi, sizeof(si)) == 0 && ver <= 1u);
            CHECK(off == fsehip_mcheck_bytes(si.n_members) && off + 32u <= buf.size());
            CHECK(!(si.flags & FSEHIP_MCHECK_BASES) || ver == 1u);
            fsehip_pack_info pk;
            CHECK((ver ? fsehip_vpack_read_header : fsehip_pack_read_header)(heap + off, buf.size() - (size_t)off, &pk) ==
                  FSE_OK);
            CHECK(pk.n_members == si.n_members && pk.content_bytes == si.content_bytes);
        }
        if (mode == 0) CHECK(rc == FSE_OK && ver == (versioned ? 1u : 0u));
        if (mode == 5) CHECK(rc == (versioned ? FSE_OK : FSE_ERR_BAD_FRAME));
        std::free(heap);
    }
    std::printf("ok heads %d accepted %d records %d\n", cases, accepted, accepted_rec);
    return accepted > cases / 8 ? 0 : 1;
}

// the CRC of `len` bytes at p as the kernels assemble it: units, the combine with x_last
static uint32_t combined(const McheckDesc& d, const uint8_t* p) {
    const uint64_t units = mcheck_units_of(d.bytes);
    uint32_t acc = 0;
    const uint32_t x_unit = crc::xpow8(kMcheckUnit);
    for (uint64_t u = 0; u < units; ++u) {
        const uint64_t off = u * kMcheckUnit, len = std::min<uint64_t>(kMcheckUnit, d.bytes - off);
        const uint32_t c = fsehip_crc32(0, p + off, (size_t)len);
        acc = crc::mulmod(acc, u + 1u == units ? d.x_last : x_unit) ^ c;
    }
    return acc;
}

static int fuzz_planner(int cases) {
    std::vector<uint8_t> data(5u * kMcheckUnit + 123u);
    for (uint8_t& b : data) b = (uint8_t)next_u64();
    for (int cs = 0; cs < cases; ++cs) {
        std::vector<fsehip_pack_member> v = valid_members(true, 19);
        const uint32_t n = (uint32_t)v.size();
        std::vector<const void*> bases(n);
        for (uint32_t m = 0; m < n; ++m) {
            fsehip_pack_member& mb = v[m];
            if (mb.n_elems * mb.elem_bytes > data.size() - 64u) mb.n_elems = (data.size() - 64u) / mb.elem_bytes;
            mb.d_ptr = data.data() + (next_u64() % (64u / mb.elem_bytes)) * mb.elem_bytes;
            bases[m] = data.data() + (next_u64() % (64u / mb.elem_bytes)) * mb.elem_bytes;
        }
        // a selection without repeats, or all
        std::vector<uint32_t> sel;
        const bool all = n == 0 || next_u64() % 2u;
        if (!all) {
            for (uint32_t m = 0; m < n; ++m)
                if (next_u64() % 2u) sel.push_back(m);
            for (size_t i = sel.size(); i > 1; --i) std::swap(sel[i - 1], sel[next_u64() % i]);
        }
        const uint32_t count = all ? n : (uint32_t)sel.size();
        const int which = (int)(next_u64() % 2u);
        const uint64_t first = next_u64() % 1000u;
        McheckDesc* out = count ? static_cast<McheckDesc*>(std::malloc(sizeof(McheckDesc) * count)) : nullptr;
        uint32_t n_long = 0;
        const uint64_t end = mcheck_plan(v.data(), which ? bases.data() : nullptr, all ? nullptr : sel.data(), count,
                                         which, first, out, &n_long);
        uint64_t unit = first;
        uint32_t longs = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t m = all ? i : sel[i];
            const fsehip_pack_member& mb = v[m];
            const McheckDesc& d = out[i];
            const bool reads = mb.n_elems && (which == kMcheckContent || mb.kind == FSEHIP_KIND_DIFF);
            CHECK(d.member == m && d.first_unit == unit);
            CHECK(d.bytes == (reads ? mb.n_elems * mb.elem_bytes : 0u));
            if (!reads) continue;
            const uint8_t* p = static_cast<const uint8_t*>(which ? bases[m] : mb.d_ptr);
            CHECK(d.ptr == (uint64_t)reinterpret_cast<uintptr_t>(p));
            const uint64_t units = mcheck_units_of(d.bytes), last = d.bytes - (units - 1u) * kMcheckUnit;
            const uint32_t alpha = (uint32_t)(d.ptr & 15u);
            CHECK(d.k_full == crc::init_share(alpha, kMcheckUnit) && d.k_last == crc::init_share(alpha, last));
            CHECK(d.x_last == crc::xpow8(last));
            CHECK(combined(d, p) == fsehip_crc32(0, p, (size_t)d.bytes));
            unit += units;
            longs += units > kMcheckSerialUnits;
        }
        CHECK(end == unit && n_long == longs);
        std::free(out);
        // the layout of two lists inside the public scratch size
        McheckList L[2];
        std::memset(L, 0, sizeof(L));
        for (uint32_t i = 0; i < count; ++i) {
            const fsehip_pack_member& mb = v[all ? i : sel[i]];
            L[0].units += mcheck_units_of(mb.n_elems * mb.elem_bytes);
            if (mb.kind == FSEHIP_KIND_DIFF) L[1].units += mcheck_units_of(mb.n_elems * mb.elem_bytes);
        }
        L[0].n = L[1].n = count;
        const uint64_t total = mcheck_layout(L, 2);
        CHECK(L[0].desc_off == kMcheckGateBytes && L[1].desc_off == L[0].desc_off + sizeof(McheckDesc) * count);
        CHECK(L[0].unit_off >= L[1].desc_off + sizeof(McheckDesc) * count && L[0].unit_off % 16u == 0);
        CHECK(L[0].span_off >= L[0].unit_off + 4u * L[0].units && L[0].span_off % 16u == 0);
        CHECK(L[1].unit_off >= L[0].span_off + 4u * count && L[1].unit_off % 16u == 0);
        CHECK(L[1].span_off >= L[1].unit_off + 4u * L[1].units && total >= L[1].span_off + 4u * count);
        const uint64_t pub = fsehip_mcheck_scratch_bytes(v.data(), n, all ? nullptr : sel.data(), count, 1);
        CHECK(pub >= total && pub % 16u == 0);
        // one list of both, as the build call lays it out
        McheckList one;
        std::memset(&one, 0, sizeof(one));
        one.n = 2u * count;
        one.units = L[0].units + L[1].units;
        CHECK(mcheck_layout(&one, 1) <= pub);
    }
    std::printf("ok planner %d\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 20000;
    if (fuzz_heads(cases)) return 1;
    return fuzz_planner(cases / 10);
}
