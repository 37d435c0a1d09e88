// fse_mcheck.cpp -- the member check record's header, sizes, planner and
// scratch layout, and the sealed pack's head reader, host side (fsehip.h
// section 2l).
//
// Plain C++ with no HIP include, as fse_check.cpp and fse_pack.cpp, over both:
// the same source builds into libfsehip.so and, with g++ alone, into the
// sanitizer fuzz of tests/native/spack_fuzz.cpp.  The kernels are
// fse_mcheck.hip, the device calls fse_capi_spack.cpp.
#include <string.h>

#include "../../include/fsehip.h"
#include "fse_mcheck_host.h"

namespace {

using namespace fsehip;

uint32_t get32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
void put32(uint8_t* p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

bool fields_ok(const fsehip_mcheck_info& f) {
    return f.version == 1u && f.algorithm == FSEHIP_CHECK_CRC32 && (f.flags & ~FSEHIP_MCHECK_BASES) == 0u &&
           f.n_members <= FSEHIP_PACK_MAX_MEMBERS && f.reserved == 0u;
}

void header_bytes(const fsehip_mcheck_info& f, uint8_t hdr[32]) {
    memset(hdr, 0, kMcheckHeaderBytes);
    memcpy(hdr, "FSES", 4);
    hdr[4] = (uint8_t)f.version;
    hdr[5] = (uint8_t)f.algorithm;
    hdr[6] = (uint8_t)f.flags;
    put32(hdr + 8, f.n_members);
    for (int i = 0; i < 8; ++i) hdr[16 + i] = (uint8_t)(f.content_bytes >> (8 * i));
    put32(hdr + 28, fsehip_crc32(0, hdr, 28));
}

uint64_t round16(uint64_t x) { return (x + 15u) & ~15ull; }

PackFlavour flavour(uint32_t versioned) { return versioned ? kFlavourVpack : kFlavourPack; }

// the scratch of the kernels for the members idx[0 .. n) of a valid list: one
// list of contents and, with_bases, one of bases
uint64_t scratch_of(const fsehip_pack_member* members, const uint32_t* idx, uint32_t n, bool with_bases) {
    McheckList L[2] = {};
    for (uint32_t i = 0; i < n; ++i) {
        const fsehip_pack_member& mb = members[idx ? idx[i] : i];
        const uint64_t units = mcheck_units_of(mb.n_elems * mb.elem_bytes);
        L[0].units += units;
        if (with_bases && pack_needs_base(mb)) L[1].units += units;
    }
    L[0].n = n;
    L[1].n = with_bases ? n : 0u;
    // the build call lays both lists out as one, which is never larger: round16(a + b) <= round16(a) + round16(b)
    return mcheck_layout(L, 2);
}

}  // namespace

extern "C" {

uint64_t fsehip_mcheck_bytes(uint32_t n_members) {
    if (n_members > FSEHIP_PACK_MAX_MEMBERS) return 0;
    return kMcheckHeaderBytes + (uint64_t)kMcheckEntryBytes * n_members;
}

int fsehip_mcheck_read_header(const uint8_t* hdr, size_t len, fsehip_mcheck_info* out) {
    if (!out || (!hdr && len)) return FSE_ERR_BAD_ARG;
    memset(out, 0, sizeof(*out));
    if (len < kMcheckHeaderBytes) return FSE_ERR_BAD_FRAME;
    if (memcmp(hdr, "FSES", 4) != 0) return FSE_ERR_BAD_FRAME;
    fsehip_mcheck_info f;
    memset(&f, 0, sizeof(f));
    f.version = hdr[4];
    f.algorithm = hdr[5];
    f.flags = hdr[6];
    f.n_members = get32(hdr + 8);
    f.reserved = (uint32_t)hdr[7] | get32(hdr + 12) | get32(hdr + 24);  // the spare byte and both reserved words: zero
    for (int i = 7; i >= 0; --i) f.content_bytes = (f.content_bytes << 8) | hdr[16 + i];
    f.header_crc = get32(hdr + 28);
    if (!fields_ok(f) || f.header_crc != fsehip_crc32(0, hdr, 28)) return FSE_ERR_BAD_FRAME;
    *out = f;
    return FSE_OK;
}

int fsehip_mcheck_write_header(const fsehip_mcheck_info* info, uint8_t hdr[32]) {
    if (!info || !hdr || !fields_ok(*info)) return FSE_ERR_BAD_ARG;
    header_bytes(*info, hdr);
    return FSE_OK;
}

int fsehip_spack_read_header(const uint8_t* buf, size_t len, fsehip_mcheck_info* info, uint32_t* versioned,
                             uint64_t* inner_off) {
    if (!info || !versioned || !inner_off || (!buf && len)) return FSE_ERR_BAD_ARG;
    *versioned = 0;
    *inner_off = 0;
    fsehip_mcheck_info f;
    const int rc = fsehip_mcheck_read_header(buf, len, &f);
    memset(info, 0, sizeof(*info));
    if (rc != FSE_OK) return rc;
    const uint64_t off = fsehip_mcheck_bytes(f.n_members);
    if (len < off || len - off < 4u) return FSE_ERR_BAD_FRAME;
    const uint8_t* in = buf + off;
    const bool v = memcmp(in, "FSEV", 4) == 0;
    if (!v && memcmp(in, "FSEM", 4) != 0) return FSE_ERR_BAD_FRAME;
    if ((f.flags & FSEHIP_MCHECK_BASES) && !v) return FSE_ERR_BAD_FRAME;
    fsehip_pack_info pk;
    if (pack_read_header(flavour(v), in, len - (size_t)off, &pk) != FSE_OK) return FSE_ERR_BAD_FRAME;
    if (pk.n_members != f.n_members || pk.content_bytes != f.content_bytes) return FSE_ERR_BAD_FRAME;
    *info = f;
    *versioned = v ? 1u : 0u;
    *inner_off = off;
    return FSE_OK;
}

uint64_t fsehip_mcheck_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, const uint32_t* sel,
                                     uint32_t n_sel, uint32_t with_bases) {
    if (pack_geom(members, n_members, nullptr, nullptr, kFlavourVpack) != FSE_OK) return 0;
    if (!sel) return scratch_of(members, nullptr, n_members, with_bases != 0u);
    for (uint32_t s = 0; s < n_sel; ++s)
        if (sel[s] >= n_members) return 0;
    return scratch_of(members, sel, n_sel, with_bases != 0u);
}

uint64_t fsehip_spack_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned,
                            uint32_t block_size) {
    const uint64_t inner = pack_bound(flavour(versioned), members, n_members, block_size);
    const uint64_t rec = fsehip_mcheck_bytes(n_members);
    return !inner || !rec || inner > UINT64_MAX - rec ? 0 : rec + inner;
}

uint64_t fsehip_spack_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned) {
    const uint64_t pack = pack_scratch_bytes(flavour(versioned), members, n_members);
    if (!pack || pack > UINT64_MAX - 15u) return 0;
    const uint64_t mc = scratch_of(members, nullptr, n_members, versioned != 0u);
    return round16(pack) > UINT64_MAX - mc ? 0 : round16(pack) + mc;
}

uint64_t fsehip_spack_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned,
                                            const uint32_t* sel, uint32_t n_sel) {
    const uint64_t pack = pack_members_scratch_bytes(flavour(versioned), members, n_members, sel, n_sel);
    if (!pack || pack > UINT64_MAX - 15u) return 0;
    const uint64_t mc = scratch_of(members, sel, n_sel, versioned != 0u);
    return round16(pack) > UINT64_MAX - mc ? 0 : round16(pack) + mc;
}

}  // extern "C"

namespace fsehip {

uint64_t mcheck_plan(const fsehip_pack_member* members, const void* const* ptrs, const uint32_t* idx, uint32_t n,
                     int which, uint64_t first_unit, McheckDesc* out, uint32_t* n_long) {
    uint32_t k_full[16];  // by the pointer's alignment mod 16
    bool have[16] = {};
    uint64_t unit = first_unit;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = idx ? idx[i] : i;
        const fsehip_pack_member& mb = members[m];
        McheckDesc& d = out[i];
        memset(&d, 0, sizeof(d));
        d.member = m;
        d.first_unit = unit;
        d.x_last = 0x80000000u;  // x^0
        if (mb.n_elems == 0 || (which == kMcheckBase && !pack_needs_base(mb))) continue;
        const void* p = ptrs ? ptrs[m] : mb.d_ptr;
        d.ptr = (uint64_t)reinterpret_cast<uintptr_t>(p);
        d.bytes = mb.n_elems * mb.elem_bytes;
        const uint64_t units = mcheck_units_of(d.bytes), last = d.bytes - (units - 1u) * kMcheckUnit;
        const uint32_t alpha = (uint32_t)(d.ptr & 15u);
        if (!have[alpha]) {
            k_full[alpha] = crc::init_share(alpha, kMcheckUnit);
            have[alpha] = true;
        }
        d.k_full = k_full[alpha];
        d.k_last = last == kMcheckUnit ? k_full[alpha] : crc::init_share(alpha, last);
        d.x_last = crc::xpow8(last);
        if (n_long && units > kMcheckSerialUnits) ++*n_long;
        unit += units;
    }
    return unit;
}

uint64_t mcheck_layout(McheckList* lists, uint32_t n_lists) {
    uint64_t at = kMcheckGateBytes;
    for (uint32_t i = 0; i < n_lists; ++i) {
        lists[i].desc_off = at;
        at += sizeof(McheckDesc) * lists[i].n;
    }
    at = round16(at);
    for (uint32_t i = 0; i < n_lists; ++i) {
        lists[i].unit_off = at;
        at += round16(4u * lists[i].units);
        lists[i].span_off = at;
        at += round16(4u * lists[i].n);
    }
    return at;
}

}  // namespace fsehip
