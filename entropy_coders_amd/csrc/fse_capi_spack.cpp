// fse_capi_spack.cpp -- the device calls of the member check record and of
// the sealed pack in the C ABI (fsehip.h section 2l): header, planner and
// scratch layout in fse_mcheck.cpp, kernels in fse_mcheck.hip, the pack calls
// themselves in fse_capi_pack.cpp.  The descriptors of every list a call
// checks reach the device through the workspace's pinned staging in one copy,
// in stream order; the lease is given back before the pack call, which takes
// the stream's workspace itself.  The header travels as a kernel argument.
// Every call is a constant number of launches whatever the member count, and
// none synchronises.
#include <string.h>

#include <vector>

#include "fse_capi_common.h"
#include "fse_mcheck_host.h"

using namespace fsehip::capi;
using fsehip::kFlavourPack;
using fsehip::kFlavourVpack;
using fsehip::kMcheckBase;
using fsehip::kMcheckContent;
using fsehip::McheckDesc;
using fsehip::McheckList;
using fsehip::PackFlavour;

namespace {

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

// the spans of the members idx[0 .. n) (nullptr: all) that `which` reads: there and aligned to their elements
bool spans_ok(const fsehip_pack_member* members, const void* const* ptrs, const uint32_t* idx, uint32_t n, int which) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t m = idx ? idx[i] : i;
        const fsehip_pack_member& mb = members[m];
        if (mb.n_elems == 0 || (which == kMcheckBase && !fsehip::pack_needs_base(mb))) continue;
        const void* p = ptrs ? ptrs[m] : mb.d_ptr;
        if (!p || !aligned(p, mb.elem_bytes)) return false;
    }
    return true;
}

// the selection is in range and names no member twice
bool selection_ok(const uint32_t* sel, uint32_t n_sel, uint32_t n) {
    std::vector<uint32_t> order(sel, sel + n_sel);
    std::sort(order.begin(), order.end());
    for (uint32_t s = 0; s < n_sel; ++s)
        if (order[s] >= n || (s && order[s] == order[s - 1u])) return false;
    return true;
}

// the descriptors to d_dst in one copy through pinned staging; the lease ends with the call
int upload(const std::vector<McheckDesc>& descs, uint8_t* d_dst, void* stream) {
    const uint64_t bytes = sizeof(McheckDesc) * descs.size();
    if (!bytes) return FSE_OK;
    Lease lease(stream);
    PinBuf* pin = lease.pin_get(bytes);
    if (!pin) return FSE_ERR_HIP;
    memcpy(pin->p, descs.data(), bytes);
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(d_dst, pin->p, bytes, hipMemcpyHostToDevice, hs) != hipSuccess) {
        (void)hipStreamSynchronize(hs);
        return FSE_ERR_HIP;
    }
    return lease.pin_sent(pin) ? FSE_OK : FSE_ERR_HIP;
}

// One list of spans on the device: its place in the scratch and what the planner found.
struct Pass {
    McheckList L{};
    uint32_t n_long = 0;
    const McheckDesc* descs(const uint8_t* d) const { return reinterpret_cast<const McheckDesc*>(d + L.desc_off); }
    uint32_t* unit_crc(uint8_t* d) const { return reinterpret_cast<uint32_t*>(d + L.unit_off); }
    uint32_t* span_crc(uint8_t* d) const { return reinterpret_cast<uint32_t*>(d + L.span_off); }
};

// the unit CRCs of a list, then its span CRCs: two launches
int run_pass(const Pass& P, uint8_t* d_mc, void* stream) {
    if (const int rc = fsehip::launch_mcheck_units(P.descs(d_mc), (uint32_t)P.L.n, P.L.units, P.unit_crc(d_mc), stream))
        return rc;
    return fsehip::launch_mcheck_combine(P.descs(d_mc), (uint32_t)P.L.n, P.n_long, P.unit_crc(d_mc), P.span_crc(d_mc),
                                         stream);
}

// The record of the members as they lie to d_record: one list, the contents
// and behind them (with_bases) the bases, so one units launch, one combine and
// the finish.  The caller has checked the list, the pointers and the scratch.
int build_record(const fsehip_pack_member* members, const void* const* bases, uint32_t n, bool with_bases,
                 uint64_t content_bytes, uint8_t* d_record, uint8_t* d_mc, uint64_t* d_out_len, const int32_t* d_result,
                 void* stream) {
    fsehip_mcheck_info info{};
    info.version = 1;
    info.algorithm = FSEHIP_CHECK_CRC32;
    info.flags = with_bases ? FSEHIP_MCHECK_BASES : 0u;
    info.n_members = n;
    info.content_bytes = content_bytes;
    uint8_t hdr[32];
    if (fsehip_mcheck_write_header(&info, hdr) != FSE_OK) return FSE_ERR_BAD_ARG;
    Pass P;
    std::vector<McheckDesc> descs((size_t)n * (with_bases ? 2u : 1u));
    uint64_t units = fsehip::mcheck_plan(members, nullptr, nullptr, n, kMcheckContent, 0, descs.data(), &P.n_long);
    if (with_bases) units = fsehip::mcheck_plan(members, bases, nullptr, n, kMcheckBase, units, descs.data() + n, &P.n_long);
    P.L.n = descs.size();
    P.L.units = units;
    fsehip::mcheck_layout(&P.L, 1);
    if (const int rc = upload(descs, d_mc + P.L.desc_off, stream)) return rc;
    if (const int rc = run_pass(P, d_mc, stream)) return rc;
    return fsehip::launch_mcheck_build_finish(hdr, P.span_crc(d_mc), n, with_bases, d_record, d_out_len,
                                              fsehip_mcheck_bytes(n), d_result, stream);
}

// what the sealed decode calls share: the record's info against the pack's, the header bytes
int sealed_args(const fsehip_mcheck_info* rec, const fsehip_pack_info* info, uint32_t versioned, const uint8_t* d_in,
                uint64_t in_len, const int32_t* d_check_result, uint8_t hdr[32]) {
    if (!rec || !info || !d_in || !d_check_result || fsehip_mcheck_write_header(rec, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    if (rec->n_members != info->n_members || rec->content_bytes != info->content_bytes) return FSE_ERR_BAD_ARG;
    if ((rec->flags & FSEHIP_MCHECK_BASES) && !versioned) return FSE_ERR_BAD_ARG;
    if (in_len < fsehip_mcheck_bytes(rec->n_members)) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

// The sealed decode around a pack decode `inner_call(gate)`: the bases of the
// members idx[0 .. n) verified first, the gate word filled; then the pack call,
// whose merge looks at the gate; then the destinations verified.
template <class Call>
int sealed_decode(const uint8_t hdr[32], const fsehip_mcheck_info* rec, const fsehip_pack_member* members,
                  const void* const* bases, const uint32_t* idx, uint32_t n, const uint8_t* d_record, uint8_t* d_mc,
                  int32_t* d_member_check, int32_t* d_base_check, int32_t* d_check_result, void* stream, Call inner_call) {
    const bool base_active = (rec->flags & FSEHIP_MCHECK_BASES) != 0u;
    Pass C, B;
    std::vector<McheckDesc> descs((size_t)n * (base_active ? 2u : 1u));
    C.L.n = n;
    C.L.units = fsehip::mcheck_plan(members, nullptr, idx, n, kMcheckContent, 0, descs.data(), &C.n_long);
    if (base_active) {
        B.L.n = n;
        B.L.units = fsehip::mcheck_plan(members, bases, idx, n, kMcheckBase, 0, descs.data() + n, &B.n_long);
    }
    McheckList L[2] = {C.L, B.L};
    fsehip::mcheck_layout(L, 2);
    C.L = L[0];
    B.L = L[1];
    int32_t* gate = reinterpret_cast<int32_t*>(d_mc);
    if (const int rc = upload(descs, d_mc + C.L.desc_off, stream)) return rc;
    if (base_active)
        if (const int rc = run_pass(B, d_mc, stream)) return rc;
    // not active: every base OK, the gate open unless the header differs
    if (const int rc = fsehip::launch_mcheck_verify_finish(hdr, d_record, base_active ? B.descs(d_mc) : C.descs(d_mc), n,
                                                           kMcheckBase, base_active, B.span_crc(d_mc), d_base_check,
                                                           d_check_result, fsehip::kMcheckBases, gate, stream))
        return rc;
    if (const int rc = inner_call(gate)) return rc;
    if (const int rc = run_pass(C, d_mc, stream)) return rc;
    return fsehip::launch_mcheck_verify_finish(hdr, d_record, C.descs(d_mc), n, kMcheckContent, true, C.span_crc(d_mc),
                                               d_member_check, d_check_result, fsehip::kMcheckContents, nullptr, stream);
}

}  // namespace

extern "C" {

int fsehip_mcheck_build(const fsehip_pack_member* members, const void* const* d_bases, uint32_t n_members,
                        uint8_t* d_record, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream) {
    if (!d_record || !d_scratch || !aligned(d_scratch, 16) || (n_members && !members)) return FSE_ERR_BAD_ARG;
    const bool with_bases = d_bases != nullptr;
    uint64_t content;
    if (const int rc = fsehip::pack_geom(members, n_members, nullptr, &content, kFlavourVpack)) return rc;
    if (!spans_ok(members, nullptr, nullptr, n_members, kMcheckContent)) return FSE_ERR_BAD_ARG;
    if (with_bases && !spans_ok(members, d_bases, nullptr, n_members, kMcheckBase)) return FSE_ERR_BAD_ARG;
    const uint64_t need = fsehip_mcheck_scratch_bytes(members, n_members, nullptr, 0, with_bases);
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return build_record(members, d_bases, n_members, with_bases, content, d_record, d_scratch, nullptr, nullptr, stream);
}

int fsehip_mcheck_verify(const fsehip_mcheck_info* info, const uint8_t* d_record, const fsehip_pack_member* members,
                         const uint32_t* sel, uint32_t n_sel, uint32_t which, const void* const* d_ptrs,
                         uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_status, int32_t* d_result,
                         fsehip_stream_t stream) {
    uint8_t hdr[32];
    if (!info || !d_record || !d_result || !d_scratch || !aligned(d_scratch, 16) || which > 1u ||
        fsehip_mcheck_write_header(info, hdr) != FSE_OK)
        return FSE_ERR_BAD_ARG;
    const uint32_t n = info->n_members;
    if (n && !members) return FSE_ERR_BAD_ARG;
    uint64_t content;
    if (const int rc = fsehip::pack_geom(members, n, nullptr, &content, kFlavourVpack)) return rc;
    if (content != info->content_bytes) return FSE_ERR_BAD_ARG;
    if (sel && !selection_ok(sel, n_sel, n)) return FSE_ERR_BAD_ARG;
    const uint32_t count = sel ? n_sel : n;
    if (count && !d_status) return FSE_ERR_BAD_ARG;
    const bool active = which == kMcheckContent || (info->flags & FSEHIP_MCHECK_BASES);
    if (which == kMcheckBase && active && !d_ptrs) {
        for (uint32_t i = 0; i < count; ++i)
            if (fsehip::pack_needs_base(members[sel ? sel[i] : i])) return FSE_ERR_BAD_ARG;
    }
    if (active && !spans_ok(members, d_ptrs, sel, count, (int)which)) return FSE_ERR_BAD_ARG;
    const uint64_t need = fsehip_mcheck_scratch_bytes(members, n, sel, n_sel, 0);
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    Pass P;
    std::vector<McheckDesc> descs(count);
    P.L.n = count;
    P.L.units = fsehip::mcheck_plan(members, d_ptrs, sel, count, active ? (int)which : kMcheckContent, 0, descs.data(),
                                    &P.n_long);
    fsehip::mcheck_layout(&P.L, 1);
    if (const int rc = upload(descs, d_scratch + P.L.desc_off, stream)) return rc;
    if (active)
        if (const int rc = run_pass(P, d_scratch, stream)) return rc;
    return fsehip::launch_mcheck_verify_finish(hdr, d_record, P.descs(d_scratch), count, (int)which, active,
                                               P.span_crc(d_scratch), d_status, d_result, fsehip::kMcheckAlone, nullptr,
                                               stream);
}

int fsehip_spack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                          const void* const* d_bases, uint32_t check_bases, uint8_t* d_scratch, uint64_t scratch_cap,
                          uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result,
                          fsehip_stream_t stream) {
    if (!p || !d_out || !d_out_len || !d_result || !d_scratch || !aligned(d_scratch, 16) || (n_members && !members))
        return FSE_ERR_BAD_ARG;
    const bool versioned = d_bases != nullptr, with_bases = versioned && check_bases;
    const PackFlavour f = versioned ? kFlavourVpack : kFlavourPack;
    uint64_t content;
    if (const int rc = fsehip::pack_geom(members, n_members, nullptr, &content, f)) return rc;
    const uint64_t rec = fsehip_mcheck_bytes(n_members);
    const uint64_t pack_need = round_up(fsehip::pack_scratch_bytes(f, members, n_members), 16);
    const uint64_t need = fsehip_spack_scratch_bytes(members, n_members, versioned);
    const uint32_t bs = p->block_size ? p->block_size : kDefaultBlock;
    const uint64_t bound = bs > kMaxBlock ? 0 : fsehip_spack_bound(members, n_members, versioned, bs);
    if (!need || !bound) return FSE_ERR_UNSUPPORTED;
    if (scratch_cap < need || out_cap < bound) return FSE_ERR_DST_TOO_SMALL;
    // the pack straight to its final place behind the record; its own checks come first
    if (const int rc = fsehip::pack_compress_impl(f, p, members, n_members, d_bases, d_scratch, pack_need, d_out + rec,
                                                  out_cap - rec, d_out_len, d_result, stream))
        return rc;
    return build_record(members, d_bases, n_members, with_bases, content, d_out, d_scratch + pack_need, d_out_len,
                        d_result, stream);
}

int fsehip_spack_decompress(const fsehip_mcheck_info* rec, const fsehip_pack_info* info, uint32_t versioned,
                            const fsehip_pack_member* members, const void* const* d_bases,
                            const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                            uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_block_status, int32_t* d_result,
                            int32_t* d_member_check, int32_t* d_base_check, int32_t* d_check_result,
                            fsehip_stream_t stream) {
    uint8_t hdr[32];
    if (const int rc = sealed_args(rec, info, versioned, d_in, in_len, d_check_result, hdr)) return rc;
    const PackFlavour f = versioned ? kFlavourVpack : kFlavourPack;
    const uint32_t n = rec->n_members;
    const uint64_t off = fsehip_mcheck_bytes(n);
    // the pack call's checks on the pack's share of the scratch, then the sealed call's own
    const uint64_t pack_need = round_up(fsehip::pack_scratch_bytes(f, members, n), 16);
    const uint64_t need = fsehip_spack_scratch_bytes(members, n, versioned);
    if (const int rc = fsehip::pack_decompress_check(f, info, members, d_bases, inner, d_in + off, in_len - off,
                                                     d_scratch, scratch_cap, d_result))
        return rc;
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return sealed_decode(hdr, rec, members, d_bases, nullptr, n, d_in, d_scratch + pack_need, d_member_check,
                         d_base_check, d_check_result, stream, [&](int32_t* gate) {
                             return fsehip::pack_decompress_launch(f, info, members, d_bases, inner, chunk_blocks,
                                                                   d_in + off, in_len - off, d_scratch, d_block_status,
                                                                   d_result, gate, stream);
                         });
}

int fsehip_spack_decompress_members(const fsehip_mcheck_info* rec, const fsehip_pack_info* info, uint32_t versioned,
                                    const fsehip_pack_member* members, const void* const* d_bases,
                                    const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
                                    uint64_t in_len, const uint32_t* sel, uint32_t n_sel, uint8_t* d_scratch,
                                    uint64_t scratch_cap, int32_t* d_member_status, int32_t* d_result,
                                    int32_t* d_member_check, int32_t* d_base_check, int32_t* d_check_result,
                                    fsehip_stream_t stream) {
    uint8_t hdr[32];
    if (const int rc = sealed_args(rec, info, versioned, d_in, in_len, d_check_result, hdr)) return rc;
    const PackFlavour f = versioned ? kFlavourVpack : kFlavourPack;
    const uint32_t n = rec->n_members;
    const uint64_t off = fsehip_mcheck_bytes(n);
    const uint64_t pack_need = round_up(fsehip::pack_members_scratch_bytes(f, members, n, sel, n_sel), 16);
    const uint64_t need = fsehip_spack_members_scratch_bytes(members, n, versioned, sel, n_sel);
    fsehip::PackMembersPlan plan;
    if (const int rc = fsehip::pack_members_check(f, info, members, d_bases, inner, d_in + off, in_len - off, sel, n_sel,
                                                  d_scratch, scratch_cap, d_result, &plan))
        return rc;
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return sealed_decode(hdr, rec, members, d_bases, sel, n_sel, d_in, d_scratch + pack_need, d_member_check,
                         d_base_check, d_check_result, stream, [&](int32_t* gate) {
                             return fsehip::pack_members_launch(f, info, members, d_bases, inner, chunk_blocks,
                                                                d_in + off, in_len - off, sel, n_sel, plan, d_scratch,
                                                                d_member_status, d_result, gate, stream);
                         });
}

}  // extern "C"
