// fse_capi_pack.cpp -- the device calls of the pack frame and of the
// versioned pack in the C ABI (fsehip.h sections 2j and 2k): header, table,
// planner and pointer checks in fse_pack.cpp, kernels in fse_pack.hip and
// fse_vpack.hip.  Every call is one transform over all members around one
// frame call of section 2b on the caller's scratch.  The member descriptors,
// the versioned pack's base pointers and the head bytes reach the device
// through the workspace's pinned staging in one copy, in stream order; the
// lease is given back before the frame call, which takes the stream's
// workspace itself.  The fsehip_pack_* and fsehip_vpack_* calls are fronts of
// one implementation per call, told apart by the flavour.
#include <string.h>

#include <vector>

#include "fse_capi_common.h"
#include "fse_mcheck_host.h"
#include "fse_pack_host.h"

using namespace fsehip::capi;
using fsehip::kFlavourPack;
using fsehip::kFlavourVpack;
using fsehip::PackDesc;
using fsehip::PackFlavour;

namespace {

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

// a member with elements: its pointer there and aligned to its elements
bool member_ptr_ok(const fsehip_pack_member& mb) {
    return mb.n_elems == 0 || (mb.d_ptr && aligned(mb.d_ptr, mb.elem_bytes));
}

// the members idx[0 .. n) (nullptr: all): every pointer there and aligned, a diff member's base too
bool pointers_ok(const fsehip_pack_member* members, const void* const* bases, const uint32_t* idx, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (!member_ptr_ok(members[idx ? idx[i] : i])) return false;
    return fsehip::pack_bases_ok(members, bases, idx, n);
}

// The descriptors, behind them the base pointers of the descriptors' members
// (the versioned pack; idx[s] is descriptor s's member, nullptr: s itself) and
// the head bytes of `members`, to d_dst in one copy through pinned staging; the
// lease ends with the call
int upload(PackFlavour f, const std::vector<PackDesc>& descs, const fsehip_pack_member* members, uint32_t n_members,
           const void* const* bases, const uint32_t* idx, uint8_t* d_dst, void* stream) {
    const uint64_t desc_bytes = sizeof(PackDesc) * descs.size(), head = fsehip::pack_head_bytes(n_members);
    const uint64_t base_bytes = f == kFlavourVpack ? 8u * descs.size() : 0u;
    Lease lease(stream);
    PinBuf* pin = lease.pin_get(desc_bytes + base_bytes + head);
    if (!pin) return FSE_ERR_HIP;
    uint8_t* h = static_cast<uint8_t*>(pin->p);
    if (desc_bytes) memcpy(h, descs.data(), desc_bytes);
    if (base_bytes) {
        uint64_t* b = reinterpret_cast<uint64_t*>(h + desc_bytes);
        for (size_t s = 0; s < descs.size(); ++s) {
            const uint32_t m = idx ? idx[s] : (uint32_t)s;
            b[s] = fsehip::pack_needs_base(members[m]) ? (uint64_t)reinterpret_cast<uintptr_t>(bases[m]) : 0u;
        }
    }
    if (fsehip::pack_write_header(f, members, n_members, h + desc_bytes + base_bytes) != FSE_OK) return FSE_ERR_BAD_ARG;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(d_dst, h, desc_bytes + base_bytes + head, hipMemcpyHostToDevice, hs) != hipSuccess) {
        (void)hipStreamSynchronize(hs);
        return FSE_ERR_HIP;
    }
    return lease.pin_sent(pin) ? FSE_OK : FSE_ERR_HIP;
}

// where the pieces of an upload of n descriptors lie from d_descs on
const PackDesc* descs_at(const uint8_t* d_descs) { return reinterpret_cast<const PackDesc*>(d_descs); }
const uint64_t* bases_at(const uint8_t* d_descs, uint64_t n) {
    return reinterpret_cast<const uint64_t*>(d_descs + sizeof(PackDesc) * n);
}
const uint8_t* head_at(PackFlavour f, const uint8_t* d_descs, uint64_t n) {
    return d_descs + fsehip::pack_desc_bytes(f) * n;
}

int launch_split(PackFlavour f, const uint8_t* d_descs, uint32_t n, uint64_t tiles, uint8_t* image, void* stream) {
    if (f == kFlavourVpack) return fsehip::launch_vpack_split(descs_at(d_descs), bases_at(d_descs, n), n, tiles, image, stream);
    return fsehip::launch_pack_split(descs_at(d_descs), n, tiles, image, stream);
}

int launch_merge(PackFlavour f, const uint8_t* d_descs, uint32_t n, uint64_t tiles, const uint8_t* planes,
                 const int32_t* result, void* stream) {
    if (f == kFlavourVpack)
        return fsehip::launch_vpack_merge(descs_at(d_descs), bases_at(d_descs, n), n, tiles, planes, result, stream);
    return fsehip::launch_pack_merge(descs_at(d_descs), n, tiles, planes, result, stream);
}

// The sealed pack's decode (fse_capi_spack.cpp) brings a gate word that its
// base verification has filled: the frame status joins it on the device, and
// the merge is handed the gate in place of d_result, storing nothing when
// either says BAD_FRAME.  A gate launch that fails ends the call: the merge is
// never launched without the word it was to look at.  gate nullptr (the pack
// calls themselves): the merge looks at d_result.
int gated_merge(PackFlavour f, const uint8_t* d_descs, uint32_t n, uint64_t tiles, const uint8_t* planes,
                const int32_t* d_result, int32_t* gate, void* stream) {
    if (!gate) return launch_merge(f, d_descs, n, tiles, planes, d_result, stream);
    if (const int rc = fsehip::launch_mcheck_gate(d_result, gate, stream)) return rc;
    return launch_merge(f, d_descs, n, tiles, planes, gate, stream);
}

// the checks of a bare transform; *image = the image's bytes
int transform_args(PackFlavour f, const fsehip_pack_member* members, uint32_t n, const void* const* bases,
                   const uint8_t* d_image, const uint8_t* d_scratch, uint64_t scratch_cap, uint64_t* image) {
    if (n && !members) return FSE_ERR_BAD_ARG;
    if (const int rc = fsehip::pack_geom(members, n, image, nullptr, f)) return rc;
    if (*image == 0) return FSE_OK;  // nothing to move: no pointer is looked at
    if (!pointers_ok(members, bases, nullptr, n)) return FSE_ERR_BAD_ARG;
    if (*image && (!d_image || !aligned(d_image, 16))) return FSE_ERR_BAD_ARG;
    if (n && (!d_scratch || !aligned(d_scratch, 16))) return FSE_ERR_BAD_ARG;
    if (scratch_cap < fsehip::pack_scratch_bytes(f, members, n) - *image) return FSE_ERR_DST_TOO_SMALL;
    return FSE_OK;
}

// the decode calls' common checks: the info, the members and the inner info agree
int decode_args(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len, const int32_t* d_result) {
    if (!info || !inner || !d_in || !d_result || (info->n_members && !members)) return FSE_ERR_BAD_ARG;
    if (info->n_members > FSEHIP_PACK_MAX_MEMBERS) return FSE_ERR_UNSUPPORTED;
    uint64_t image, content;
    if (const int rc = fsehip::pack_geom(members, info->n_members, &image, &content, f)) return rc;
    uint8_t hb[32];
    if (info->version != 1u || image != info->image_bytes || content != info->content_bytes ||
        fsehip_frame_write_header(inner, hb) != FSE_OK || inner->n_total != image)
        return FSE_ERR_BAD_ARG;
    if (in_len < fsehip::pack_head_bytes(info->n_members) + 32u) return FSE_ERR_BAD_ARG;
    return FSE_OK;
}

int split(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, const void* const* bases,
          uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, void* stream) {
    uint64_t image;
    if (const int rc = transform_args(f, members, n_members, bases, d_image, d_scratch, scratch_cap, &image)) return rc;
    if (image == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    std::vector<PackDesc> descs(n_members);
    const uint64_t tiles = fsehip::pack_plan(members, n_members, descs.data());
    if (const int rc = upload(f, descs, members, n_members, bases, nullptr, d_scratch, stream)) return rc;
    return launch_split(f, d_scratch, n_members, tiles, d_image, stream);
}

int merge(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, const void* const* bases,
          const uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, void* stream) {
    uint64_t image;
    if (const int rc = transform_args(f, members, n_members, bases, d_image, d_scratch, scratch_cap, &image)) return rc;
    if (!fsehip::pack_decode_spans_ok(members, bases, nullptr, n_members)) return FSE_ERR_BAD_ARG;
    if (image == 0) return FSE_OK;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    std::vector<PackDesc> descs(n_members);
    const uint64_t tiles = fsehip::pack_plan(members, n_members, descs.data());
    if (const int rc = upload(f, descs, members, n_members, bases, nullptr, d_scratch, stream)) return rc;
    return launch_merge(f, d_scratch, n_members, tiles, d_image, nullptr, stream);
}

int compress(PackFlavour f, const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
             const void* const* bases, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
             uint64_t* d_out_len, int32_t* d_result, void* stream) {
    if (!p || !d_out || !d_out_len || !d_result || !d_scratch || (n_members && !members)) return FSE_ERR_BAD_ARG;
    uint64_t image;
    if (const int rc = fsehip::pack_geom(members, n_members, &image, nullptr, f)) return rc;
    // the frame call's own rules, ahead of the split launch
    const auto [bs, n_blocks, geom_rc] = block_geom(p->block_size, image, false);
    (void)n_blocks;
    if (geom_rc != FSE_OK) return geom_rc;
    if (p->nstates > 2 || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (!pointers_ok(members, bases, nullptr, n_members)) return FSE_ERR_BAD_ARG;
    if (p->ckpt_interval && !ckpt_interval_ok(p->nstates == 1 ? 1u : 2u, p->ckpt_interval)) return FSE_ERR_BAD_ARG;
    const uint64_t bound = fsehip::pack_bound(f, members, n_members, bs);
    const uint64_t need = fsehip::pack_scratch_bytes(f, members, n_members);
    if (!bound || !need) return FSE_ERR_UNSUPPORTED;
    if (scratch_cap < need || out_cap < bound) return FSE_ERR_DST_TOO_SMALL;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    std::vector<PackDesc> descs(n_members);
    const uint64_t tiles = fsehip::pack_plan(members, n_members, descs.data());
    const uint64_t head = fsehip::pack_head_bytes(n_members);
    uint8_t* d_descs = d_scratch + image;
    if (const int rc = upload(f, descs, members, n_members, bases, nullptr, d_descs, stream)) return rc;
    if (const int rc = launch_split(f, d_descs, n_members, tiles, d_scratch, stream)) return rc;
    if (const int rc = fsehip_frame_compress(p, d_scratch, image, d_out + head, out_cap - head, d_out_len, d_result,
                                             stream))
        return rc;
    return fsehip::launch_pack_finish(head_at(f, d_descs, n_members), head, d_out, d_out_len, stream);
}

// The whole decode in two halves, so that the sealed pack can run the first,
// verify its bases, and then run the second: every check before any device
// use but the question for a device itself, then the launches.
int decompress_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                     const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len,
                     const uint8_t* d_scratch, uint64_t scratch_cap, const int32_t* d_result) {
    if (const int rc = decode_args(f, info, members, inner, d_in, in_len, d_result)) return rc;
    const uint32_t n = info->n_members;
    if (!d_scratch || !aligned(d_scratch, 16)) return FSE_ERR_BAD_ARG;
    if (!pointers_ok(members, bases, nullptr, n)) return FSE_ERR_BAD_ARG;
    if (!fsehip::pack_decode_spans_ok(members, bases, nullptr, n)) return FSE_ERR_BAD_ARG;
    const uint64_t need = fsehip::pack_scratch_bytes(f, members, n);
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    return FSE_OK;
}

int decompress_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                      const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                      const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, int32_t* d_block_status,
                      int32_t* d_result, int32_t* gate, void* stream) {
    const uint32_t n = info->n_members;
    std::vector<PackDesc> descs(n);
    const uint64_t tiles = fsehip::pack_plan(members, n, descs.data());
    const uint64_t head = fsehip::pack_head_bytes(n), image = info->image_bytes;
    uint8_t* d_descs = d_scratch + image;
    if (const int rc = upload(f, descs, members, n, bases, nullptr, d_descs, stream)) return rc;
    if (const int rc = fsehip_frame_decompress(inner, chunk_blocks, d_in + head, in_len - head, d_scratch, image,
                                               d_block_status, d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_pack_check(head_at(f, d_descs, n), head, d_in, d_result, d_block_status,
                                                 inner->n_blocks, false, stream))
        return rc;
    return gated_merge(f, d_descs, n, tiles, d_scratch, d_result, gate, stream);
}

int decompress(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
               const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
               uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_block_status, int32_t* d_result,
               void* stream) {
    if (const int rc = decompress_check(f, info, members, bases, inner, d_in, in_len, d_scratch, scratch_cap, d_result))
        return rc;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return decompress_launch(f, info, members, bases, inner, chunk_blocks, d_in, in_len, d_scratch, d_block_status,
                             d_result, nullptr, stream);
}

// The selected-member decode, in the same two halves; the check half leaves
// its plan for the launch half.  Scratch: the selected members' planes,
// stride_m bytes each, from offset 0 on (every one 16-byte aligned); the plane
// ranges' statuses of the frame call; the selected members' descriptors (and
// base pointers); the head bytes.
int members_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                  const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len,
                  const uint32_t* sel, uint32_t n_sel, const uint8_t* d_scratch, uint64_t scratch_cap,
                  const int32_t* d_result, fsehip::PackMembersPlan* plan) {
    if (const int rc = decode_args(f, info, members, inner, d_in, in_len, d_result)) return rc;
    const uint32_t n = info->n_members;
    if (!d_scratch || !aligned(d_scratch, 16) || (n_sel && !sel)) return FSE_ERR_BAD_ARG;
    if (const int rc = fsehip::pack_plan_selected(members, n, sel, n_sel, &plan->descs, &plan->ranges,
                                                  &plan->planes_bytes, &plan->tiles))
        return rc;
    if (!pointers_ok(members, bases, sel, n_sel)) return FSE_ERR_BAD_ARG;
    if (!fsehip::pack_decode_spans_ok(members, bases, sel, n_sel)) return FSE_ERR_BAD_ARG;
    const uint64_t need = fsehip::pack_members_scratch_bytes(f, members, n, sel, n_sel);
    if (!need || scratch_cap < need) return FSE_ERR_DST_TOO_SMALL;
    return FSE_OK;
}

int members_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                   const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
                   uint64_t in_len, const uint32_t* sel, uint32_t n_sel, const fsehip::PackMembersPlan& plan,
                   uint8_t* d_scratch, int32_t* d_member_status, int32_t* d_result, int32_t* gate, void* stream) {
    const uint32_t n = info->n_members;
    const uint64_t head = fsehip::pack_head_bytes(n), planes_bytes = plan.planes_bytes;
    const uint32_t n_ranges = (uint32_t)plan.ranges.size();
    int32_t* plane_status = reinterpret_cast<int32_t*>(d_scratch + planes_bytes);
    uint8_t* d_descs = d_scratch + planes_bytes + round_up(4ull * n_ranges, 16);
    if (const int rc = upload(f, plan.descs, members, n, bases, sel, d_descs, stream)) return rc;
    if (const int rc = fsehip_frame_decompress_ranges(inner, chunk_blocks, d_in + head, in_len - head,
                                                      plan.ranges.data(), n_ranges, d_scratch, planes_bytes,
                                                      n_ranges ? plane_status : nullptr, d_result, stream))
        return rc;
    if (const int rc = fsehip::launch_pack_check(head_at(f, d_descs, n_sel), head, d_in, d_result, nullptr, 0, true,
                                                 stream))
        return rc;
    if (const int rc = fsehip::launch_pack_member_status(descs_at(d_descs), n_sel, plane_status, d_member_status,
                                                         d_result, stream))
        return rc;
    return gated_merge(f, d_descs, n_sel, plan.tiles, d_scratch, d_result, gate, stream);
}

int decompress_members(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                       const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                       const uint8_t* d_in, uint64_t in_len, const uint32_t* sel, uint32_t n_sel, uint8_t* d_scratch,
                       uint64_t scratch_cap, int32_t* d_member_status, int32_t* d_result, void* stream) {
    fsehip::PackMembersPlan plan;
    if (const int rc = members_check(f, info, members, bases, inner, d_in, in_len, sel, n_sel, d_scratch, scratch_cap,
                                     d_result, &plan))
        return rc;
    if (!device_ok()) return FSE_ERR_NO_DEVICE;
    return members_launch(f, info, members, bases, inner, chunk_blocks, d_in, in_len, sel, n_sel, plan, d_scratch,
                          d_member_status, d_result, nullptr, stream);
}

}  // namespace

// the sealed pack's way in (fse_mcheck_host.h)
namespace fsehip {

int pack_compress_impl(PackFlavour f, const fsehip_frame_params* p, const fsehip_pack_member* members,
                       uint32_t n_members, const void* const* bases, uint8_t* d_scratch, uint64_t scratch_cap,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result, void* stream) {
    return compress(f, p, members, n_members, bases, d_scratch, scratch_cap, d_out, out_cap, d_out_len, d_result,
                    stream);
}

int pack_decompress_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                          const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in,
                          uint64_t in_len, const uint8_t* d_scratch, uint64_t scratch_cap, const int32_t* d_result) {
    return decompress_check(f, info, members, bases, inner, d_in, in_len, d_scratch, scratch_cap, d_result);
}

int pack_decompress_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                           const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                           const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, int32_t* d_block_status,
                           int32_t* d_result, int32_t* gate, void* stream) {
    return decompress_launch(f, info, members, bases, inner, chunk_blocks, d_in, in_len, d_scratch, d_block_status,
                             d_result, gate, stream);
}

int pack_members_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                       const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len,
                       const uint32_t* sel, uint32_t n_sel, const uint8_t* d_scratch, uint64_t scratch_cap,
                       const int32_t* d_result, PackMembersPlan* plan) {
    return members_check(f, info, members, bases, inner, d_in, in_len, sel, n_sel, d_scratch, scratch_cap, d_result,
                         plan);
}

int pack_members_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                        const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                        const uint8_t* d_in, uint64_t in_len, const uint32_t* sel, uint32_t n_sel,
                        const PackMembersPlan& plan, uint8_t* d_scratch, int32_t* d_member_status, int32_t* d_result,
                        int32_t* gate, void* stream) {
    return members_launch(f, info, members, bases, inner, chunk_blocks, d_in, in_len, sel, n_sel, plan, d_scratch,
                          d_member_status, d_result, gate, stream);
}

}  // namespace fsehip

extern "C" {

int fsehip_pack_split(const fsehip_pack_member* members, uint32_t n_members, uint8_t* d_image, uint8_t* d_scratch,
                      uint64_t scratch_cap, fsehip_stream_t stream) {
    return split(kFlavourPack, members, n_members, nullptr, d_image, d_scratch, scratch_cap, stream);
}

int fsehip_pack_merge(const fsehip_pack_member* members, uint32_t n_members, const uint8_t* d_image,
                      uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream) {
    return merge(kFlavourPack, members, n_members, nullptr, d_image, d_scratch, scratch_cap, stream);
}

int fsehip_pack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                         uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                         uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    return compress(kFlavourPack, p, members, n_members, nullptr, d_scratch, scratch_cap, d_out, out_cap, d_out_len,
                    d_result, stream);
}

int fsehip_pack_decompress(const fsehip_pack_info* info, const fsehip_pack_member* members,
                           const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                           uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_block_status, int32_t* d_result,
                           fsehip_stream_t stream) {
    return decompress(kFlavourPack, info, members, nullptr, inner, chunk_blocks, d_in, in_len, d_scratch, scratch_cap,
                      d_block_status, d_result, stream);
}

int fsehip_pack_decompress_members(const fsehip_pack_info* info, const fsehip_pack_member* members,
                                   const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
                                   uint64_t in_len, const uint32_t* sel, uint32_t n_sel, uint8_t* d_scratch,
                                   uint64_t scratch_cap, int32_t* d_member_status, int32_t* d_result,
                                   fsehip_stream_t stream) {
    return decompress_members(kFlavourPack, info, members, nullptr, inner, chunk_blocks, d_in, in_len, sel, n_sel,
                              d_scratch, scratch_cap, d_member_status, d_result, stream);
}

int fsehip_vpack_split(const fsehip_pack_member* members, uint32_t n_members, const void* const* d_bases,
                       uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream) {
    return split(kFlavourVpack, members, n_members, d_bases, d_image, d_scratch, scratch_cap, stream);
}

int fsehip_vpack_merge(const fsehip_pack_member* members, uint32_t n_members, const void* const* d_bases,
                       const uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream) {
    return merge(kFlavourVpack, members, n_members, d_bases, d_image, d_scratch, scratch_cap, stream);
}

int fsehip_vpack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                          const void* const* d_bases, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream) {
    return compress(kFlavourVpack, p, members, n_members, d_bases, d_scratch, scratch_cap, d_out, out_cap, d_out_len,
                    d_result, stream);
}

int fsehip_vpack_decompress(const fsehip_pack_info* info, const fsehip_pack_member* members,
                            const void* const* d_bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                            const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                            int32_t* d_block_status, int32_t* d_result, fsehip_stream_t stream) {
    return decompress(kFlavourVpack, info, members, d_bases, inner, chunk_blocks, d_in, in_len, d_scratch,
                      scratch_cap, d_block_status, d_result, stream);
}

int fsehip_vpack_decompress_members(const fsehip_pack_info* info, const fsehip_pack_member* members,
                                    const void* const* d_bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                                    const uint8_t* d_in, uint64_t in_len, const uint32_t* sel, uint32_t n_sel,
                                    uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_member_status,
                                    int32_t* d_result, fsehip_stream_t stream) {
    return decompress_members(kFlavourVpack, info, members, d_bases, inner, chunk_blocks, d_in, in_len, sel, n_sel,
                              d_scratch, scratch_cap, d_member_status, d_result, stream);
}

}  // extern "C"
