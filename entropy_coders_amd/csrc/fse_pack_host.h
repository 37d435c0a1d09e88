// fse_pack_host.h -- what the translation units of the pack frame and of the
// versioned pack share (fsehip.h sections 2j and 2k): the device descriptor
// of one member, the planner of fse_pack.cpp that fills it, and the launchers
// of fse_pack.hip and fse_vpack.hip, called by fse_capi_pack.cpp.  Plain C++ with no HIP include (a stream travels as
// void*), so that fse_pack.cpp builds with g++ alone.  Not part of the public
// ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/fsehip.h"

namespace fsehip {

constexpr uint32_t kPackHeaderBytes = 32;
constexpr uint32_t kPackEntryBytes = 16;

// One member as the kernels see it.  plane[k] is where byte k of its elements
// lies, from the base the kernel is given (the image, or the range scratch of a
// selected-member decode), a multiple of 16.  A tile is one workgroup's work:
// up to 256 consecutive 16-element groups of one member, FSEHIP_DELTA_RESTART
// elements; the member's first is first_tile and it has ceil(n_elems / 4096).
struct PackDesc {
    uint64_t ptr;  // the member's elements (split: source, merge: destination)
    uint64_t n_elems;
    uint64_t plane[8];
    uint64_t first_tile;
    uint32_t w;
    uint32_t kind;
    uint32_t status0;  // a selected member: its first plane range's status word
    uint32_t pad;
};
static_assert(sizeof(PackDesc) == 104, "uploaded as bytes");

inline uint64_t pack_head_bytes(uint64_t n) { return kPackHeaderBytes + kPackEntryBytes * n; }

// The two containers over this code: the pack frame (magic "FSEM", planes and
// delta members) and the versioned pack ("FSEV", diff members as well, whose
// base pointers travel behind the descriptors as one uint64_t per member).
enum PackFlavour { kFlavourPack = 0, kFlavourVpack = 1 };

// per member, what reaches the device: the descriptor, and a base pointer in the versioned pack
inline uint64_t pack_desc_bytes(PackFlavour f) { return sizeof(PackDesc) + (f == kFlavourVpack ? 8u : 0u); }

// FSE_OK and the two sums of a member list, or UNSUPPORTED: more members than
// FSEHIP_PACK_MAX_MEMBERS, a kind or width outside the flavour's lists, a sum
// that overflows.  Pointers are not looked at.
int pack_geom(const fsehip_pack_member* members, uint64_t n, uint64_t* image_bytes, uint64_t* content_bytes,
              PackFlavour f = kFlavourPack);

// the host calls of either container: fsehip_pack_* and fsehip_vpack_* are fronts of these
uint64_t pack_image_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members);
uint64_t pack_bound(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size);
uint64_t pack_scratch_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members);
uint64_t pack_members_scratch_bytes(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members,
                                    const uint32_t* sel, uint32_t n_sel);
uint64_t pack_plane_offset(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint32_t m,
                           uint32_t k);
int pack_read_header(PackFlavour f, const uint8_t* buf, size_t len, fsehip_pack_info* out);
int pack_read_members(PackFlavour f, const uint8_t* buf, size_t len, fsehip_pack_member* members,
                      uint32_t members_cap, fsehip_pack_info* out, fsehip_frame_info* inner);
int pack_write_header(PackFlavour f, const fsehip_pack_member* members, uint32_t n_members, uint8_t* out);

// The pointer checks of the versioned pack's device calls, over the members
// idx[0 .. n) of a valid list (idx nullptr: all n); members without elements
// take no part, and a base counts for a diff member only.
// a diff member with elements
bool pack_needs_base(const fsehip_pack_member& mb);
// every such member's base is there and aligned to its elements (bases may be nullptr when there is none)
bool pack_bases_ok(const fsehip_pack_member* members, const void* const* bases, const uint32_t* idx, uint32_t n);
// The decode side: no destination shares a byte with another destination, nor
// with the base of a diff member, except that a diff member's destination may
// be its base itself (the in-place update).  O(n log n).  bases nullptr: the
// destinations alone.
bool pack_decode_spans_ok(const fsehip_pack_member* members, const void* const* bases, const uint32_t* idx,
                          uint32_t n);

// The descriptors of a valid list with plane offsets into the image; returns the tile count.
uint64_t pack_plan(const fsehip_pack_member* members, uint32_t n, PackDesc* out);

// The selected members sel[0 .. n_sel) of a valid list, their planes decoded
// into scratch from offset 0 on, stride_m bytes each: one frame range per plane
// (member after member, byte 0 first), the descriptors with plane offsets into
// that scratch, the scratch bytes used (*planes_bytes, a multiple of 16) and
// the tile count.  BAD_ARG for a selection out of range or named twice.
int pack_plan_selected(const fsehip_pack_member* members, uint32_t n, const uint32_t* sel, uint32_t n_sel,
                       std::vector<PackDesc>* descs, std::vector<fsehip_frame_range>* ranges, uint64_t* planes_bytes,
                       uint64_t* tiles);

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t; d_descs is the device copy of n descriptors covering `tiles`.
int launch_pack_split(const PackDesc* d_descs, uint32_t n, uint64_t tiles, uint8_t* image, void* stream);
// `result`: the frame-status word (nullptr: none); BAD_FRAME there stores nothing
int launch_pack_merge(const PackDesc* d_descs, uint32_t n, uint64_t tiles, const uint8_t* planes,
                      const int32_t* result, void* stream);
// The versioned pack's transforms (fse_vpack.hip): as the two above, with
// d_bases[m] the base of member m's descriptor (read for diff members only).
int launch_vpack_split(const PackDesc* d_descs, const uint64_t* d_bases, uint32_t n, uint64_t tiles, uint8_t* image,
                       void* stream);
int launch_vpack_merge(const PackDesc* d_descs, const uint64_t* d_bases, uint32_t n, uint64_t tiles,
                       const uint8_t* planes, const int32_t* result, void* stream);
// encode: the head bytes at d_head to `out`, *out_len += head_bytes
int launch_pack_finish(const uint8_t* d_head, uint64_t head_bytes, uint8_t* out, uint64_t* out_len, void* stream);
// decode, after the frame call: the head bytes at `in` against d_head; on a
// difference result[0] = BAD_FRAME.  Then, with result[0] BAD_FRAME, every
// status (nullptr: none) BAD_FRAME and result[1] = n_status.  zero_count (the
// members call): result[1] = 0 either way, for the member-status launch to
// count into.
int launch_pack_check(const uint8_t* d_head, uint64_t head_bytes, const uint8_t* in, int32_t* result, int32_t* status,
                      uint64_t n_status, bool zero_count, void* stream);
// members: member_status[s] = the first failing status of the member's w plane
// ranges (BAD_FRAME for all when result[0] says so), result[1] += members with one
int launch_pack_member_status(const PackDesc* d_descs, uint32_t n_sel, const int32_t* plane_status,
                              int32_t* member_status, int32_t* result, void* stream);

}  // namespace fsehip
