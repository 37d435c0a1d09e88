// fse_mcheck_host.h -- what the translation units of the member check record
// and of the sealed pack share (fsehip.h section 2l): the device descriptor of
// one checked span, the planner of fse_mcheck.cpp that fills it, the scratch
// layout, and the launchers of fse_mcheck.hip, called by fse_capi_spack.cpp.
// Plain C++ with no HIP include (a stream travels as void*), so that
// fse_mcheck.cpp builds with g++ alone.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fsehip.h"
#include "fse_check_host.h"
#include "fse_pack_host.h"

namespace fsehip {

constexpr uint32_t kMcheckHeaderBytes = 32;
constexpr uint32_t kMcheckEntryBytes = 8;

// A work unit: up to 64 KiB of one span, counted from the span's own byte 0.
// An implementation constant: the format does not know it.
constexpr uint32_t kMcheckUnitLog = 16;
constexpr uint64_t kMcheckUnit = 1ull << kMcheckUnitLog;
// The combine: a span of up to kMcheckSerialUnits units is folded by one
// thread; a longer one by a workgroup, kMcheckRun units per thread and a tree
// over the kMcheckCombineThreads runs of a chunk.
constexpr uint32_t kMcheckSerialUnits = 64;
constexpr uint32_t kMcheckRun = 16, kMcheckCombineThreads = 256, kMcheckCombineLevels = 8;

// One span as the kernels see it: a member's content or a diff member's base.
// k_full / k_last: the init value's share (crc::init_share) of a full unit and
// of the span's last unit at this pointer's alignment mod 16 -- the same for
// every unit of the span, a unit being a multiple of 16.  x_last: x^(8 * bytes
// of the last unit), the combine's last step.  `member`: the record's table
// entry the span is compared with or written to.
struct McheckDesc {
    uint64_t ptr;
    uint64_t bytes;  // 0: no unit, CRC 0
    uint64_t first_unit;
    uint32_t k_full;
    uint32_t k_last;
    uint32_t x_last;
    uint32_t member;
};
static_assert(sizeof(McheckDesc) == 40, "uploaded as bytes");

constexpr uint64_t mcheck_units_of(uint64_t bytes) {
    return (bytes >> kMcheckUnitLog) + ((bytes & (kMcheckUnit - 1u)) ? 1u : 0u);
}

enum McheckWhich { kMcheckContent = 0, kMcheckBase = 1 };

// The descriptors of the members idx[0 .. n) (nullptr: all n) of a valid list,
// units numbered from first_unit on.  kMcheckContent: every member's
// n_elems * w bytes at ptrs[m] (ptrs nullptr: at its d_ptr).  kMcheckBase: the
// same bytes at ptrs[m] for a diff member with elements, no bytes for any
// other.  Returns the unit after the last; *n_long (may be nullptr) += the
// spans above kMcheckSerialUnits.
uint64_t mcheck_plan(const fsehip_pack_member* members, const void* const* ptrs, const uint32_t* idx, uint32_t n,
                     int which, uint64_t first_unit, McheckDesc* out, uint32_t* n_long);

// Scratch of the kernels, from a 16-byte aligned address: 64 bytes (the gate
// word of the sealed decode), the descriptors of both lists back to back (one
// upload), then per list the unit CRCs and the span CRCs.
struct McheckList {
    uint64_t n, units;                      // in: spans and units
    uint64_t desc_off, unit_off, span_off;  // out: byte offsets into the scratch
};
constexpr uint64_t kMcheckGateBytes = 64;
uint64_t mcheck_layout(McheckList* lists, uint32_t n_lists);

// The launchers return an FSE status (FSE_OK or FSE_ERR_HIP).  `stream` is a
// hipStream_t; d_descs the device copy of n descriptors covering `units`.
// unit_crc[u] = the CRC-32 of unit u, for all units: one launch, grid capped.
int launch_mcheck_units(const McheckDesc* d_descs, uint32_t n, uint64_t units, uint32_t* unit_crc, void* stream);
// span_crc[i] = the units of span i combined (0 without units): one launch
int launch_mcheck_combine(const McheckDesc* d_descs, uint32_t n, uint32_t n_long, const uint32_t* unit_crc,
                          uint32_t* span_crc, void* stream);
// build: the 32 header bytes and the table to `record`; entry m = span_crc[m]
// and, with_bases, span_crc[n + m].  out_len (nullptr: none): *out_len += add,
// unless `result` (the pack compress's status word; nullptr: none) holds an error.
int launch_mcheck_build_finish(const uint8_t hdr[32], const uint32_t* span_crc, uint32_t n, bool with_bases,
                               uint8_t* record, uint64_t* out_len, uint64_t add, const int32_t* result, void* stream);
// verify: the header on the device against hdr; span i against word `which` of
// entry descs[i].member; status[i] (nullptr: none) OK / CHECKSUM, BAD_FRAME for
// all on another header.  active false: nothing was computed, every span OK.
//   kMcheckAlone    result[0] = OK / CHECKSUM / BAD_FRAME, result[1] = failed spans
//   kMcheckBases    result[0] likewise, result[1] = 0, result[2] = failed, result[3] = 0;
//                   gate[0] = BAD_FRAME when one failed or the header differs, else OK
//   kMcheckContents result[1] = failed; result[0] BAD_FRAME on another header, CHECKSUM
//                   when one failed and it held OK, kept otherwise
enum McheckMode { kMcheckAlone = 0, kMcheckBases = 1, kMcheckContents = 2 };
int launch_mcheck_verify_finish(const uint8_t hdr[32], const uint8_t* record, const McheckDesc* d_descs, uint32_t n,
                                int which, bool active, const uint32_t* span_crc, int32_t* status, int32_t* result,
                                int mode, int32_t* gate, void* stream);
// the sealed decode's gate: gate[0] = BAD_FRAME when result[0] is, kept otherwise
int launch_mcheck_gate(const int32_t* result, int32_t* gate, void* stream);

// The pack calls of fse_capi_pack.cpp as the sealed pack uses them: the
// implementations behind fsehip_pack_* and fsehip_vpack_*, the decodes in their
// two halves.  *_check: every check the pack call makes before any device use
// (but NO_DEVICE, the caller's), for the pack's share of the scratch.  *_launch: the launches, for arguments
// that passed the check.  `gate`: a device word that the merge is handed in
// place of d_result after the frame's BAD_FRAME has joined it on the device; a
// gate launch that fails ends the call without a merge.
struct PackMembersPlan {  // what pack_members_check leaves for pack_members_launch
    std::vector<PackDesc> descs;
    std::vector<fsehip_frame_range> ranges;
    uint64_t planes_bytes = 0, tiles = 0;
};
int pack_compress_impl(PackFlavour f, const fsehip_frame_params* p, const fsehip_pack_member* members,
                       uint32_t n_members, const void* const* bases, uint8_t* d_scratch, uint64_t scratch_cap,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result, void* stream);
int pack_decompress_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                          const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in,
                          uint64_t in_len, const uint8_t* d_scratch, uint64_t scratch_cap, const int32_t* d_result);
int pack_decompress_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                           const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                           const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, int32_t* d_block_status,
                           int32_t* d_result, int32_t* gate, void* stream);
int pack_members_check(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                       const void* const* bases, const fsehip_frame_info* inner, const uint8_t* d_in, uint64_t in_len,
                       const uint32_t* sel, uint32_t n_sel, const uint8_t* d_scratch, uint64_t scratch_cap,
                       const int32_t* d_result, PackMembersPlan* plan);
int pack_members_launch(PackFlavour f, const fsehip_pack_info* info, const fsehip_pack_member* members,
                        const void* const* bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                        const uint8_t* d_in, uint64_t in_len, const uint32_t* sel, uint32_t n_sel,
                        const PackMembersPlan& plan, uint8_t* d_scratch, int32_t* d_member_status, int32_t* d_result,
                        int32_t* gate, void* stream);

}  // namespace fsehip
