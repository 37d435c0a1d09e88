// fse_decode.hip -- decode side of the batched FSE (tANS) block codec, gfx950:
// the host entry of the block decoders.  No kernel lives here; the kernels
// are one file per family, over the shared device pieces of
// fse_decode_dev.hpp:
//
//   fse_decode_tables.hip  hdr_parse_kernel, dtable_blocks_kernel: header
//                          parse and decode tables to HBM (launch_dtables)
//   fse_decode_seg.hip     decode_pre_kernel: segment-parallel decode on the
//                          sidecar, the block and its table staged in LDS
//   fse_decode_serial.hip  serial_ring_kernel with sym_map_kernel (L <= 12),
//                          serial2_decode_kernel and decode1_serial_kernel
//                          (L 13..15): sidecar-less decode, one lane per block
//   fse_decode_single.hip  single_ftab_kernel, single_decode_kernel: one
//                          stream on the scalar unit (launch_single)
//
// Wire format: the reference's fse_compress2 / fse_compress blocks
// (lib.rs:112-183): NCount header || backward bit stack + marker bit.
#include <cstdio>

#include "fse_decode_host.h"

namespace fsehip {

hipError_t launch_decode(const DecParams& P, uint32_t lmax, hipStream_t stream) {
    if (!P.dt || !P.dtinfo) return hipErrorInvalidValue;
    return P.sidecar ? launch_decode_seg(P, lmax, stream) : launch_decode_serial(P, lmax, stream);
}

int occupancy_line(char* buf, int len, int cap, const char* name, const void* k, int threads) {
    int nb = -1;
    hipFuncAttributes fa{};
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, threads, 0);
    (void)hipFuncGetAttributes(&fa, k);
    if (len < cap)
        len += snprintf(buf + len, cap - len, "%s: %d WG/CU (lds %zu B, vgpr %d)\n", name, nb, fa.sharedSizeBytes,
                        fa.numRegs);
    return len;
}

int occupancy_report_dec(char* buf, int cap) { return occupancy_lines_serial(buf, occupancy_lines_seg(buf, 0, cap), cap); }

}  // namespace fsehip
