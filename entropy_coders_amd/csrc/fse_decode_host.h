// fse_decode_host.h -- what the decoder's translation units share on the host
// side: the family launchers behind launch_decode (fse_decode.hip), the
// families' lines of occupancy_report_dec, and the one mapping of a runtime
// table log to a compile-time LMAX.  Internal to the fse_decode*.hip files.
#pragma once
#include <type_traits>

#include "fse_kernels.h"

namespace fsehip {

// f(std::integral_constant<int, LMAX>{}) for the kernels' LMAX that serves
// table logs up to lmax: 11, 12, 13, 14 or 15
template <class F>
void with_lmax(uint32_t lmax, F&& f) {
    if (lmax <= 11) f(std::integral_constant<int, 11>{});
    else if (lmax <= 12) f(std::integral_constant<int, 12>{});
    else if (lmax <= 13) f(std::integral_constant<int, 13>{});
    else if (lmax <= 14) f(std::integral_constant<int, 14>{});
    else f(std::integral_constant<int, 15>{});
}

// segment-parallel decode on the sidecar (fse_decode_seg.hip)
hipError_t launch_decode_seg(const DecParams& P, uint32_t lmax, hipStream_t stream);
// sidecar-less blocks, reference-mode host streams, sidecar recording (fse_decode_serial.hip)
hipError_t launch_decode_serial(const DecParams& P, uint32_t lmax, hipStream_t stream);

// occupancy_report_dec: one line for kernel k, appended at buf + len; returns
// the new length.  Each family appends the lines of its own kernels.
int occupancy_line(char* buf, int len, int cap, const char* name, const void* k, int threads = 256);
int occupancy_lines_seg(char* buf, int len, int cap);
int occupancy_lines_serial(char* buf, int len, int cap);

}  // namespace fsehip
