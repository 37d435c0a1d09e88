"""Resource guard for the check record's kernels (CPU test, no GPU needed),
from the gfx950 code-object metadata inside libfsehip.so: the CRC kernel's
three instances (build, verify, ranges) keep their twenty 1 KiB tables in LDS
(20,480 bytes, the whole 160 KiB of a CU for 8 workgroups), spill nothing to
scratch and stay at or below 64 VGPRs, so 8 workgroups of 256 threads fit a
CU: the capped grid's count (DESIGN.md section 5 "Check").  The finish
kernels hold the combine's multiplier tables and its reduction array."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

CRC_LDS = 20 * 1024
CRC_VGPRS = 64
CRC_WGS = 8


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["build", "verify", "ranges"])
def test_crc_kernel_resources(meta, mode):
    tag = f"16check_crc_kernelILi{mode}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    md = meta[hits[0]]
    assert md[".group_segment_fixed_size"] == CRC_LDS, (hits[0], md[".group_segment_fixed_size"])
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= CRC_VGPRS, (hits[0], md[".vgpr_count"])
    assert md[".max_flat_workgroup_size"] == 256
    assert workgroups_per_cu(md) == CRC_WGS, (hits[0], md[".vgpr_count"], workgroups_per_cu(md))


@pytest.mark.parametrize("kernel,lds", [("check_build_finish_kernel", 8192), ("check_verify_finish_kernel", 8192),
                                        ("check_status_kernel", 0), ("check_ranges_begin_kernel", 0)])
def test_finish_kernels_use_no_scratch(meta, kernel, lds):
    hits = [k for k in meta if f"{len(kernel)}{kernel}" in k]
    assert len(hits) == 1, (kernel, hits)
    md = meta[hits[0]]
    assert md[".group_segment_fixed_size"] == lds, (hits[0], md[".group_segment_fixed_size"])
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
