"""Resource guard for the member check record's kernels (CPU test, no GPU
needed), from the gfx950 code-object metadata inside libfsehip.so.  The units
kernel is the check record's CRC kernel over a descriptor table and keeps its
numbers, for the same reason: twenty 1 KiB tables in LDS (20,480 bytes, the
whole 160 KiB of a CU for 8 workgroups), nothing spilled to scratch, no
dynamic stack, at most 64 VGPRs, so 8 workgroups of 256 threads fit a CU --
the capped grid's count.  The combine and finish kernels use no scratch."""
import pytest

from test_kernel_resources import meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)
from test_pack_resources import find

UNITS_LDS = 20 * 1024
UNITS_VGPRS = 64
UNITS_WGS = 8


def test_units_kernel_resources(meta):
    md = find(meta, "mcheck_units_kernel")
    # the build this test came with has 51 VGPRs here (the check record's CRC kernel: see its own test)
    print(f"\n[spack] mcheck_units_kernel: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, "
          f"{md['.group_segment_fixed_size']} B LDS, {workgroups_per_cu(md)} workgroups per CU")
    assert md[".group_segment_fixed_size"] == UNITS_LDS, md[".group_segment_fixed_size"]
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= UNITS_VGPRS, md[".vgpr_count"]
    assert md[".max_flat_workgroup_size"] == 256
    assert workgroups_per_cu(md) == UNITS_WGS, (md[".vgpr_count"], workgroups_per_cu(md))


@pytest.mark.parametrize("kernel,lds", [("mcheck_combine_kernel", 4096 + 1024), ("mcheck_build_finish_kernel", 0),
                                        ("mcheck_verify_finish_kernel", 4), ("mcheck_gate_kernel", 0)])
def test_combine_and_finish_kernels_use_no_scratch(meta, kernel, lds):
    md = find(meta, kernel)
    print(f"\n[spack] {kernel}: {md['.vgpr_count']} VGPRs, {md['.group_segment_fixed_size']} B LDS")
    assert md[".group_segment_fixed_size"] == lds, md[".group_segment_fixed_size"]
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
