"""Resource guard for the diff kernels (CPU test, no GPU needed), from the
gfx950 code-object metadata inside libfsehip.so: every instance (1-, 2-, 4- and
8-byte elements) of the three kernels has no LDS, no private segment (no
register spills to scratch) and no dynamic stack, and keeps at least as many
256-thread workgroups per CU as delta_split_kernel of the same width keeps
(6 at 8-byte elements): the diff transforms hold two operands' registers
where the delta split holds one, and must not pay for them in occupancy.

What a CU keeps: test_kernel_resources.workgroups_per_cu is the register
file's share alone (512 / the allocation, per SIMD) and says 32, 16 and 12 for
delta_split_kernel at 1, 2 and 4 bytes.  A CU holds 32 waves, 8 per SIMD,
whatever the registers allow, so no kernel keeps more than 8 workgroups of 256
threads; the comparison is of min(8, that figure) on both sides: 8, 8, 8 and 6
workgroups, i.e. at most 64 VGPRs at 1, 2 and 4 bytes and at most 80 at 8."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

KERNELS = ["diff_split_kernel", "diff_merge_kernel", "diff_merge_pieces_kernel"]
CU_WAVES = 32  # the wave slots of a CU: 8 per SIMD


def one(meta, kernel, w):
    tag = f"{len(kernel)}{kernel}ILi{w}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    return meta[hits[0]]


def kept(md):
    """Workgroups a CU really keeps: by registers and LDS, and by its wave slots."""
    return min(workgroups_per_cu(md), CU_WAVES // (-(-md[".max_flat_workgroup_size"] // 64)))


def test_what_the_delta_split_keeps(meta):
    assert [kept(one(meta, "delta_split_kernel", w)) for w in (1, 2, 4, 8)] == [8, 8, 8, 6]


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("kernel", KERNELS)
def test_diff_kernel_resources(meta, kernel, w):
    md = one(meta, kernel, w)
    floor = kept(one(meta, "delta_split_kernel", w))
    print(f"\n[diff] {kernel}<{w}>: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, "
          f"{md['.group_segment_fixed_size']} B LDS, {kept(md)} workgroups per CU "
          f"(delta_split_kernel<{w}>: {floor})")
    assert md[".max_flat_workgroup_size"] == 256
    assert md[".group_segment_fixed_size"] == 0
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    assert kept(md) >= floor, (kernel, w, md[".vgpr_count"])
