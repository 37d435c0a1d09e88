"""Resource guard for the pack kernels (CPU test, no GPU needed), from the
gfx950 code-object metadata inside libfsehip.so.  Each of the two is one
kernel for every width and kind (the switch is uniform per workgroup), so its
registers are those of its widest case: no private segment (no register spills
to scratch), no dynamic stack; the split keeps everything in registers; the
merge passes only the delta sum's wave totals through LDS, no more than
delta_merge_kernel<8> does; and the VGPRs recorded here leave at least 4
workgroups of 256 threads per CU, the delta kernels' floor."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

# VGPRs recorded from the build this test came with: 82 for the split and 58
# for the merge, set by the widest case, 8-byte delta elements
# (delta_split_kernel<8> has 76, delta_merge_kernel<8> 60).  The limits are
# the next multiples of the 8-register granule: the same workgroups per CU.
VGPR_LIMIT = {"pack_split_kernel": 88, "pack_merge_kernel": 64}


def find(meta, kernel):
    hits = [k for k in meta if f"{len(kernel)}{kernel}E" in k]
    assert len(hits) == 1, (kernel, hits)
    return meta[hits[0]]


@pytest.mark.parametrize("kernel", ["pack_split_kernel", "pack_merge_kernel"])
def test_pack_kernel_resources(meta, kernel):
    md = find(meta, kernel)
    lds = md[".group_segment_fixed_size"]
    print(f"\n[pack] {kernel}: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, {lds} B LDS, "
          f"{workgroups_per_cu(md)} workgroups per CU")
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    assert md[".max_flat_workgroup_size"] == 256
    delta8 = [meta[k] for k in meta if "18delta_merge_kernelILi8EE" in k]
    assert len(delta8) == 1
    if kernel == "pack_split_kernel":
        assert lds == 0, lds
    else:
        assert 0 < lds <= delta8[0][".group_segment_fixed_size"], (lds, delta8[0][".group_segment_fixed_size"])
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= VGPR_LIMIT[kernel], md[".vgpr_count"]
    assert workgroups_per_cu(md) >= 4, md[".vgpr_count"]
