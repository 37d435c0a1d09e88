"""Resource guard for the versioned pack's kernels (CPU test, no GPU needed),
from the gfx950 code-object metadata inside libfsehip.so, as
tests/test_pack_resources.py.  Each of the two is one kernel for every width
and all three kinds, so its registers are those of its widest case: no
private segment (no register spills to scratch), no dynamic stack; the split
keeps everything in registers; the merge passes only the delta sum's wave
totals through LDS, no more than delta_merge_kernel<8> does; and the VGPRs
recorded here leave at least 4 workgroups of 256 threads per CU.  The pack
frame's own kernels are still there under their own names, once each."""
import pytest

from test_kernel_resources import meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)
from test_pack_resources import find

# VGPRs recorded from the build this test came with: 82 for the split (the
# pack split's 82, set by 8-byte delta elements; diff_split_kernel<8> has 73)
# and 81 for the merge, set by 8-byte diff elements, whose planes, base and
# elements are live together (diff_merge_kernel<8> has 73, pack_merge_kernel
# 58).  The limits are the next multiples of the 8-register granule: the same
# workgroups per CU, 5.
VGPR_LIMIT = {"vpack_split_kernel": 88, "vpack_merge_kernel": 88}


@pytest.mark.parametrize("kernel", ["vpack_split_kernel", "vpack_merge_kernel"])
def test_vpack_kernel_resources(meta, kernel):
    md = find(meta, kernel)
    lds = md[".group_segment_fixed_size"]
    print(f"\n[vpack] {kernel}: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, {lds} B LDS, "
          f"{workgroups_per_cu(md)} workgroups per CU")
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    assert md[".max_flat_workgroup_size"] == 256
    delta8 = [meta[k] for k in meta if "18delta_merge_kernelILi8EE" in k]
    assert len(delta8) == 1
    if kernel == "vpack_split_kernel":
        assert lds == 0, lds
    else:
        assert 0 < lds <= delta8[0][".group_segment_fixed_size"], (lds, delta8[0][".group_segment_fixed_size"])
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= VGPR_LIMIT[kernel], md[".vgpr_count"]
    assert workgroups_per_cu(md) >= 4, md[".vgpr_count"]


@pytest.mark.parametrize("kernel", ["pack_split_kernel", "pack_merge_kernel"])
def test_the_pack_kernels_are_still_found_once(meta, kernel):
    find(meta, kernel)  # asserts exactly one symbol with the kernel's mangled name
