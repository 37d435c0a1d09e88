"""Resource guard for the delta kernels (CPU test, no GPU needed), from the
gfx950 code-object metadata inside libfsehip.so: every instance (1-, 2-, 4- and
8-byte elements) has no private segment (no register spills to scratch) and
no dynamic stack; the split keeps everything in registers; the two merge
kernels pass only their wave totals through LDS, within one 1,280-byte
granule; and at least 4 workgroups of 256 threads fit a CU."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

KERNELS = ["delta_split_kernel", "delta_merge_kernel", "delta_merge_pieces_kernel"]
LDS_GRANULE = 1280


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("kernel", KERNELS)
def test_delta_kernel_resources(meta, kernel, w):
    tag = f"{len(kernel)}{kernel}ILi{w}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    md = meta[hits[0]]
    lds = md[".group_segment_fixed_size"]
    print(f"\n[delta] {kernel}<{w}>: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, {lds} B LDS, "
          f"{workgroups_per_cu(md)} workgroups per CU")
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    if kernel == "delta_split_kernel":
        assert lds == 0, (hits[0], lds)
    else:
        assert 0 < lds <= LDS_GRANULE, (hits[0], lds)
    assert workgroups_per_cu(md) >= 4, (hits[0], md[".vgpr_count"])
