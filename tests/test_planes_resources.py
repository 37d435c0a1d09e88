"""Resource guard for the plane kernels (CPU test, no GPU needed): split,
merge and the pieces merge are bandwidth kernels that change bytes' places in
registers, so from the gfx950 code-object metadata inside libfsehip.so each of
their instances (2-, 4- and 8-byte elements) has no LDS and no private
segment (no register spills to scratch)."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

KERNELS = ["planes_split_kernel", "planes_merge_kernel", "planes_merge_pieces_kernel"]


@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("kernel", KERNELS)
def test_plane_kernels_use_registers_only(meta, kernel, w):
    tag = f"{len(kernel)}{kernel}ILi{w}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    md = meta[hits[0]]
    assert md[".group_segment_fixed_size"] == 0, (hits[0], md[".group_segment_fixed_size"])
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False)
    # 256 threads at <= 64 VGPRs: 8 workgroups per CU, the capped grid's count
    assert workgroups_per_cu(md) >= 8, (hits[0], md[".vgpr_count"])
