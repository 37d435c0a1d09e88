"""Resource guard for the size estimate's kernels (CPU test, no GPU needed),
from the gfx950 code-object metadata inside libfsehip.so: no instance has a
private segment (no register spills to scratch) or a dynamic stack; the image
histogram keeps its per-plane sub-histograms in 16 KiB (1-byte elements) or
32 KiB of LDS and at most 128 VGPRs, so at least 4 workgroups of 256 threads
fit a CU at every width; the per-block estimate is one wave on 2,564 bytes.
The VGPR counts are the ones measured when the kernels were written: a change
that moves them is looked at, not waved through."""
import pytest

from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

# (W, DELTA) -> (LDS bytes, VGPRs)
IMAGE_HISTOGRAM = {
    (1, True): (16384, 62),
    (2, True): (32768, 56),
    (4, True): (32768, 64),
    (8, True): (32768, 113),
    (2, False): (32768, 56),
    (4, False): (32768, 57),
    (8, False): (32768, 89),
}


def clean(md, name):
    assert md.get(".private_segment_fixed_size", 0) == 0, f"{name}: register spills to scratch"
    assert not md.get(".uses_dynamic_stack", False), name


@pytest.mark.parametrize("w,delta", sorted(IMAGE_HISTOGRAM))
def test_image_histogram_resources(meta, w, delta):
    tag = f"22image_histogram_kernelILi{w}ELb{int(delta)}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    md = meta[hits[0]]
    lds, vgprs = IMAGE_HISTOGRAM[(w, delta)]
    print(f"\n[estimate] image_histogram_kernel<{w}, {delta}>: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, "
          f"{md['.group_segment_fixed_size']} B LDS, {workgroups_per_cu(md)} workgroups per CU")
    clean(md, hits[0])
    assert md[".group_segment_fixed_size"] == lds, (hits[0], md[".group_segment_fixed_size"])
    assert md[".vgpr_count"] == vgprs, (hits[0], md[".vgpr_count"])
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= 128
    assert workgroups_per_cu(md) >= 4, (hits[0], md[".vgpr_count"])


def test_no_other_image_histogram_instance(meta):
    """The plane image has no 1-byte form: seven instances, not eight."""
    assert len([k for k in meta if "22image_histogram_kernel" in k]) == len(IMAGE_HISTOGRAM)


def test_estimate_blocks_resources(meta):
    hits = [k for k in meta if "22estimate_blocks_kernel" in k]
    assert len(hits) == 1, hits
    md = meta[hits[0]]
    print(f"\n[estimate] estimate_blocks_kernel: {md['.vgpr_count']} VGPRs, {md['.sgpr_count']} SGPRs, "
          f"{md['.group_segment_fixed_size']} B LDS")
    clean(md, hits[0])
    assert md[".group_segment_fixed_size"] == 2564 and md[".vgpr_count"] == 49
    init = [k for k in meta if "15est_init_kernel" in k]
    assert len(init) == 1
    clean(meta[init[0]], init[0])
    assert meta[init[0]][".group_segment_fixed_size"] == 0
