"""Resource guard for the diff image's histogram (CPU test, no GPU needed),
from the gfx950 code-object metadata inside libfsehip.so: four instances of
diff_histogram_kernel (1-, 2-, 4- and 8-byte elements), each with the delta
histogram's LDS (16 KiB at 1 byte, 32 KiB otherwise), no private segment (no
register spills to scratch) and no dynamic stack, at most 128 VGPRs + AGPRs and
so at least 4 workgroups of 256 threads per CU -- at 8 bytes too, where the
lane holds two operands of 32 dwords.  The VGPR counts are the ones measured
when the kernel was written, pinned as tests/test_estimate_resources.py pins
the image histogram's."""
import pytest

from test_estimate_resources import clean
from test_kernel_resources import kernel_metadata, meta, workgroups_per_cu  # noqa: F401  (meta: the fixture)

# W -> (LDS bytes, VGPRs)
DIFF_HISTOGRAM = {1: (16384, 60), 2: (32768, 60), 4: (32768, 65), 8: (32768, 128)}


@pytest.mark.parametrize("w", sorted(DIFF_HISTOGRAM))
def test_diff_histogram_resources(meta, w):
    tag = f"21diff_histogram_kernelILi{w}EE"
    hits = [k for k in meta if tag in k]
    assert len(hits) == 1, (tag, hits)
    md = meta[hits[0]]
    lds, vgprs = DIFF_HISTOGRAM[w]
    print(f"\n[estimate] diff_histogram_kernel<{w}>: {md['.vgpr_count']} VGPRs, {md.get('.agpr_count', 0)} AGPRs, "
          f"{md['.sgpr_count']} SGPRs, {md['.group_segment_fixed_size']} B LDS, {workgroups_per_cu(md)} workgroups per CU")
    clean(md, hits[0])
    assert md[".max_flat_workgroup_size"] == 256
    assert md[".group_segment_fixed_size"] == lds, (hits[0], md[".group_segment_fixed_size"])
    assert md[".vgpr_count"] + md.get(".agpr_count", 0) <= 128
    assert workgroups_per_cu(md) >= 4, (hits[0], md[".vgpr_count"])
    assert md[".vgpr_count"] == vgprs, (hits[0], md[".vgpr_count"])


def test_four_instances(meta):
    assert len([k for k in meta if "21diff_histogram_kernel" in k]) == len(DIFF_HISTOGRAM)
