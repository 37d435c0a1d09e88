"""LDS layout guard of the encode kernels (CPU test, reads the code-object
metadata as test_kernel_resources.py does).

The one-wave encode kernels at L <= 11 keep the 16-copy sub-histogram as a
view over st / tt and the front of the phase-1 scratch instead of a member of
its own: 12,592 B, which is 10 LDS allocation granules of 1,280 B
(profiles/enc_occ/) and 12 workgroups per CU, where 14,768 B was 12 granules
and 10 per CU.  A byte over 12,800 B costs the twelfth workgroup; more than
168 allocated VGPRs costs the third wave per SIMD.  The L >= 12 kernels'
tables already exceed the sub-histograms: their sizes must not move."""
import pytest

from tests.test_kernel_resources import _find, kernel_metadata, meta  # noqa: F401  (meta: fixture)

LDS_GRANULE = 1280  # measured: tools/micro/occ_probe.hip, profiles/enc_occ/occ_probe_parent.txt
LDS_BYTES = 160 * 1024

OVERLAID = [
    "_ZN6fsehip20encode_blocks_kernelILi11ELi64ELi2EE",
    "_ZN6fsehip20encode_blocks_kernelILi11ELi64ELi1EE",
    "_ZN6fsehip21encode_streams_kernelILi11ELi64ELi2EE",
    "_ZN6fsehip21encode_streams_kernelILi11ELi64ELi1EE",
]

# static LDS bytes of the L = 12 .. 15 encode kernels before the overlay (blocks and streams, 2- and 1-state)
UNCHANGED = {12: 16928, 13: 24880, 14: 40960, 15: 73728}


@pytest.mark.parametrize("prefix", OVERLAID)
def test_overlaid_kernels_fit_twelve_per_cu(meta, prefix):  # noqa: F811
    md = _find(meta, prefix)
    lds = md[".group_segment_fixed_size"]
    assert lds <= 12800, (prefix, lds)
    granules = -(-lds // LDS_GRANULE)
    assert (LDS_BYTES // LDS_GRANULE) // granules >= 12, (prefix, lds)
    vgprs = -(-(md[".vgpr_count"] + md.get(".agpr_count", 0)) // 8) * 8
    assert vgprs <= 168, (prefix, md[".vgpr_count"])
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"


@pytest.mark.parametrize("lmax", sorted(UNCHANGED))
@pytest.mark.parametrize("kern", ["20encode_blocks_kernel", "21encode_streams_kernel"])
@pytest.mark.parametrize("ns", [2, 1])
def test_larger_tables_keep_their_sizes(meta, lmax, kern, ns):  # noqa: F811
    md = _find(meta, f"_ZN6fsehip{kern}ILi{lmax}ELi64ELi{ns}EE")
    assert md[".group_segment_fixed_size"] == UNCHANGED[lmax], (kern, lmax, ns)
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"


def test_two_blocks_per_wave_kernels_keep_their_sizes(meta):  # noqa: F811
    """The T = 32 path (two blocks per wave) is as it was."""
    assert _find(meta, "_ZN6fsehip20encode_blocks_kernelILi11ELi32ELi2EE")[".group_segment_fixed_size"] == 18752
    assert _find(meta, "_ZN6fsehip20encode_blocks_kernelILi12ELi32ELi2EE")[".group_segment_fixed_size"] == 27184
