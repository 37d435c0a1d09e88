"""Encode time against resident workgroups per CU: FSEHIP_ENC_XLDS adds
dynamic LDS to each encode workgroup, lowering occupancy step by step
(diagnostics: is the encoder latency-bound or throughput-bound?).

LDS is allocated in granules of 1,280 B, 128 to a CU (measured:
tools/micro/occ_probe.hip, profiles/enc_occ/), so a count of workgroups per
CU is had by padding the kernel's static LDS to the most whole granules that
fit that many times.  (Up to round 6 this tool padded to 160 KiB / count - 64
bytes from a base of 17,472 B, on a 512 B granule model: the counts it
printed were mostly one above the real ones.)  For 10, 11 or 12 per CU the
launcher's own FSEHIP_ENC_WGS does the same; tools/enc_occ_ab.py times those."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the environment knobs this tool sets live only in the diagnostics build
os.environ.setdefault("FSEHIP_LIB", "libfsehip_diag.so")

import torch  # noqa: E402

from entropy_coders_amd import BlockCodec, _lib  # noqa: E402
from tools.ablate import timeit  # noqa: E402

LDS_CU = 160 * 1024
LDS_GRANULE = 1280
KERNEL = "_ZN6fsehip20encode_blocks_kernelILi11ELi64ELi2EE"  # C2 encode


def static_lds():
    """The kernel's static LDS bytes, from the code object of the library in use."""
    if "OCC_BASE_LDS" in os.environ:
        return int(os.environ["OCC_BASE_LDS"])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_kernel_resources import kernel_metadata

    md = kernel_metadata(_lib.LIB_PATH)
    (name,) = [k for k in md if k.startswith(KERNEL)]
    return md[name][".group_segment_fixed_size"]


def pad_for(wg, base):
    """Dynamic LDS bytes that leave exactly `wg` workgroups per CU (0: the kernel alone allows no more)."""
    per = LDS_CU // LDS_GRANULE // wg * LDS_GRANULE  # the most whole granules that fit wg times
    return max(0, per - base)


def resident(lds):
    return LDS_CU // LDS_GRANULE // -(-lds // LDS_GRANULE)


def main():
    n = int(os.environ.get("ABL_BYTES", 1 << 30))
    base = static_lds()
    print(f"static LDS {base} B = {-(-base // LDS_GRANULE)} granules: {resident(base)} workgroups per CU unpadded")
    for kind, prob, tlog in [(0, 0.155, 0), (2, 0.0, 11)]:
        codec = BlockCodec(table_log=tlog)
        src = codec.generate(kind, prob, 0x5EED0002, n)
        cb = codec.alloc(n)
        for wg in tuple(int(x) for x in os.environ.get("OCC_WGS", "12,11,10,9,8,7,6,5,4").split(",")):
            x = pad_for(wg, base)
            os.environ["FSEHIP_ENC_XLDS"] = str(x)
            t = timeit(lambda: codec.compress_into(src, cb), reps=5)
            print(f"kind={kind} p={prob} wg/cu={resident(base + x)} xlds={x}  {t:.4f} ms", flush=True)
        os.environ["FSEHIP_ENC_XLDS"] = "0"
        del cb, src


if __name__ == "__main__":
    main()
