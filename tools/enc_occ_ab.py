"""Encode time against resident workgroups per CU, by whole LDS granules
(diagnostics).  The library named by FSEHIP_LIB encodes 1 GiB of C2 data, of
near-uniform data at L = 11 and of skewed data at L = 9 and prints the median
of 7 HIP-event timings per input: once at the launcher's default, and, on a
diagnostics build (libfsehip_*diag.so: FSEHIP_ENC_WGS is live there), at the
default and at each count in OCC_WGS (default 10,11,12), three passes in
rotated order.  The C2 blocks' bytes, lengths, payload
bits, sidecar and statuses are checked against the digest file AB_DIGEST names
(written by the first run).  Run through tools/gpu_run.sh abpy:enc_occ_ab:...,
three alternating rounds over the builds."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FSEHIP_LIB", "libfsehip.so")
import torch  # noqa: E402

from entropy_coders_amd import BlockCodec  # noqa: E402
from tools.ablate import timeit  # noqa: E402

n = 1 << 30
lib = os.environ["FSEHIP_LIB"]
counts = [0]
if "diag" in lib:
    counts += [int(x) for x in os.environ.get("OCC_WGS", "10,11,12").split(",")]


def digest(cb):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    nb = cb["comp_len"].numel()
    blocks = cb["out"].view(nb, -1)
    keep = torch.arange(blocks.shape[1], device=blocks.device)[None, :] < cb["comp_len"][:, None]
    h.update(blocks[keep].cpu().numpy().tobytes())  # each block's compressed bytes, in order
    for key in ("comp_len", "payload_bits", "sidecar", "status"):
        h.update(cb[key].cpu().numpy().tobytes())
    return h.hexdigest()


for name, kind, prob, tlog in [("C2", 0, 0.155, 0), ("uniform L11", 2, 0.0, 11), ("skewed L9", 0, 0.77, 9)]:
    codec = BlockCodec(table_log=tlog)
    src = codec.generate(kind, prob, 0x5EED0002, n)
    cb = codec.alloc(n)
    # three passes over the counts, each starting one further on, so that a drift over the
    # process's lifetime does not fall on the same count every time
    ms = {wgs: [] for wgs in counts}
    for p in range(3 if len(counts) > 1 else 1):
        for wgs in counts[p % len(counts):] + counts[:p % len(counts)]:
            os.environ["FSEHIP_ENC_WGS"] = str(wgs)
            ms[wgs].append(timeit(lambda: codec.compress_into(src, cb), reps=7))
    out = [f"wgs={wgs or 'default'} " + " / ".join(f"{t:.4f}" for t in ms[wgs]) + " ms" for wgs in counts]
    path = os.environ.get("AB_DIGEST")
    if name == "C2" and path:
        for wgs in counts:
            os.environ["FSEHIP_ENC_WGS"] = str(wgs)
            codec.compress_into(src, cb)
            d = digest(cb)
            if not os.path.exists(path):
                open(path, "w").write(d)
            elif open(path).read().strip() != d:
                print(f"{lib}: {name} wgs={wgs}: bytes DIFFER", flush=True)
                sys.exit(1)
        out.append("bytes same")
    print(f"{lib}: {name}: " + ", ".join(out), flush=True)
    del src, cb
    torch.cuda.empty_cache()
