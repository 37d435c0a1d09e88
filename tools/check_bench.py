#!/usr/bin/env python3
"""What the check record costs (sealed buffers, fsehip.h section 2f).  One
process, HIP events on one stream, all legs of a group alternating; every
output is checked once after the timing.

The bare kernels over --gib of bytes, at check_log 16 and 12:

  copy       a device-to-device copy of the same bytes: one read and one write
  histogram  fsehip_histogram_blocks over the same bytes: the comparator, the
             same shape of work (every byte read once, one LDS access a byte)
  build      fsehip_check_build
  verify     fsehip_check_verify

End to end, on C2 data (the bench's generator, p = 0.155) and on a bf16
randn * 0.02 tensor through the plane frame, each of --gib:

  compress_sealed / compress    the _into forms of the sealed and the bare container
  decompress_sealed / decompress
  range_1mib_sealed / range_1mib  one 1 MiB range with and without its verify

Prints one JSON object and, with --out, writes it there.  GPU only.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ckpt", type=int, default=128)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec

    if not torch.cuda.is_available():
        sys.exit("check_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    n_bytes = int(a.gib * (1 << 30)) // 65536 * 65536
    lib, st = codec.lib, codec._stream()
    p = lambda t: t.data_ptr()  # noqa: E731

    def timed(legs):
        times = {k: [] for k in legs}
        for r in range(a.warmup + a.reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                    "max_ms": round(max(v), 4)} for k, v in times.items()}

    def read_rates(legs, n):
        for v in legs.values():
            v["gb_read_per_s"] = round(n / (v["median_ms"] * 1e-3) / 1e9, 1)
        return legs

    c2 = codec.generate(0, 0.155, 0x5EED0002, n_bytes)

    def bare(check_log):
        n_cb = (n_bytes + (1 << check_log) - 1) >> check_log
        rec = torch.empty(32 + 4 * n_cb, dtype=torch.uint8, device=dev)
        flat = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(256 * (n_bytes // 65536), dtype=torch.int32, device=dev)
        status = torch.zeros(n_cb, dtype=torch.int32, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        assert lib.fsehip_check_build(check_log, p(c2), n_bytes, p(rec), st) == 0
        info = codec.check_info(rec)
        legs = read_rates(timed({
            "copy": lambda: flat.copy_(c2),
            "histogram": lambda: lib.fsehip_histogram_blocks(p(c2), n_bytes, 65536, p(counts), None, st),
            "build": lambda: lib.fsehip_check_build(check_log, p(c2), n_bytes, p(rec), st),
            "verify": lambda: codec.check_verify_into(rec, info, c2, status, res),
        }), n_bytes)
        for k in ("build", "verify", "copy"):
            legs[k]["of_histogram"] = round(legs[k]["median_ms"] / legs["histogram"]["median_ms"], 3)
        import zlib

        ok = info.content_crc == zlib.crc32(c2.cpu().numpy().tobytes()) and res.tolist() == [0, 0]
        return {"check_log": check_log, "n_cb": n_cb, "legs": legs, "outputs_ok": bool(ok and not bool(status.any()))}

    def end_to_end(kind, x):
        n = x.numel()
        w = x.element_size()
        scratch = None
        if kind == "planes":
            scratch = torch.empty(codec.planes_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        sbuf = torch.empty(codec.sealed_bound(x, kind), dtype=torch.uint8, device=dev)
        bound = codec.frame_bound(n) if kind == "frame" else codec.planes_bound(n, w)
        bbuf = torch.empty(bound, dtype=torch.uint8, device=dev)
        slen, blen = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        res = torch.zeros(2, dtype=torch.int32, device=dev)

        def bare_compress():
            if kind == "frame":
                codec.compress_frame_into(x, bbuf, blen, res)
            else:
                codec.compress_planes_into(x, scratch, bbuf, blen, res)

        comp = timed({
            "compress_sealed": lambda: codec.compress_sealed_into(x, kind, sbuf, slen, res, scratch),
            "compress": bare_compress,
        })
        rec_bytes = codec.check_bytes(n * w)
        sealed_buf = sbuf[: rec_bytes + int(slen.item())]
        bare_buf = bbuf[: int(blen.item())]
        sealed = codec.sealed_info(sealed_buf)
        inner = codec.sealed_inner_info(kind, bare_buf)
        finfo = inner if kind == "frame" else inner[1]
        out = torch.empty_like(x)
        bst = torch.zeros(finfo.n_blocks, dtype=torch.int32, device=dev)
        cst = torch.zeros(sealed[0].n_cb, dtype=torch.int32, device=dev)
        cres = torch.zeros(2, dtype=torch.int32, device=dev)

        def bare_decompress():
            if kind == "frame":
                codec.decompress_frame_into(bare_buf, inner, out, bst, res)
            else:
                codec.decompress_planes_into(bare_buf, *inner, scratch, out, bst, res)

        dec = timed({
            "decompress_sealed": lambda: codec.decompress_sealed_into(sealed_buf, sealed, inner, out, bst, res, cst,
                                                                      cres, scratch),
            "decompress": bare_decompress,
        })
        d_off, d_n = (n // 2 + 12345) // (65536 // w) * (65536 // w), (1 << 20) // w  # whole check blocks
        piece = torch.empty(d_n, dtype=x.dtype, device=dev)
        rst = torch.zeros(1, dtype=torch.int32, device=dev)
        vst = torch.zeros(1, dtype=torch.int32, device=dev)
        if kind == "frame":
            rg = codec.frame_ranges([(d_off, d_n, 0)])
            bare_range = lambda: codec.decompress_frame_ranges_into(bare_buf, inner, rg, piece, rst, res)  # noqa: E731
        else:
            rg = codec.planes_ranges([(d_off, d_n, 0)])
            rscratch = torch.empty(codec.planes_ranges_scratch_bytes(w, rg), dtype=torch.uint8, device=dev)
            bare_range = lambda: codec.decompress_planes_ranges_into(bare_buf, *inner, rg, rscratch, piece, rst,  # noqa: E731
                                                                     res)
        vrg = codec.frame_ranges([(d_off * w, d_n * w, 0)])

        def sealed_range():
            bare_range()
            codec.check_verify_ranges_into(sealed_buf, sealed[0], vrg, piece, vst, cres)

        rng = timed({"range_1mib_sealed": sealed_range, "range_1mib": bare_range})
        out.zero_()
        codec.decompress_sealed_into(sealed_buf, sealed, inner, out, bst, res, cst, cres, scratch)
        ok = bool(torch.equal(out.view(torch.uint8), x.view(torch.uint8)) and cres.tolist() == [0, 0]
                  and not bool(cst.any()) and not bool(bst.any()))
        sealed_range()
        ok = ok and bool(torch.equal(piece.view(torch.uint8), x[d_off: d_off + d_n].view(torch.uint8))
                         and vst.tolist() == [0] and cres.tolist() == [0, 0])
        ok = ok and codec.check_ranges_verified_bytes(sealed[0], vrg) == d_n * w
        for legs, s, b in ((comp, "compress_sealed", "compress"), (dec, "decompress_sealed", "decompress"),
                           (rng, "range_1mib_sealed", "range_1mib")):
            legs["sealing_costs_ms"] = round(legs[s]["median_ms"] - legs[b]["median_ms"], 4)
        return {"kind": kind, "raw_bytes": n * w, "sealed_bytes": sealed_buf.numel(), "record_bytes": rec_bytes,
                "compress": comp, "decompress": dec, "range": rng, "outputs_ok": ok}

    g = torch.Generator(device=dev).manual_seed(0x5EED0F00)
    bf16 = (torch.randn(n_bytes // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16).view(torch.int16)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup, "bytes": n_bytes,
              "bare": [bare(16), bare(12)],
              "end_to_end": [end_to_end("frame", c2), end_to_end("planes", bf16)]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
