#!/usr/bin/env python3
"""What the byte-plane split costs and buys (the plane frame, fsehip.h
section 2d).  One process, HIP events on one stream, all legs of a group
alternating; every output is checked once after the timing.

Transforms (--gib of raw bytes, element widths 2 and 4, and once more with an
element count that is no multiple of 16):

  copy    a device-to-device copy of the same bytes: one read and one write,
          the bound for a transform
  split   fsehip_planes_split
  merge   fsehip_planes_merge
  torch   x.view(uint8).view(-1, w).t().contiguous(): the split in torch

End to end, on one bf16 randn * 0.02 tensor of --gib:

  compress_planes / compress_frame      the _into forms, with both output sizes
  decompress_planes / decompress_frame
  range_1mib        one 1 MiB element range (fsehip_planes_decompress_ranges)
  whole_then_slice  decompress_planes, then a copy of the same slice

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
        sys.exit("planes_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    n_bytes = int(a.gib * (1 << 30)) // 256 * 256

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

    def rates(legs, moved):
        """GB/s of bytes read plus bytes written, from the median."""
        for v in legs.values():
            v["gb_per_s"] = round(moved / (v["median_ms"] * 1e-3) / 1e9, 1)
        return legs

    def transforms(w, n):
        ints = {2: torch.int16, 4: torch.int32}[w]
        x = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int32, device=dev).to(ints)
        if w == 4:
            x = x * 65537
        image = torch.empty(codec.planes_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        back = torch.empty_like(x)
        flat = torch.empty(n * w, dtype=torch.uint8, device=dev)
        planes = torch.empty((w, n), dtype=torch.uint8, device=dev)
        lib, st = codec.lib, codec._stream()
        p = lambda t: t.data_ptr()  # noqa: E731
        legs = {
            "copy": lambda: flat.copy_(x.view(torch.uint8)),
            "split": lambda: lib.fsehip_planes_split(w, p(x), n, p(image), st),
            "merge": lambda: lib.fsehip_planes_merge(w, p(image), n, p(back), st),
            "torch": lambda: planes.copy_(x.view(torch.uint8).view(-1, w).t()),
        }
        r = rates(timed(legs), 2 * n * w)
        stride = (n + 15) // 16 * 16
        want = x.view(torch.uint8).view(-1, w).t()
        ok = all(torch.equal(image[k * stride: k * stride + n], want[k]) and not bool(image[k * stride + n: (k + 1) * stride].any())
                 for k in range(w))
        for k in ("split", "merge", "torch"):
            r[k]["of_copy"] = round(r["copy"]["median_ms"] / r[k]["median_ms"], 3)
        return {"elem_bytes": w, "n_elems": n, "legs": r, "outputs_ok": bool(ok and torch.equal(back, x))}

    def end_to_end():
        n = n_bytes // 2
        g = torch.Generator(device=dev).manual_seed(0x5EED0F00)
        x = (torch.randn(n, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        xb = x.view(torch.uint8)
        scratch = torch.empty(codec.planes_scratch_bytes(n, 2), dtype=torch.uint8, device=dev)
        pbuf = torch.empty(codec.planes_bound(n, 2), dtype=torch.uint8, device=dev)
        fbuf = torch.empty(codec.frame_bound(2 * n), dtype=torch.uint8, device=dev)
        plen, flen = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        comp = rates(timed({
            "compress_planes": lambda: codec.compress_planes_into(x, scratch, pbuf, plen, res),
            "compress_frame": lambda: codec.compress_frame_into(xb, fbuf, flen, res),
        }), 2 * n)
        pframe, fframe = pbuf[: int(plen.item())], fbuf[: int(flen.item())]
        info, inner = codec.planes_info(pframe)
        finfo = codec.frame_info(fframe)
        out = torch.empty(n, dtype=torch.bfloat16, device=dev)
        fout = torch.empty(2 * n, dtype=torch.uint8, device=dev)
        pst = torch.zeros(inner.n_blocks, dtype=torch.int32, device=dev)
        fst = torch.zeros(finfo.n_blocks, dtype=torch.int32, device=dev)
        d_off, d_n = n // 2 + 12345, (1 << 20) // 2
        rg = codec.planes_ranges([(d_off, d_n, 0)])
        rscratch = torch.empty(codec.planes_ranges_scratch_bytes(2, rg), dtype=torch.uint8, device=dev)
        piece = torch.empty(d_n, dtype=torch.bfloat16, device=dev)
        rst = torch.zeros(1, dtype=torch.int32, device=dev)

        def whole():
            codec.decompress_planes_into(pframe, info, inner, scratch, out, pst, res)

        def whole_then_slice():
            whole()
            piece.copy_(out[d_off: d_off + d_n])

        dec = rates(timed({
            "decompress_planes": whole,
            "decompress_frame": lambda: codec.decompress_frame_into(fframe, finfo, fout, fst, res),
        }), 2 * n)
        rng = timed({
            "range_1mib": lambda: codec.decompress_planes_ranges_into(pframe, info, inner, rg, rscratch, piece, rst, res),
            "whole_then_slice": whole_then_slice,
        })
        ok = {}
        out.zero_()
        whole()
        ok["decompress_planes"] = bool(torch.equal(out.view(torch.int16), x.view(torch.int16)) and int(res[0]) == 0)
        fout.zero_()
        codec.decompress_frame_into(fframe, finfo, fout, fst, res)
        ok["decompress_frame"] = bool(torch.equal(fout, xb))
        piece.zero_()
        codec.decompress_planes_ranges_into(pframe, info, inner, rg, rscratch, piece, rst, res)
        ok["range_1mib"] = bool(torch.equal(piece.view(torch.int16), x[d_off: d_off + d_n].view(torch.int16))
                                and res.tolist() == [0, 0])
        return {"n_elems": n, "raw_bytes": 2 * n, "plane_frame_bytes": pframe.numel(), "byte_frame_bytes": fframe.numel(),
                "size_ratio": round(pframe.numel() / fframe.numel(), 4), "compress": comp, "decompress": dec,
                "range": rng, "outputs_ok": ok}

    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup,
              "transforms": [transforms(2, n_bytes // 2), transforms(4, n_bytes // 4), transforms(2, n_bytes // 2 - 5),
                             transforms(4, n_bytes // 4 - 5)],
              "end_to_end": end_to_end()}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
