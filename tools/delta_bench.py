#!/usr/bin/env python3
"""What the delta transforms cost and what the delta frame buys (fsehip.h
section 2e).  One process, HIP events on one stream, all legs of a group
alternating; every output is checked once after the timing.

Transforms (--gib of raw bytes, element widths 2, 4 and 8, full-range random
elements), all in one run:

  copy    a device-to-device copy of the same bytes: one read and one write,
          the bound for a transform
  split   fsehip_planes_split        encode   fsehip_delta_encode
  merge   fsehip_planes_merge        decode   fsehip_delta_decode

End to end, on the two index tensors of DESIGN.md section 5 "Delta" scaled to
--gib (int64 sorted ids = cumsum of geometric(1/1000); int32 CSR offsets =
cumsum of poisson(40), which wraps at this size as the format allows):

  compress_delta / compress_planes      the _into forms, with both output sizes
  decompress_delta / decompress_planes
  range_1mib        one 1 MiB element range of each frame

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
        sys.exit("delta_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    n_bytes = int(a.gib * (1 << 30)) // 256 * 256
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}

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
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
        x = (x ^ (x >> 21)).to(ints[w])  # the low 8 w bits of 64 random ones
        p_image = torch.empty(codec.planes_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        d_image = torch.empty(codec.delta_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        p_back, d_back = torch.empty_like(x), torch.empty_like(x)
        flat = torch.empty(n * w, dtype=torch.uint8, device=dev)
        lib, st = codec.lib, codec._stream()
        p = lambda t: t.data_ptr()  # noqa: E731
        legs = {
            "copy": lambda: flat.copy_(x.view(torch.uint8)),
            "split": lambda: lib.fsehip_planes_split(w, p(x), n, p(p_image), st),
            "encode": lambda: lib.fsehip_delta_encode(w, p(x), n, p(d_image), st),
            "merge": lambda: lib.fsehip_planes_merge(w, p(p_image), n, p(p_back), st),
            "decode": lambda: lib.fsehip_delta_decode(w, p(d_image), n, p(d_back), st),
        }
        r = rates(timed(legs), 2 * n * w)
        for k in ("split", "encode", "merge", "decode"):
            r[k]["of_copy"] = round(r["copy"]["median_ms"] / r[k]["median_ms"], 3)
        r["encode"]["of_split"] = round(r["split"]["median_ms"] / r["encode"]["median_ms"], 3)
        r["decode"]["of_merge"] = round(r["merge"]["median_ms"] / r["decode"]["median_ms"], 3)
        # the image against torch: z of the first 2^20 elements, restarts at 4,096
        m = min(n, 1 << 20)
        xs = x[:m].to(torch.int64)
        d = xs.clone()
        d[1:] -= xs[:-1]
        d[::4096] = xs[::4096]
        d = d.to(ints[w])  # wrap to the width
        z = ((d << 1) ^ (d >> (8 * w - 1))).view(torch.uint8).view(-1, w)
        stride = (n + 15) // 16 * 16
        ok = all(torch.equal(d_image[k * stride: k * stride + m], z[:, k]) for k in range(w))
        return {"elem_bytes": w, "n_elems": n, "legs": r,
                "outputs_ok": bool(ok and torch.equal(d_back, x) and torch.equal(p_back, x))}

    def end_to_end(name, x):
        n, w = x.numel(), x.element_size()
        scratch = torch.empty(codec.delta_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        dbuf = torch.empty(codec.delta_bound(n, w), dtype=torch.uint8, device=dev)
        pbuf = torch.empty(codec.planes_bound(n, w), dtype=torch.uint8, device=dev)
        dlen, plen = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        comp = rates(timed({
            "compress_delta": lambda: codec.compress_delta_into(x, scratch, dbuf, dlen, res),
            "compress_planes": lambda: codec.compress_planes_into(x, scratch, pbuf, plen, res),
        }), n * w)
        dframe, pframe = dbuf[: int(dlen.item())], pbuf[: int(plen.item())]
        dinfo, dinner = codec.delta_info(dframe)
        pinfo, pinner = codec.planes_info(pframe)
        out = torch.empty_like(x)
        dst = torch.zeros(dinner.n_blocks, dtype=torch.int32, device=dev)
        pst = torch.zeros(pinner.n_blocks, dtype=torch.int32, device=dev)
        d_off, d_n = n // 2 + 12345, (1 << 20) // w
        rg = codec.planes_ranges([(d_off, d_n, 0)])
        rscratch = torch.empty(max(codec.delta_ranges_scratch_bytes(w, rg), codec.planes_ranges_scratch_bytes(w, rg)),
                               dtype=torch.uint8, device=dev)
        piece = torch.empty(d_n, dtype=x.dtype, device=dev)
        rst = torch.zeros(1, dtype=torch.int32, device=dev)

        def delta():
            codec.decompress_delta_into(dframe, dinfo, dinner, scratch, out, dst, res)

        def planes():
            codec.decompress_planes_into(pframe, pinfo, pinner, scratch, out, pst, res)

        def delta_range():
            codec.decompress_delta_ranges_into(dframe, dinfo, dinner, rg, rscratch, piece, rst, res)

        def planes_range():
            codec.decompress_planes_ranges_into(pframe, pinfo, pinner, rg, rscratch, piece, rst, res)

        dec = rates(timed({"decompress_delta": delta, "decompress_planes": planes}), n * w)
        rng = timed({"delta_range_1mib": delta_range, "planes_range_1mib": planes_range})
        ok = {}
        for k, fn in (("decompress_delta", delta), ("decompress_planes", planes)):
            out.zero_()
            fn()
            ok[k] = bool(torch.equal(out, x) and int(res[0]) == 0 and not bool((dst if fn is delta else pst).any()))
        for k, fn in (("delta_range_1mib", delta_range), ("planes_range_1mib", planes_range)):
            piece.zero_()
            fn()
            ok[k] = bool(torch.equal(piece, x[d_off: d_off + d_n]) and res.tolist() == [0, 0])
        return {"tensor": name, "elem_bytes": w, "n_elems": n, "raw_bytes": n * w, "delta_frame_bytes": dframe.numel(),
                "plane_frame_bytes": pframe.numel(), "delta_of_raw": round(dframe.numel() / (n * w), 4),
                "planes_of_raw": round(pframe.numel() / (n * w), 4),
                "delta_of_planes": round(dframe.numel() / pframe.numel(), 4),
                "compress": comp, "decompress": dec, "range": rng, "outputs_ok": ok}

    def sorted_ids():
        n = n_bytes // 8
        return torch.cumsum(torch.empty(n, device=dev).geometric_(1 / 1000).to(torch.int64), 0)

    def csr_offsets():
        n = n_bytes // 4
        return torch.cumsum(torch.poisson(torch.full((n,), 40.0, device=dev)).to(torch.int64), 0).to(torch.int32)

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup,
              "transforms": [transforms(w, n_bytes // w) for w in (2, 4, 8)],
              "end_to_end": [end_to_end("int64 sorted ids", sorted_ids()), end_to_end("int32 CSR offsets", csr_offsets())]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
