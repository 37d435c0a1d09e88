#!/usr/bin/env python3
"""What the diff transforms cost and what the diff frame buys (fsehip.h
section 2h).  One process, HIP events on one stream, all legs of a group
alternating; every output is checked once after the timing.

Transforms (--gib of raw bytes, element widths 2, 4 and 8, full-range random
elements and base), all in one run:

  copy      a device-to-device copy of the same bytes: one read and one write
  split     fsehip_planes_split      encode        fsehip_delta_encode
  merge     fsehip_planes_merge      decode        fsehip_delta_decode
  diff_encode                fsehip_diff_encode: two reads and one write
  diff_decode                fsehip_diff_decode into another tensor
  diff_decode_in_place       fsehip_diff_decode with d_dst == d_base

A diff transform moves three streams where the others move two, so each diff
leg is reported against the copy (of_copy) and against 1.5 x the copy's time
(of_copy_x1p5).

End to end, on the first two rows of DESIGN.md section 5 "Diff" scaled to
--gib of bf16 (bf16 copies of an fp32 master randn * 0.02, the master moved by
1e-4 * randn and by 1e-5 * randn):

  compress_diff / compress_planes       the _into forms, with both output sizes
  decompress_diff / decompress_planes
  range_1mib        one 1 MiB element range of each frame
  predicted         tests/diff_ref.py on the first 2^18 elements of the same
                    tensors: what the reference says the ratio should be

Prints one JSON object and, with --out, writes it there.  GPU only.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
        sys.exit("diff_bench needs a GPU")
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
        """GB/s of bytes read plus bytes written, from the median; `moved` a number or a dict by leg."""
        for k, v in legs.items():
            m = moved[k] if isinstance(moved, dict) else moved
            v["gb_per_s"] = round(m / (v["median_ms"] * 1e-3) / 1e9, 1)
        return legs

    def rand(w, n):
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
        return (x ^ (x >> 21)).to(ints[w])  # the low 8 w bits of 64 random ones

    def transforms(w, n):
        x, b = rand(w, n), rand(w, n)
        p_image = torch.empty(codec.planes_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        d_image = torch.empty(codec.delta_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        f_image = torch.empty(codec.diff_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        p_back, d_back, f_back = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        in_place = b.clone()
        flat = torch.empty(n * w, dtype=torch.uint8, device=dev)
        lib, st = codec.lib, codec._stream()
        p = lambda t: t.data_ptr()  # noqa: E731
        legs = {
            "copy": lambda: flat.copy_(x.view(torch.uint8)),
            "split": lambda: lib.fsehip_planes_split(w, p(x), n, p(p_image), st),
            "encode": lambda: lib.fsehip_delta_encode(w, p(x), n, p(d_image), st),
            "diff_encode": lambda: lib.fsehip_diff_encode(w, p(x), p(b), n, p(f_image), st),
            "merge": lambda: lib.fsehip_planes_merge(w, p(p_image), n, p(p_back), st),
            "decode": lambda: lib.fsehip_delta_decode(w, p(d_image), n, p(d_back), st),
            "diff_decode": lambda: lib.fsehip_diff_decode(w, p(f_image), n, p(f_back), p(b), st),
            "diff_decode_in_place": lambda: lib.fsehip_diff_decode(w, p(f_image), n, p(in_place), p(in_place), st),
        }
        diff_legs = ("diff_encode", "diff_decode", "diff_decode_in_place")
        r = rates(timed(legs), {k: (3 if k in diff_legs else 2) * n * w for k in legs})
        for k in legs:
            if k != "copy":
                r[k]["of_copy"] = round(r["copy"]["median_ms"] / r[k]["median_ms"], 3)
        for k in diff_legs:
            r[k]["of_copy_x1p5"] = round(1.5 * r["copy"]["median_ms"] / r[k]["median_ms"], 3)
        # the image against torch: z of the first 2^20 elements
        m = min(n, 1 << 20)
        d = (x[:m].to(torch.int64) - b[:m].to(torch.int64)).to(ints[w])  # wrap to the width
        z = ((d << 1) ^ (d >> (8 * w - 1))).view(torch.uint8).view(-1, w)
        stride = (n + 15) // 16 * 16
        ok = all(torch.equal(f_image[k * stride: k * stride + m], z[:, k]) for k in range(w))
        in_place.copy_(b)
        legs["diff_decode_in_place"]()
        return {"elem_bytes": w, "n_elems": n, "legs": r,
                "outputs_ok": bool(ok and torch.equal(f_back, x) and torch.equal(in_place, x)
                                   and torch.equal(d_back, x) and torch.equal(p_back, x))}

    def predicted(x, b):
        """tests/diff_ref.py on the first 2^18 elements: (diff, planes) as fractions of their raw bytes."""
        try:
            import diff_ref as DF
            import planes_ref as PR
        except ImportError:
            return None
        m = min(x.numel(), 1 << 18)
        xs, bs = (t[:m].view(ints[t.element_size()]).cpu().numpy() for t in (x, b))
        return {"n_elems": m, "diff_of_raw": round(len(DF.build(xs, bs, codec.block_size, a.ckpt, 2)) / xs.nbytes, 4),
                "planes_of_raw": round(len(PR.build(xs, codec.block_size, a.ckpt, 2)) / xs.nbytes, 4)}

    def end_to_end(name, x, b):
        n, w = x.numel(), x.element_size()
        scratch = torch.empty(codec.diff_scratch_bytes(n, w), dtype=torch.uint8, device=dev)
        dbuf = torch.empty(codec.diff_bound(n, w), dtype=torch.uint8, device=dev)
        pbuf = torch.empty(codec.planes_bound(n, w), dtype=torch.uint8, device=dev)
        dlen, plen = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        comp = rates(timed({
            "compress_diff": lambda: codec.compress_diff_into(x, b, scratch, dbuf, dlen, res),
            "compress_planes": lambda: codec.compress_planes_into(x, scratch, pbuf, plen, res),
        }), n * w)
        dframe, pframe = dbuf[: int(dlen.item())], pbuf[: int(plen.item())]
        dinfo, dinner = codec.diff_info(dframe)
        pinfo, pinner = codec.planes_info(pframe)
        out = torch.empty_like(x)
        dst = torch.zeros(dinner.n_blocks, dtype=torch.int32, device=dev)
        pst = torch.zeros(pinner.n_blocks, dtype=torch.int32, device=dev)
        d_off, d_n = n // 2 + 12345, (1 << 20) // w
        rg = codec.planes_ranges([(d_off, d_n, 0)])
        rscratch = torch.empty(max(codec.diff_ranges_scratch_bytes(w, rg), codec.planes_ranges_scratch_bytes(w, rg)),
                               dtype=torch.uint8, device=dev)
        piece = torch.empty(d_n, dtype=x.dtype, device=dev)
        rst = torch.zeros(1, dtype=torch.int32, device=dev)

        def diff():
            codec.decompress_diff_into(dframe, dinfo, dinner, b, scratch, out, dst, res)

        def planes():
            codec.decompress_planes_into(pframe, pinfo, pinner, scratch, out, pst, res)

        def diff_range():
            codec.decompress_diff_ranges_into(dframe, dinfo, dinner, rg, b, rscratch, piece, rst, res)

        def planes_range():
            codec.decompress_planes_ranges_into(pframe, pinfo, pinner, rg, rscratch, piece, rst, res)

        dec = rates(timed({"decompress_diff": diff, "decompress_planes": planes}), n * w)
        rng = timed({"diff_range_1mib": diff_range, "planes_range_1mib": planes_range})
        ok = {}
        bits = ints[w]
        for k, fn in (("decompress_diff", diff), ("decompress_planes", planes)):
            out.zero_()
            fn()
            ok[k] = bool(torch.equal(out.view(bits), x.view(bits)) and int(res[0]) == 0
                         and not bool((dst if fn is diff else pst).any()))
        for k, fn in (("diff_range_1mib", diff_range), ("planes_range_1mib", planes_range)):
            piece.zero_()
            fn()
            ok[k] = bool(torch.equal(piece.view(bits), x[d_off: d_off + d_n].view(bits)) and res.tolist() == [0, 0])
        return {"tensor": name, "elem_bytes": w, "n_elems": n, "raw_bytes": n * w,
                "unchanged_elements": round(float((x.view(bits) == b.view(bits)).float().mean()), 4),
                "diff_frame_bytes": dframe.numel(), "plane_frame_bytes": pframe.numel(),
                "diff_of_raw": round(dframe.numel() / (n * w), 4), "planes_of_raw": round(pframe.numel() / (n * w), 4),
                "diff_of_planes": round(dframe.numel() / pframe.numel(), 4), "predicted": predicted(x, b),
                "compress": comp, "decompress": dec, "range": rng, "outputs_ok": ok}

    def master_moved(step):
        n = n_bytes // 2
        w32 = torch.randn(n, device=dev) * 0.02
        return (w32 + step * torch.randn(n, device=dev)).bfloat16(), w32.bfloat16()

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup,
              "transforms": [transforms(w, n_bytes // w) for w in (2, 4, 8)],
              "end_to_end": [end_to_end("bf16 master 1e-4", *master_moved(1e-4)),
                             end_to_end("bf16 master 1e-5", *master_moved(1e-5))]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
