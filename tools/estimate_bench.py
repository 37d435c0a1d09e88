#!/usr/bin/env python3
"""What the size estimate costs and what it saves (fsehip.h section 2g).  One
process, HIP events on one stream, all legs of a group alternating; every
output is checked once after the timing.

Histograms (--gib of raw bytes, element widths 2, 4 and 8), on full-range
random elements and on small ones (zero high planes, every lane on bin 0):

  copy             a device-to-device copy of the same bytes
  hist_frame       fsehip_histogram_blocks over the raw bytes
  planes_fused     fsehip_image_histogram, PLANES: the source read once, no image
  planes_two_step  fsehip_planes_split, then fsehip_histogram_blocks of the image
  delta_fused / delta_two_step   the same with fsehip_delta_encode

End to end, on the two index tensors of DESIGN.md section 5 "Delta" and on
bf16 weights, scaled to --gib:

  estimate         fsehip_estimate of all three kinds
  compress_frame / compress_planes / compress_delta   the _into forms: what
                   finding the smallest container costs without the estimate
  compress_auto    estimate, the 24-byte copy to the host, the chosen _into call

Prints one JSON object and, with --out, writes it there.  GPU only.
"""
import argparse
import ctypes as C
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

    from entropy_coders_amd import BlockCodec, estimate_choose

    if not torch.cuda.is_available():
        sys.exit("estimate_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    bs = codec.block_size
    n_bytes = int(a.gib * (1 << 30)) // 256 * 256
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}
    lib, st = codec.lib, codec._stream()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

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

    def histograms(w, n, data):
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
        x = (x ^ (x >> 21)).to(ints[w]) if data == "random" else (x & 127).to(ints[w])
        n_image = codec.planes_scratch_bytes(n, w)
        nb = codec.n_blocks(n_image)
        image = torch.empty(n_image, dtype=torch.uint8, device=dev)
        flat = torch.empty(n * w, dtype=torch.uint8, device=dev)
        cnt = {k: torch.zeros(nb * 256, dtype=torch.int32, device=dev)
               for k in ("frame", "planes_fused", "planes_two_step", "delta_fused", "delta_two_step")}

        def two_step(transform, key):
            transform(w, p(x), n, p(image), st)
            lib.fsehip_histogram_blocks(p(image), n_image, bs, p(cnt[key]), None, st)

        legs = {
            "copy": lambda: flat.copy_(x.view(torch.uint8)),
            "hist_frame": lambda: lib.fsehip_histogram_blocks(p(x), n * w, bs, p(cnt["frame"]), None, st),
            "planes_fused": lambda: lib.fsehip_image_histogram(1, w, p(x), n, bs, p(cnt["planes_fused"]), st),
            "planes_two_step": lambda: two_step(lib.fsehip_planes_split, "planes_two_step"),
            "delta_fused": lambda: lib.fsehip_image_histogram(2, w, p(x), n, bs, p(cnt["delta_fused"]), st),
            "delta_two_step": lambda: two_step(lib.fsehip_delta_encode, "delta_two_step"),
        }
        r = timed(legs)
        for k in ("planes", "delta"):
            r[k + "_fused"]["of_two_step"] = round(r[k + "_two_step"]["median_ms"] / r[k + "_fused"]["median_ms"], 3)
            r[k + "_fused"]["of_copy"] = round(r["copy"]["median_ms"] / r[k + "_fused"]["median_ms"], 3)
        ok = bool(torch.equal(cnt["planes_fused"], cnt["planes_two_step"])
                  and torch.equal(cnt["delta_fused"], cnt["delta_two_step"])
                  and int(cnt["planes_fused"].sum(dtype=torch.int64)) == n_image)
        return {"elem_bytes": w, "n_elems": n, "data": data, "legs": r, "outputs_ok": ok}

    def end_to_end(name, x):
        n, w = x.numel(), x.element_size()
        raw = x.view(torch.uint8)
        scratch = torch.empty(max(codec.delta_scratch_bytes(n, w), codec.estimate_scratch_bytes(x)), dtype=torch.uint8,
                              device=dev)
        bufs = {"frame": torch.empty(codec.frame_bound(n * w), dtype=torch.uint8, device=dev),
                "planes": torch.empty(codec.planes_bound(n, w), dtype=torch.uint8, device=dev),
                "delta": torch.empty(codec.delta_bound(n, w), dtype=torch.uint8, device=dev)}
        lens = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in bufs}
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        est = torch.zeros(3, dtype=torch.int64, device=dev)
        direct = {"frame": lambda: codec.compress_frame_into(raw, bufs["frame"], lens["frame"], res),
                  "planes": lambda: codec.compress_planes_into(x, scratch, bufs["planes"], lens["planes"], res),
                  "delta": lambda: codec.compress_delta_into(x, scratch, bufs["delta"], lens["delta"], res)}
        chosen = {}

        def auto():
            codec.estimate_into(x, scratch, est)
            host = est.cpu().numpy().view("uint64")
            chosen["kind"] = estimate_choose([int(v) for v in host])
            direct[chosen["kind"]]()

        legs = {"estimate": lambda: codec.estimate_into(x, scratch, est), "compress_auto": auto}
        legs.update({"compress_" + k: fn for k, fn in direct.items()})
        r = timed(legs)
        real = {k: int(v.item()) for k, v in lens.items()}
        estimates = {k: int(v) for k, v in zip(("frame", "planes", "delta"), est.cpu().numpy().view("uint64"))}
        three = sum(r["compress_" + k]["median_ms"] for k in direct)
        r["estimate"]["of_three_compresses"] = round(three / r["estimate"]["median_ms"], 2)
        r["compress_auto"]["over_direct"] = round(r["compress_auto"]["median_ms"]
                                                  / r["compress_" + chosen["kind"]]["median_ms"], 3)
        return {"tensor": name, "elem_bytes": w, "n_elems": n, "raw_bytes": n * w, "estimated_bytes": estimates,
                "real_bytes": real, "estimate_off": {k: round(estimates[k] / real[k] - 1, 5) for k in real},
                "chosen": chosen["kind"], "smallest": min(real, key=real.get), "three_compresses_ms": round(three, 4),
                "legs": r, "outputs_ok": chosen["kind"] == min(real, key=real.get)}

    def sorted_ids():
        n = n_bytes // 8
        return torch.cumsum(torch.empty(n, device=dev).geometric_(1 / 1000).to(torch.int64), 0)

    def csr_offsets():
        n = n_bytes // 4
        return torch.cumsum(torch.poisson(torch.full((n,), 40.0, device=dev)).to(torch.int64), 0).to(torch.int32)

    def bf16_weights():
        return (torch.randn(n_bytes // 2, device=dev) * 0.02).to(torch.bfloat16)

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": bs, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup,
              "histograms": [histograms(w, n_bytes // w, d) for w in (2, 4, 8) for d in ("random", "small")],
              "end_to_end": [end_to_end("int64 sorted ids", sorted_ids()),
                             end_to_end("int32 CSR offsets", csr_offsets()),
                             end_to_end("bf16 weights", bf16_weights())]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
