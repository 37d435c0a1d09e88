#!/usr/bin/env python3
"""What the estimate with a base costs and what it saves (fsehip.h section
2i).  One process, HIP events on one stream, all legs of a group alternating;
every output is checked once after the timing.  The method is
tools/estimate_bench.py's.

The diff image's histogram (--gib of raw bytes per tensor, element widths 2, 4
and 8), on a small step from a random base and on two unrelated tensors:

  copy            a device-to-device copy of one tensor's bytes
  diff_fused      fsehip_diff_image_histogram: both sources read once, no image
  diff_two_step   fsehip_diff_encode, then fsehip_histogram_blocks of the image

End to end, on bf16 weights after a 1e-4 step, on unrelated bf16 weights and
on an int32 table with 2 % of its rows replaced, scaled to --gib:

  estimate        fsehip_estimate_base of all four kinds
  compress_frame / compress_planes / compress_delta / compress_diff   the _into
                  forms: what finding the smallest container costs without it
  compress_auto   estimate, the 40-byte copy to the host, the chosen _into call

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

KINDS = ("frame", "planes", "delta", "diff")


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
        sys.exit("estimate_diff_bench needs a GPU")
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

    def rand(n, w):
        x = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=dev)
        return (x ^ (x >> 21)).to(ints[w])

    def histograms(w, n, data):
        base = rand(n, w)
        x = base + torch.randint(-64, 65, (n,), dtype=ints[w], device=dev) if data == "small step" else rand(n, w)
        n_image = codec.diff_scratch_bytes(n, w)
        nb = codec.n_blocks(n_image)
        image = torch.empty(n_image, dtype=torch.uint8, device=dev)
        flat = torch.empty(n * w, dtype=torch.uint8, device=dev)
        cnt = {k: torch.zeros(nb * 256, dtype=torch.int32, device=dev) for k in ("fused", "two_step")}

        def two_step():
            lib.fsehip_diff_encode(w, p(x), p(base), n, p(image), st)
            lib.fsehip_histogram_blocks(p(image), n_image, bs, p(cnt["two_step"]), None, st)

        legs = {
            "copy": lambda: flat.copy_(x.view(torch.uint8)),
            "diff_fused": lambda: lib.fsehip_diff_image_histogram(w, p(x), p(base), n, bs, p(cnt["fused"]), st),
            "diff_two_step": two_step,
        }
        r = timed(legs)
        r["diff_fused"]["of_two_step"] = round(r["diff_two_step"]["median_ms"] / r["diff_fused"]["median_ms"], 3)
        r["diff_fused"]["of_copy"] = round(r["copy"]["median_ms"] / r["diff_fused"]["median_ms"], 3)
        ok = bool(torch.equal(cnt["fused"], cnt["two_step"]) and int(cnt["fused"].sum(dtype=torch.int64)) == n_image)
        return {"elem_bytes": w, "n_elems": n, "data": data, "legs": r, "outputs_ok": ok}

    def end_to_end(name, x, base):
        n, w = x.numel(), x.element_size()
        raw = x.view(torch.uint8)
        scratch = torch.empty(max(codec.diff_scratch_bytes(n, w), codec.estimate_scratch_bytes(x, base=base)),
                              dtype=torch.uint8, device=dev)
        bufs = {"frame": torch.empty(codec.frame_bound(n * w), dtype=torch.uint8, device=dev),
                "planes": torch.empty(codec.planes_bound(n, w), dtype=torch.uint8, device=dev),
                "delta": torch.empty(codec.delta_bound(n, w), dtype=torch.uint8, device=dev),
                "diff": torch.empty(codec.diff_bound(n, w), dtype=torch.uint8, device=dev)}
        lens = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in bufs}
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        est = torch.zeros(5, dtype=torch.int64, device=dev)
        direct = {"frame": lambda: codec.compress_frame_into(raw, bufs["frame"], lens["frame"], res),
                  "planes": lambda: codec.compress_planes_into(x, scratch, bufs["planes"], lens["planes"], res),
                  "delta": lambda: codec.compress_delta_into(x, scratch, bufs["delta"], lens["delta"], res),
                  "diff": lambda: codec.compress_diff_into(x, base, scratch, bufs["diff"], lens["diff"], res)}
        chosen = {}

        def auto():
            codec.estimate_into(x, scratch, est, base=base)
            host = est.cpu().numpy().view("uint64")
            chosen["kind"] = estimate_choose([int(v) for v in host])
            direct[chosen["kind"]]()

        legs = {"estimate": lambda: codec.estimate_into(x, scratch, est, base=base), "compress_auto": auto}
        legs.update({"compress_" + k: fn for k, fn in direct.items()})
        r = timed(legs)
        real = {k: int(v.item()) for k, v in lens.items()}
        host = est.cpu().numpy().view("uint64")
        estimates = {k: int(host[i]) for k, i in zip(KINDS, (0, 1, 2, 4))}
        four = sum(r["compress_" + k]["median_ms"] for k in direct)
        r["estimate"]["of_four_compresses"] = round(four / r["estimate"]["median_ms"], 2)
        r["compress_auto"]["over_direct"] = round(r["compress_auto"]["median_ms"]
                                                  / r["compress_" + chosen["kind"]]["median_ms"], 3)
        return {"tensor": name, "elem_bytes": w, "n_elems": n, "raw_bytes": n * w, "estimated_bytes": estimates,
                "real_bytes": real, "estimate_off": {k: round(estimates[k] / real[k] - 1, 5) for k in real},
                "chosen": chosen["kind"], "smallest": min(real, key=real.get), "four_compresses_ms": round(four, 4),
                "legs": r, "outputs_ok": chosen["kind"] == min(real, key=real.get)}

    def bf16_step():
        w32 = torch.randn(n_bytes // 2, device=dev) * 0.02
        return (w32 + 1e-4 * torch.randn_like(w32)).to(torch.bfloat16), w32.to(torch.bfloat16)

    def bf16_unrelated():
        n = n_bytes // 2
        return ((torch.randn(n, device=dev) * 0.02).to(torch.bfloat16),
                (torch.randn(n, device=dev) * 0.02).to(torch.bfloat16))

    def int32_table():
        n = n_bytes // 4
        table = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device=dev)
        newer = torch.where(torch.rand(n, device=dev) < 0.02,
                            torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device=dev), table)
        return newer, table

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": bs, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup,
              "histograms": [histograms(w, n_bytes // w, d) for w in (2, 4, 8) for d in ("small step", "unrelated")],
              "end_to_end": [end_to_end("bf16 after a 1e-4 step", *bf16_step()),
                             end_to_end("bf16 unrelated", *bf16_unrelated()),
                             end_to_end("int32 table, 2% replaced", *int32_table())]}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
