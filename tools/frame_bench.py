#!/usr/bin/env python3
"""What the frame costs over the block codec (fsehip.h section 2b).

Input: the C2 workload (LUT p = 0.155, 64 KiB blocks, checkpoints every 64
pairs), 1 GiB by default.  Each repeat times, with HIP events on one stream
and alternating, so that all legs see the same box at the same time:

  encode            BlockCodec.compress_into alone (slot layout)
  encode+pack       compress_into + fsehip_pack_blocks into a preallocated
                    stream (offsets by a torch scan, no host sync): the
                    block codec's way to one contiguous buffer, at its best
  encode+pack_dev   compress_into + dist.pack_device as a caller uses it
                    (allocates, one host sync for the total)
  frame_compress    BlockCodec.compress_frame_into (no host sync)
  decode            decompress_into alone
  unpack+decode     fsehip_unpack_blocks (preallocated slots) + decompress_into
  unpack_dev+decode dist.unpack_device (allocates and zero-fills slots) + decompress_into
  frame_decompress  BlockCodec.decompress_frame_into

The packed stream of the baseline holds the block bytes only (its lengths and
checkpoints stay in separate arrays); the frame carries them, so it moves
8 * spb more bytes per FSE block.  A second input, uniform random bytes (all
RAW), shows the fallback: one encode plus one copy, frame = n + 4 nb + 32.

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
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ckpt", type=int, default=64)
    ap.add_argument("--chunk-blocks", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec, dist
    from entropy_coders_amd._lib import check

    if not torch.cuda.is_available():
        sys.exit("frame_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = a.mib << 20
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    lib, nb = codec.lib, codec.n_blocks(n)
    hs = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(legs, reps, warmup):
        """legs: name -> callable; per-repeat event times in ms, legs alternating."""
        times = {k: [] for k in legs}
        for r in range(warmup + reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= warmup:
                    times[k].append(e0.elapsed_time(e1))
        return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                    "max_ms": round(max(v), 4)} for k, v in times.items()}

    def run(name, src):
        cb = codec.alloc(n)
        packed = torch.empty(nb * codec.slot_bytes // 2 if name == "c2" else nb * codec.slot_bytes, dtype=torch.uint8,
                             device=dev)
        frame = torch.empty(codec.frame_bound(n), dtype=torch.uint8, device=dev)
        flen = torch.zeros(1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        st = torch.zeros(nb, dtype=torch.int32, device=dev)
        slots2 = torch.empty(nb * codec.slot_bytes, dtype=torch.uint8, device=dev)
        state = {}

        def pack_prealloc():
            codec.compress_into(src, cb)
            off = dist.exclusive_offsets(cb["comp_len"])
            check(lib.fsehip_pack_blocks(p(cb["out"]), codec.slot_bytes, p(cb["comp_len"]), p(off), nb, p(packed),
                                         hs()), "pack")
            state["off"] = off

        def pack_dev():
            codec.compress_into(src, cb)
            state["stream"], _ = dist.pack_device(cb["out"], codec.slot_bytes, cb["comp_len"])

        enc = {
            "encode": lambda: codec.compress_into(src, cb),
            "encode+pack": pack_prealloc,
            "encode+pack_dev": pack_dev,
            "frame_compress": lambda: codec.compress_frame_into(src, frame, flen, res, a.chunk_blocks),
        }
        r = {"encode_side": timed(enc, a.reps, a.warmup)}
        frame_len = int(flen.item())
        fr = frame[:frame_len]
        info = codec.frame_info(fr)
        comp_total = int(cb["comp_len"].to(torch.int64).sum())
        r.update(n_total=n, n_blocks=nb, frame_len=frame_len, blocks_not_fse=int(res[1]), packed_bytes=comp_total,
                 statuses_ok=bool((cb["status"] == 0).all()))
        all_ok = r["statuses_ok"]
        cb2 = dict(cb, out=slots2)

        def unpack_prealloc():
            check(lib.fsehip_unpack_blocks(p(packed), p(state["off"]), p(cb["comp_len"]), nb, p(slots2),
                                           codec.slot_bytes, hs()), "unpack")
            codec.decompress_into(cb2, out, st)

        def unpack_dev():
            s = dist.unpack_device(state["stream"], cb["comp_len"], codec.slot_bytes)
            codec.decompress_into(dict(cb, out=s), out, st)

        dec = {"frame_decompress": lambda: codec.decompress_frame_into(fr, info, out, st, res, a.chunk_blocks)}
        if all_ok:  # the block codec decodes only what it could encode
            dec = {"decode": lambda: codec.decompress_into(cb, out, st), "unpack+decode": unpack_prealloc,
                   "unpack_dev+decode": unpack_dev, **dec}
        r["decode_side"] = timed(dec, a.reps, a.warmup)
        # the last leg timed was the frame's: its output must be the input
        codec.decompress_frame_into(fr, info, out, st, res, a.chunk_blocks)
        torch.cuda.synchronize()
        r["frame_round_trip_ok"] = bool(torch.equal(out, src)) and int(res[0]) == 0 and int(res[1]) == 0
        return r

    result = {"device": torch.cuda.get_device_name(dev), "mib": a.mib, "block_size": codec.block_size,
              "ckpt_interval": a.ckpt, "chunk_blocks": a.chunk_blocks or 4096, "reps": a.reps, "warmup": a.warmup}
    result["c2"] = run("c2", codec.generate(0, 0.155, 0x5EED0002, n))
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0009)
    rnd = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)
    result["random"] = run("random", rnd)
    result["random"]["frame_is_n_plus_directory"] = result["random"]["frame_len"] == n + 4 * nb + 32
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
