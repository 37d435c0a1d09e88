#!/usr/bin/env python3
"""What decoding byte ranges of a frame costs (fsehip_frame_decompress_ranges,
fsehip.h section 2b) beside decoding the whole frame.

Input: the C2 workload (LUT p = 0.155, 64 KiB blocks, checkpoints every 64
pairs), one frame per --mib size (default 1024 and 256).  Each repeat times,
with HIP events on one stream and all legs alternating:

  a_whole_frame        fsehip_frame_decompress of the whole frame
  b_range_all_direct   one range = the whole frame, destination 16-byte
                       aligned: the direct route
  c_range_all_bounce   the same with the destination off by one byte: the
                       bounce route
  d_range_1mib         one 1 MiB range at an odd src_off in the middle
  e_ranges_4k          one 4 KiB range in every fourth block (4,096 ranges at
                       1 GiB), packed back to back, one call
  f_whole_then_slice_d what a user has without the call: a_whole_frame into a
                       scratch output, then one copy of the 1 MiB slice
  f_whole_then_slice_e a_whole_frame, then one strided copy of the 4 KiB
                       pieces (the cheapest way to collect them)

Every leg's output is compared with the input once, after the timing.  The
range calls include their host planner and the upload of its lists.
--only LEG runs one leg alone (for a kernel trace).  Prints one JSON object
and, with --out, writes it there.  GPU only.
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
    ap.add_argument("--mib", type=int, nargs="+", default=[1024, 256])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ckpt", type=int, default=64)
    ap.add_argument("--chunk-blocks", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec

    if not torch.cuda.is_available():
        sys.exit("frame_ranges_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    bs = codec.block_size

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

    def run(mib):
        n = mib << 20
        nb = codec.n_blocks(n)
        src = codec.generate(0, 0.155, 0x5EED0002, n)
        frame = codec.compress_frame(src)
        info = codec.frame_info(frame)
        full = torch.empty(n, dtype=torch.uint8, device=dev)       # leg a, and f's scratch output
        shifted = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        st = torch.zeros(nb, dtype=torch.int32, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        assert full.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
        d_off, d_len = n // 2 + 12345, 1 << 20
        out_d = torch.empty(d_len, dtype=torch.uint8, device=dev)
        e_blocks = list(range(0, nb, 4))
        e_in, e_len = 1001, 4096  # an odd place inside each block
        e_ranges = [(b * bs + e_in, e_len, i * e_len) for i, b in enumerate(e_blocks)]
        out_e = torch.empty(len(e_blocks) * e_len, dtype=torch.uint8, device=dev)
        rst1 = torch.zeros(1, dtype=torch.int32, device=dev)
        rst_e = torch.zeros(len(e_ranges), dtype=torch.int32, device=dev)
        e_view = full.as_strided((len(e_blocks), e_len), (4 * bs, 1), e_in)
        cbk = a.chunk_blocks

        def whole():
            codec.decompress_frame_into(frame, info, full, st, res, cbk)

        def slice_d():
            whole()
            out_d.copy_(full[d_off: d_off + d_len])

        def slice_e():
            whole()
            out_e.view(len(e_blocks), e_len).copy_(e_view)

        # the fsehip_frame_range arrays are built once: the legs time the C call, not Python lists
        rg_b, rg_c = codec.frame_ranges([(0, n, 0)]), codec.frame_ranges([(0, n, 1)])
        rg_d, rg_e = codec.frame_ranges([(d_off, d_len, 0)]), codec.frame_ranges(e_ranges)
        legs = {
            "a_whole_frame": whole,
            "b_range_all_direct": lambda: codec.decompress_frame_ranges_into(frame, info, rg_b, full, rst1, res, cbk),
            "c_range_all_bounce": lambda: codec.decompress_frame_ranges_into(frame, info, rg_c, shifted, rst1, res, cbk),
            "d_range_1mib": lambda: codec.decompress_frame_ranges_into(frame, info, rg_d, out_d, rst1, res, cbk),
            "e_ranges_4k": lambda: codec.decompress_frame_ranges_into(frame, info, rg_e, out_e, rst_e, res, cbk),
            "f_whole_then_slice_d": slice_d,
            "f_whole_then_slice_e": slice_e,
        }
        if a.only:
            legs = {a.only: legs[a.only]}
        r = {"n_total": n, "n_blocks": nb, "frame_len": frame.numel(), "e_ranges": len(e_ranges),
             "legs": timed(legs)}
        # every leg once more, checked against the input
        want_e = src.as_strided((len(e_blocks), e_len), (4 * bs, 1), e_in).reshape(-1)
        ok = {}
        for k, fn in legs.items():
            for t in (full, shifted, out_d, out_e):
                t.zero_()
            fn()
            torch.cuda.synchronize()
            good = int(res[0]) == 0 and int(res[1]) == 0
            if k in ("a_whole_frame", "b_range_all_direct"):
                good = good and torch.equal(full, src)
            elif k == "c_range_all_bounce":
                good = good and torch.equal(shifted[1: 1 + n], src)
            elif k in ("d_range_1mib", "f_whole_then_slice_d"):
                good = good and torch.equal(out_d, src[d_off: d_off + d_len])
            else:
                good = good and torch.equal(out_e, want_e)
            ok[k] = bool(good)
        r["outputs_ok"] = ok
        return r

    result = {"device": torch.cuda.get_device_name(dev), "block_size": bs, "ckpt_interval": a.ckpt,
              "chunk_blocks": a.chunk_blocks or 4096, "reps": a.reps, "warmup": a.warmup,
              "frames": {str(m): run(m) for m in a.mib}}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
