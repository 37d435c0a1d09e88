#!/usr/bin/env python3
"""What the versioned pack costs and what it buys (fsehip.h section 2k): the
next checkpoint against the previous one.  One process, all legs of a group
alternating round by round, medians reported; every output is checked once
after the timing.

(a) one large member: --gib of bf16 bits as ONE diff member through
    fsehip_vpack_split / fsehip_vpack_merge (out of place and in place),
    against fsehip_diff_encode / fsehip_diff_decode of the same tensors and
    1.5 device-to-device copies of the tensor's bytes: the transform reads
    two streams and writes one (HIP events on one stream).

(b) the synthetic checkpoint of tools/pack_bench.py (--members bf16 tensors
    of 256 to 2^22 elements, plus fp32 and int64 tensors) after a step of
    --steps (1e-4 and 1e-5 of randn noise on the fp32 master; the int64
    counters advance by one): compress_pack(bases=) / decompress_pack(bases=)
    out of place and in place, against the loop of compress_diff /
    decompress_diff over the same tensors and compress_pack / decompress_pack
    without bases.  The _into forms on preallocated buffers (host wall clock
    from the first call to the end of the stream, and the host time until the
    last call returned) and the Python calls as a user writes them.  Kernel
    launches are counted once per leg with torch.profiler where that works;
    sizes are the containers' lengths.

The loop and the pack without bases are the yardsticks.  Prints one JSON
object and, with --out, writes it there.  GPU only.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--steps", type=float, nargs="+", default=[1e-4, 1e-5])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ckpt", type=int, default=128)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec

    if not torch.cuda.is_available():
        sys.exit("vpack_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    lib, st = codec.lib, codec._stream()
    u8 = torch.uint8

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed_events(legs):
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
        return {k: summary(v) for k, v in times.items()}

    def timed_wall(legs):
        """Host wall clock of fn() plus the stream's end, and of fn() alone (the enqueue)."""
        total, enq = {k: [] for k in legs}, {k: [] for k in legs}
        for r in range(a.warmup + a.reps):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r >= a.warmup:
                    total[k].append((t2 - t0) * 1e3)
                    enq[k].append((t1 - t0) * 1e3)
        return {k: dict(summary(total[k]), enqueue_median_ms=round(statistics.median(enq[k]), 4)) for k in legs}

    def launches(fn):
        """Kernel launches of one fn(), counted by torch.profiler; None where it cannot."""
        if a.no_launch_count:
            return None
        try:
            from torch.profiler import ProfilerActivity, profile

            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = 0
            for e in prof.events():
                if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower() \
                        and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                    n += 1
            return n or None
        except Exception as e:  # the count is extra: the timings stand without it
            return f"unavailable: {type(e).__name__}"

    # ------------------------------------------------------------ (a) one large member
    def one_large_member():
        n = int(a.gib * (1 << 30)) // 2 // 256 * 256
        w32 = torch.randn(n, device=dev) * 0.02
        base = w32.to(torch.bfloat16).view(torch.int16)
        x = (w32 + 1e-4 * torch.randn(n, device=dev)).to(torch.bfloat16).view(torch.int16)
        del w32
        names, barr = codec.pack_bases([x], [base])
        members = codec.pack_members([x], names, versioned=True)
        image_bytes = int(lib.fsehip_vpack_image_bytes(members, 1))
        k_image = torch.empty(image_bytes, dtype=u8, device=dev)
        d_image = torch.empty(codec.diff_scratch_bytes(n, 2), dtype=u8, device=dev)
        extra = torch.empty(codec.pack_scratch_bytes(members, 1, versioned=True) - image_bytes, dtype=u8, device=dev)
        k_back, d_back = torch.empty_like(x), torch.empty_like(x)
        k_place, d_place = base.clone(), base.clone()  # the in-place legs: decoded over and over, checked after a reset
        back_members = codec.pack_members([k_back], names, versioned=True)
        place_members = codec.pack_members([k_place], names, versioned=True)
        _, place_barr = codec.pack_bases([k_place], [k_place])
        flat = torch.empty(3 * n, dtype=u8, device=dev)
        src3 = torch.empty(3 * n, dtype=u8, device=dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        legs = {
            "copy_1p5": lambda: flat.copy_(src3),
            "diff_encode": lambda: lib.fsehip_diff_encode(2, p(x), p(base), n, p(d_image), st),
            "vpack_split": lambda: lib.fsehip_vpack_split(members, 1, barr, p(k_image), p(extra), extra.numel(), st),
            "diff_decode": lambda: lib.fsehip_diff_decode(2, p(d_image), n, p(d_back), p(base), st),
            "vpack_merge": lambda: lib.fsehip_vpack_merge(back_members, 1, barr, p(k_image), p(extra), extra.numel(), st),
            "diff_decode_in_place": lambda: lib.fsehip_diff_decode(2, p(d_image), n, p(d_place), p(d_place), st),
            "vpack_merge_in_place": lambda: lib.fsehip_vpack_merge(place_members, 1, place_barr, p(k_image), p(extra),
                                                                   extra.numel(), st),
        }
        r = timed_events(legs)
        for v in r.values():
            v["gb_per_s"] = round(6 * n / (v["median_ms"] * 1e-3) / 1e9, 1)  # two streams read, one written
        for mine, theirs in (("vpack_split", "diff_encode"), ("vpack_merge", "diff_decode"),
                             ("vpack_merge_in_place", "diff_decode_in_place")):
            r[mine]["of_" + theirs] = round(r[theirs]["median_ms"] / r[mine]["median_ms"], 3)
            r[mine]["spread_of_" + theirs] = [round(r[theirs]["min_ms"] / r[theirs]["median_ms"], 3),
                                              round(r[theirs]["max_ms"] / r[theirs]["median_ms"], 3)]
        for k in legs:
            if k != "copy_1p5":
                r[k]["of_copy_1p5"] = round(r["copy_1p5"]["median_ms"] / r[k]["median_ms"], 3)
        stride = (n + 15) // 16 * 16
        k_place.copy_(base)
        d_place.copy_(base)
        legs["vpack_merge_in_place"]()
        legs["diff_decode_in_place"]()
        torch.cuda.synchronize()
        ok = (torch.equal(k_image[:stride], d_image[stride:]) and torch.equal(k_image[stride:], d_image[:stride])
              and torch.equal(k_back, x) and torch.equal(d_back, x) and torch.equal(k_place, x)
              and torch.equal(d_place, x))  # one member: the diff image, top byte first
        return {"elem_bytes": 2, "n_elems": n, "raw_bytes": 2 * n, "legs": r, "outputs_ok": bool(ok)}

    # ------------------------------------------------------------ (b) the next checkpoint against the previous one
    def checkpoint_masters():
        """tools/pack_bench.py's checkpoint as fp32 masters (bf16 and fp32 members) and int64 tensors."""
        g = torch.Generator().manual_seed(7)
        ms = []
        lo, hi = math.log(256), math.log(1 << 22)
        for u in torch.rand(a.members, generator=g).tolist():
            ms.append(("bf16", torch.randn(int(math.exp(lo + (hi - lo) * u)), device=dev) * 0.02))
        for u in torch.rand(max(a.members // 25, 1), generator=g).tolist():  # fp32: norm weights, scales
            ms.append(("fp32", torch.randn(int(256 * 2 ** (8 * u)), device=dev) * 0.02 + 1.0))
        for u in torch.rand(max(a.members // 50, 1), generator=g).tolist():  # int64: step counters, index tables
            n = int(256 * 2 ** (8 * u))
            ms.append(("int64", torch.cumsum(torch.randint(0, 2000, (n,), device=dev), 0)))
        return ms

    def version(ms, step):
        out = []
        for kind, m in ms:
            if kind == "int64":
                out.append(m + 1 if step else m.clone())
            else:
                v = m + step * torch.randn_like(m) if step else m
                out.append(v.to(torch.bfloat16) if kind == "bf16" else v.clone())
        return out

    def checkpoint(bases, xs, step):
        n = len(xs)
        raw = sum(x.numel() * x.element_size() for x in xs)
        names, barr = codec.pack_bases(xs, bases)
        members = codec.pack_members(xs, names, versioned=True)
        plain = codec.pack_members(xs)
        # ---- buffers of the _into forms
        v_scratch = torch.empty(codec.pack_scratch_bytes(members, n, versioned=True), dtype=u8, device=dev)
        v_buf = torch.empty(codec.pack_bound(members, n, versioned=True), dtype=u8, device=dev)
        k_buf = torch.empty(codec.pack_bound(plain, n), dtype=u8, device=dev)
        v_len, k_len = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        d_scratch = torch.empty(max(codec.diff_scratch_bytes(x.numel(), x.element_size()) for x in xs), dtype=u8,
                                device=dev)
        d_bufs = [torch.empty(codec.diff_bound(x.numel(), x.element_size()), dtype=u8, device=dev) for x in xs]
        d_lens = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = [d_lens[i: i + 1] for i in range(n)]

        def vpack_into():
            codec.compress_pack_into(members, n, v_scratch, v_buf, v_len, res, bases=barr)

        def pack_into():
            codec.compress_pack_into(plain, n, v_scratch, k_buf, k_len, res)

        def loop_into():
            for x, b, o, ln in zip(xs, bases, d_bufs, d_len):
                codec.compress_diff_into(x, b, d_scratch, o, ln, res)

        comp_legs = {"loop_compress_diff_into": loop_into, "compress_pack_into": pack_into,
                     "compress_vpack_into": vpack_into}
        comp_into = timed_wall(comp_legs)
        comp_py = timed_wall({"loop_compress_diff": lambda: [codec.compress_diff(x, b) for x, b in zip(xs, bases)],
                              "compress_pack": lambda: codec.compress_pack(xs),
                              "compress_pack_bases": lambda: codec.compress_pack(xs, bases=bases)})
        counts = {k: launches(fn) for k, fn in comp_legs.items()}
        for fn in comp_legs.values():
            fn()
        torch.cuda.synchronize()
        v_frame, k_frame = v_buf[: int(v_len.item())], k_buf[: int(k_len.item())]
        d_frames = [b[: int(ln)] for b, ln in zip(d_bufs, d_lens.tolist())]
        # ---- decode
        v_head, k_head = codec.pack_info(v_frame), codec.pack_info(k_frame)
        infos = [codec.diff_info(f) for f in d_frames]
        v_outs, k_outs, d_outs = ([torch.empty_like(x) for x in xs] for _ in range(3))
        v_place = [b.clone() for b in bases]  # the in-place leg's state: decoded over and over, checked after a reset
        v_st = torch.zeros(v_head.inner.n_blocks, dtype=torch.int32, device=dev)
        k_st = torch.zeros(k_head.inner.n_blocks, dtype=torch.int32, device=dev)
        d_st = [torch.zeros(inner.n_blocks, dtype=torch.int32, device=dev) for _, inner in infos]

        def unvpack_into():
            codec.decompress_pack_into(v_frame, v_head, v_outs, v_scratch, v_st, res, bases=bases)

        def unvpack_in_place():
            codec.decompress_pack_into(v_frame, v_head, v_place, v_scratch, v_st, res, bases=v_place)

        def unpack_into():
            codec.decompress_pack_into(k_frame, k_head, k_outs, v_scratch, k_st, res)

        def unloop_into():
            for f, (info, inner), b, o, s in zip(d_frames, infos, bases, d_outs, d_st):
                codec.decompress_diff_into(f, info, inner, b, d_scratch, o, s, res)

        dts = [x.dtype for x in xs]
        dec_legs = {"loop_decompress_diff_into": unloop_into, "decompress_pack_into": unpack_into,
                    "decompress_vpack_into": unvpack_into, "decompress_vpack_in_place": unvpack_in_place}
        dec_into = timed_wall(dec_legs)
        dec_py = timed_wall({"loop_decompress_diff": lambda: [codec.decompress_diff(f, b) for f, b in zip(d_frames, bases)],
                             "decompress_pack": lambda: codec.decompress_pack(k_frame, dts),
                             "decompress_pack_bases": lambda: codec.decompress_pack(v_frame, dts, bases=bases)})
        counts.update({k: launches(fn) for k, fn in dec_legs.items() if k != "decompress_vpack_in_place"})
        for o in v_outs + k_outs + d_outs:
            o.zero_()
        for s, b in zip(v_place, bases):
            s.copy_(b)
        oks = {}
        unvpack_into()
        oks["vpack"] = bool(int(res[0]) == 0 and not bool(v_st.any()))
        unvpack_in_place()
        oks["vpack_in_place"] = bool(int(res[0]) == 0 and not bool(v_st.any()))
        unpack_into()
        oks["pack"] = bool(int(res[0]) == 0 and not bool(k_st.any()))
        unloop_into()
        torch.cuda.synchronize()
        same = lambda outs: all(torch.equal(o.view(u8), x.view(u8)) for o, x in zip(outs, xs))  # noqa: E731
        oks["vpack"] = oks["vpack"] and same(v_outs)
        oks["vpack_in_place"] = oks["vpack_in_place"] and same(v_place)
        oks["pack"] = oks["pack"] and same(k_outs)
        oks["loop"] = same(d_outs) and not any(bool(s.any()) for s in d_st)
        loop_bytes = sum(f.numel() for f in d_frames)

        def ratios(t, loop, pack, mine):
            t["vpack_of_loop_time"] = round(t[mine]["median_ms"] / t[loop]["median_ms"], 4)
            t["vpack_of_pack_time"] = round(t[mine]["median_ms"] / t[pack]["median_ms"], 4)
            return t

        return {
            "step": step, "members": n, "raw_bytes": raw,
            "bytes": {"versioned_pack": v_frame.numel(), "pack": k_frame.numel(), "loop_of_diff_frames": loop_bytes,
                      "versioned_pack_of_raw": round(v_frame.numel() / raw, 4),
                      "versioned_pack_of_pack": round(v_frame.numel() / k_frame.numel(), 4),
                      "versioned_pack_of_loop": round(v_frame.numel() / loop_bytes, 4)},
            "compress_into": ratios(comp_into, "loop_compress_diff_into", "compress_pack_into", "compress_vpack_into"),
            "compress_python": ratios(comp_py, "loop_compress_diff", "compress_pack", "compress_pack_bases"),
            "decompress_into": ratios(dec_into, "loop_decompress_diff_into", "decompress_pack_into", "decompress_vpack_into"),
            "decompress_python": ratios(dec_py, "loop_decompress_diff", "decompress_pack", "decompress_pack_bases"),
            "kernel_launches": counts,
            "outputs_ok": oks,
        }

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup}
    if a.gib > 0:
        result["one_large_member"] = one_large_member()
        torch.cuda.empty_cache()
    masters = checkpoint_masters()
    bases = version(masters, 0.0)
    result["checkpoints"] = []
    for step in a.steps:
        result["checkpoints"].append(checkpoint(bases, version(masters, step), step))
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
