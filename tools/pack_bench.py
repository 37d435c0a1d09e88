#!/usr/bin/env python3
"""What the pack frame costs and what it buys (fsehip.h section 2j).  One
process, all legs of a group alternating round by round, medians reported;
every output is checked once after the timing.

(a) one large member: --gib of bf16 bits as ONE member through
    fsehip_pack_split / fsehip_pack_merge, against fsehip_planes_split /
    fsehip_planes_merge of the same tensor and a device-to-device copy of the
    same bytes (HIP events on one stream).

(b) a synthetic checkpoint: --members bf16 tensors of 256 to 2^22 elements
    (log-uniform, randn * 0.02), plus fp32 and int64 tensors, all as plane
    members, through compress_pack / decompress_pack against the loop of
    compress_planes / decompress_planes over the same tensors.  Two forms of
    each: the Python calls as a user writes them (allocation and the
    synchronisation that reads a length included; host wall clock) and the
    _into forms on preallocated buffers (host wall clock from the first call to
    the end of the stream, and the host time until the last call returned).
    Kernel launches are counted once per leg with torch.profiler where that
    works; total bytes are the containers' lengths.

(c) one member out of the pack: a 1 MiB member through
    decompress_pack_members_into against the whole decode.

The loop is the yardstick.  Prints one JSON object and, with --out, writes it
there.  GPU only.
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ckpt", type=int, default=128)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec

    if not torch.cuda.is_available():
        sys.exit("pack_bench needs a GPU")
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
        x = (torch.randn(n, device=dev) * 0.02).to(torch.bfloat16).view(torch.int16)
        members = codec.pack_members([x])
        image_bytes = int(lib.fsehip_pack_image_bytes(members, 1))
        k_image = torch.empty(image_bytes, dtype=u8, device=dev)
        p_image = torch.empty(codec.planes_scratch_bytes(n, 2), dtype=u8, device=dev)
        extra = torch.empty(codec.pack_scratch_bytes(members, 1) - image_bytes, dtype=u8, device=dev)
        k_back, p_back = torch.empty_like(x), torch.empty_like(x)
        back_members = codec.pack_members([k_back])
        flat = torch.empty(2 * n, dtype=u8, device=dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        legs = {
            "copy": lambda: flat.copy_(x.view(u8)),
            "planes_split": lambda: lib.fsehip_planes_split(2, p(x), n, p(p_image), st),
            "pack_split": lambda: lib.fsehip_pack_split(members, 1, p(k_image), p(extra), extra.numel(), st),
            "planes_merge": lambda: lib.fsehip_planes_merge(2, p(p_image), n, p(p_back), st),
            "pack_merge": lambda: lib.fsehip_pack_merge(back_members, 1, p(k_image), p(extra), extra.numel(), st),
        }
        r = timed_events(legs)
        for v in r.values():
            v["gb_per_s"] = round(4 * n / (v["median_ms"] * 1e-3) / 1e9, 1)  # bytes read plus bytes written
        r["pack_split"]["of_planes_split"] = round(r["planes_split"]["median_ms"] / r["pack_split"]["median_ms"], 3)
        r["pack_merge"]["of_planes_merge"] = round(r["planes_merge"]["median_ms"] / r["pack_merge"]["median_ms"], 3)
        for k in ("planes_split", "pack_split", "planes_merge", "pack_merge"):
            r[k]["of_copy"] = round(r["copy"]["median_ms"] / r[k]["median_ms"], 3)
        stride = (n + 15) // 16 * 16
        ok = (torch.equal(k_image[:stride], p_image[stride:]) and torch.equal(k_image[stride:], p_image[:stride])
              and torch.equal(k_back, x) and torch.equal(p_back, x))  # one member: the plane image, top byte first
        return {"elem_bytes": 2, "n_elems": n, "raw_bytes": 2 * n, "legs": r, "outputs_ok": bool(ok)}

    # ------------------------------------------------------------ (b) a synthetic checkpoint
    def checkpoint_tensors():
        g = torch.Generator().manual_seed(7)
        xs = []
        lo, hi = math.log(256), math.log(1 << 22)
        for u in torch.rand(a.members, generator=g).tolist():
            n = int(math.exp(lo + (hi - lo) * u))
            xs.append((torch.randn(n, device=dev) * 0.02).to(torch.bfloat16))
        for u in torch.rand(max(a.members // 25, 1), generator=g).tolist():  # fp32: norm weights, scales
            xs.append(torch.randn(int(256 * 2 ** (8 * u)), device=dev) * 0.02 + 1.0)
        for u in torch.rand(max(a.members // 50, 1), generator=g).tolist():  # int64: step counters, index tables
            n = int(256 * 2 ** (8 * u))
            xs.append(torch.cumsum(torch.randint(0, 2000, (n,), device=dev), 0))
        return xs

    def checkpoint(xs):
        n = len(xs)
        raw = sum(x.numel() * x.element_size() for x in xs)
        members = codec.pack_members(xs)
        # ---- buffers of the _into forms
        k_scratch = torch.empty(codec.pack_scratch_bytes(members, n), dtype=u8, device=dev)
        k_buf = torch.empty(codec.pack_bound(members, n), dtype=u8, device=dev)
        k_len = torch.zeros(1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)
        p_scratch = torch.empty(max(codec.planes_scratch_bytes(x.numel(), x.element_size()) for x in xs), dtype=u8,
                                device=dev)
        p_bufs = [torch.empty(codec.planes_bound(x.numel(), x.element_size()), dtype=u8, device=dev) for x in xs]
        p_lens = torch.zeros(n, dtype=torch.int64, device=dev)
        p_len = [p_lens[i: i + 1] for i in range(n)]

        def pack_into():
            codec.compress_pack_into(members, n, k_scratch, k_buf, k_len, res)

        def loop_into():
            for x, b, ln in zip(xs, p_bufs, p_len):
                codec.compress_planes_into(x, p_scratch, b, ln, res)

        comp_into = timed_wall({"loop_compress_planes_into": loop_into, "compress_pack_into": pack_into})
        comp_py = timed_wall({"loop_compress_planes": lambda: [codec.compress_planes(x) for x in xs],
                              "compress_pack": lambda: codec.compress_pack(xs)})
        counts = {"loop_compress_planes_into": launches(loop_into), "compress_pack_into": launches(pack_into)}
        loop_into()
        pack_into()
        torch.cuda.synchronize()
        k_frame = k_buf[: int(k_len.item())]
        p_frames = [b[: int(ln)] for b, ln in zip(p_bufs, p_lens.tolist())]
        # ---- decode
        head = codec.pack_info(k_frame)
        infos = [codec.planes_info(f) for f in p_frames]
        k_outs = [torch.empty_like(x) for x in xs]
        p_outs = [torch.empty_like(x) for x in xs]
        k_st = torch.zeros(head.inner.n_blocks, dtype=torch.int32, device=dev)
        p_st = [torch.zeros(inner.n_blocks, dtype=torch.int32, device=dev) for _, inner in infos]

        def unpack_into():
            codec.decompress_pack_into(k_frame, head, k_outs, k_scratch, k_st, res)

        def unloop_into():
            for f, (info, inner), o, s in zip(p_frames, infos, p_outs, p_st):
                codec.decompress_planes_into(f, info, inner, p_scratch, o, s, res)

        dts = [x.dtype for x in xs]
        dec_into = timed_wall({"loop_decompress_planes_into": unloop_into, "decompress_pack_into": unpack_into})
        dec_py = timed_wall({"loop_decompress_planes": lambda: [codec.decompress_planes(f, d) for f, d in zip(p_frames, dts)],
                             "decompress_pack": lambda: codec.decompress_pack(k_frame, dts)})
        counts.update({"loop_decompress_planes_into": launches(unloop_into), "decompress_pack_into": launches(unpack_into)})
        for o in k_outs + p_outs:
            o.zero_()
        unpack_into()
        ok_pack = bool(int(res[0]) == 0 and not bool(k_st.any()))
        unloop_into()
        torch.cuda.synchronize()
        ok_pack = ok_pack and all(torch.equal(o.view(u8), x.view(u8)) for o, x in zip(k_outs, xs))
        ok_loop = all(torch.equal(o.view(u8), x.view(u8)) for o, x in zip(p_outs, xs)) and not any(bool(s.any()) for s in p_st)
        # ---- (c) one member out of the pack
        target = 1 << 20
        m = min(range(n), key=lambda i: abs(xs[i].numel() * xs[i].element_size() - target))
        one = torch.empty_like(xs[m])
        m_scratch = torch.empty(codec.pack_members_scratch_bytes(head.members, n, [m]), dtype=u8, device=dev)
        m_st = torch.zeros(1, dtype=torch.int32, device=dev)

        def one_member():
            codec.decompress_pack_members_into(k_frame, head, [m], [one], m_scratch, m_st, res)

        sel = timed_wall({"decompress_pack_into": unpack_into, "one_member_into": one_member})
        one.zero_()
        one_member()
        torch.cuda.synchronize()
        ok_one = bool(torch.equal(one.view(u8), xs[m].view(u8)) and res.tolist() == [0, 0] and m_st.tolist() == [0])
        sep = sum(f.numel() for f in p_frames)

        def ratio(t, loop, pack):
            t["pack_of_loop_time"] = round(t[pack]["median_ms"] / t[loop]["median_ms"], 4)
            return t

        return {
            "members": n, "bf16_members": a.members, "raw_bytes": raw,
            "largest_member_bytes": max(x.numel() * x.element_size() for x in xs),
            "median_member_bytes": int(statistics.median(x.numel() * x.element_size() for x in xs)),
            "bytes": {"separate_plane_frames": sep, "pack": k_frame.numel(), "separate_of_raw": round(sep / raw, 4),
                      "pack_of_raw": round(k_frame.numel() / raw, 4), "pack_of_separate": round(k_frame.numel() / sep, 5)},
            "compress_into": ratio(comp_into, "loop_compress_planes_into", "compress_pack_into"),
            "compress_python": ratio(comp_py, "loop_compress_planes", "compress_pack"),
            "decompress_into": ratio(dec_into, "loop_decompress_planes_into", "decompress_pack_into"),
            "decompress_python": ratio(dec_py, "loop_decompress_planes", "decompress_pack"),
            "kernel_launches": counts,
            "one_member": {"member": m, "member_bytes": xs[m].numel() * xs[m].element_size(), "legs": sel,
                           "of_whole_decode": round(sel["one_member_into"]["median_ms"]
                                                    / sel["decompress_pack_into"]["median_ms"], 5)},
            "outputs_ok": {"pack": ok_pack, "loop": bool(ok_loop), "one_member": ok_one},
        }

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "reps": a.reps, "warmup": a.warmup}
    result["one_large_member"] = one_large_member()
    torch.cuda.empty_cache()
    result["checkpoint"] = checkpoint(checkpoint_tensors())
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
