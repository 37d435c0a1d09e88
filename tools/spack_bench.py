#!/usr/bin/env python3
"""What the member check record and the sealed pack cost (fsehip.h section
2l).  One process, the legs of every measurement alternating round by round
(--rounds, after --warmup rounds), medians reported; every output is checked
once after the timing.

(1) the record of a checkpoint: fsehip_mcheck_build over tools/pack_bench.py's
    synthetic checkpoint (--members bf16 tensors of 256 to 2^22 elements, plus
    fp32 and int64 tensors: 1,060 at the default), against the loop of
    fsehip_check_build per tensor and a device-to-device copy of the same
    bytes.  Host wall clock from the first call to the end of the stream, and
    the host time until the last call returned.  Kernel launches are counted
    once per leg with torch.profiler where that works, beside the counts read
    from the code (three per fsehip_mcheck_build, two per fsehip_check_build).

(2) one large member: --gib of bytes as ONE member through fsehip_mcheck_build,
    against fsehip_check_build of the same bytes (HIP events on one stream).
    The threshold set in advance: no more than 1.15 x fsehip_check_build.

(3) the checkpoint update: compress_pack_sealed / decompress_pack_sealed with
    bases= and outs=bases (the _into forms on preallocated buffers), against
    compress_pack(bases=) / decompress_pack unsealed.

Prints one JSON object and, with --out, writes it there.  GPU only.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GATE = 1.15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ckpt", type=int, default=128)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from entropy_coders_amd import BlockCodec

    if not torch.cuda.is_available():
        sys.exit("spack_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    codec = BlockCodec(ckpt_interval=a.ckpt, device=dev)
    lib, st = codec.lib, codec._stream()
    u8 = torch.uint8
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed_events(legs):
        times = {k: [] for k in legs}
        for r in range(a.warmup + a.rounds):
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
        total, enq = {k: [] for k in legs}, {k: [] for k in legs}
        for r in range(a.warmup + a.rounds):
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
        """Kernel launches of one fn(), counted by torch.profiler (as tools/pack_bench.py does); a string where it cannot."""
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
            return n or "unavailable: no kernel event"
        except Exception as e:  # the count is extra: the timings stand without it
            return f"unavailable: {type(e).__name__}"

    def checkpoint_tensors():
        """tools/pack_bench.py's checkpoint, drawn the same way."""
        g = torch.Generator().manual_seed(7)
        xs = []
        lo, hi = math.log(256), math.log(1 << 22)
        for u in torch.rand(a.members, generator=g).tolist():
            xs.append((torch.randn(int(math.exp(lo + (hi - lo) * u)), device=dev) * 0.02).to(torch.bfloat16))
        for u in torch.rand(max(a.members // 25, 1), generator=g).tolist():
            xs.append(torch.randn(int(256 * 2 ** (8 * u)), device=dev) * 0.02 + 1.0)
        for u in torch.rand(max(a.members // 50, 1), generator=g).tolist():
            xs.append(torch.cumsum(torch.randint(0, 2000, (int(256 * 2 ** (8 * u)),), device=dev), 0))
        return xs

    def crc_of(x):
        return zlib.crc32(x.view(u8).cpu().numpy().tobytes()) if x.numel() else 0

    # ------------------------------------------------------------ (1) the record of a checkpoint
    def record_of_checkpoint(xs):
        n = len(xs)
        raw = sum(x.numel() * x.element_size() for x in xs)
        members = codec.pack_members(xs)
        scratch = torch.empty(codec.mcheck_scratch_bytes(members, n), dtype=u8, device=dev)
        record = torch.empty(32 + 8 * n, dtype=u8, device=dev)
        recs = [torch.empty(int(lib.fsehip_check_bytes(x.numel() * x.element_size(), 16)), dtype=u8, device=dev)
                for x in xs]
        copies = [torch.empty_like(x) for x in xs]

        def mcheck():
            rc = lib.fsehip_mcheck_build(members, None, n, p(record), p(scratch), scratch.numel(), st)
            assert rc == 0, rc

        def loop():
            for x, r in zip(xs, recs):
                lib.fsehip_check_build(16, p(x), x.numel() * x.element_size(), p(r), st)

        def copy():
            for x, c in zip(xs, copies):
                c.copy_(x)

        legs = timed_wall({"loop_check_build": loop, "mcheck_build": mcheck, "loop_copy": copy})
        for v in legs.values():
            v["gb_per_s"] = round(raw / (v["median_ms"] * 1e-3) / 1e9, 1)
        mcheck()
        loop()
        torch.cuda.synchronize()
        table = record[32:].cpu().numpy().view("<u4").reshape(n, 2)
        pick = sorted(range(n), key=lambda i: xs[i].numel())[:: max(n // 40, 1)]  # small to large
        ok = all(int(table[i, 0]) == crc_of(xs[i]) for i in pick) and not table[:, 1].any()
        ok = ok and all(int.from_bytes(bytes(recs[i][20:24].cpu().numpy()), "little") == int(table[i, 0]) for i in pick)
        return {"members": n, "raw_bytes": raw, "legs": legs,
                "mcheck_of_loop_time": round(legs["mcheck_build"]["median_ms"] / legs["loop_check_build"]["median_ms"], 4),
                "mcheck_of_copy_time": round(legs["mcheck_build"]["median_ms"] / legs["loop_copy"]["median_ms"], 4),
                "kernel_launches_counted": {"mcheck_build": launches(mcheck), "loop_check_build": launches(loop)},
                "kernel_launches_by_the_code": {"mcheck_build": 3, "loop_check_build": 2 * n}, "outputs_ok": bool(ok)}

    # ------------------------------------------------------------ (2) one large member
    def one_large_member():
        n = int(a.gib * (1 << 30)) // 256 * 256
        x = torch.randint(0, 256, (n,), dtype=u8, device=dev)
        members = codec.pack_members([x])
        scratch = torch.empty(codec.mcheck_scratch_bytes(members, 1), dtype=u8, device=dev)
        record = torch.empty(40, dtype=u8, device=dev)
        rec = torch.empty(int(lib.fsehip_check_bytes(n, 16)), dtype=u8, device=dev)
        legs = timed_events({
            "check_build": lambda: lib.fsehip_check_build(16, p(x), n, p(rec), st),
            "mcheck_build": lambda: lib.fsehip_mcheck_build(members, None, 1, p(record), p(scratch), scratch.numel(), st),
        })
        for v in legs.values():
            v["gb_per_s"] = round(n / (v["median_ms"] * 1e-3) / 1e9, 1)
        torch.cuda.synchronize()
        want = crc_of(x)
        got = int.from_bytes(bytes(record[32:36].cpu().numpy()), "little")
        got_k = int.from_bytes(bytes(rec[20:24].cpu().numpy()), "little")
        ratio = legs["mcheck_build"]["median_ms"] / legs["check_build"]["median_ms"]
        return {"bytes": n, "legs": legs, "mcheck_of_check_build_time": round(ratio, 4), "gate": GATE,
                "gate_met": bool(ratio <= GATE), "outputs_ok": bool(got == want and got_k == want)}

    # ------------------------------------------------------------ (3) the checkpoint update
    def checkpoint_update(xs):
        n = len(xs)
        raw = sum(x.numel() * x.element_size() for x in xs)
        ints = [x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]) for x in xs]
        g = torch.Generator(device=dev).manual_seed(3)
        olds = [(x - torch.randint(-2, 3, x.shape, device=dev, generator=g).to(x.dtype)) for x in ints]
        kinds, barr = codec.pack_bases(ints, olds)
        members = codec.pack_members(ints, kinds, versioned=True)
        scratch = torch.empty(codec.pack_sealed_scratch_bytes(members, n, True), dtype=u8, device=dev)
        s_buf = torch.empty(codec.pack_sealed_bound(members, n, True), dtype=u8, device=dev)
        v_buf = torch.empty(codec.pack_bound(members, n, True), dtype=u8, device=dev)
        s_len, v_len = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int32, device=dev)

        comp = timed_wall({
            "compress_pack_into": lambda: codec.compress_pack_into(members, n, scratch, v_buf, v_len, res, bases=barr),
            "compress_pack_sealed_into": lambda: codec.compress_pack_sealed_into(members, n, scratch, s_buf, s_len, res,
                                                                                 bases=barr),
        })
        torch.cuda.synchronize()
        sealed, plain = s_buf[: int(s_len.item())], v_buf[: int(v_len.item())]
        ok = bool(torch.equal(sealed[32 + 8 * n:], plain))
        rec, head = codec.pack_sealed_info(sealed)
        vhead = codec.pack_info(plain)
        bst = torch.zeros(head.inner.n_blocks, dtype=torch.int32, device=dev)
        mc, bc = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        cres = torch.zeros(4, dtype=torch.int32, device=dev)
        work = [o.clone() for o in olds]

        def reset():
            for w, o in zip(work, olds):
                w.copy_(o)

        def unsealed():
            reset()
            codec.decompress_pack_into(plain, vhead, work, scratch, bst, res, bases=work)

        def sealed_decode():
            reset()
            codec.decompress_pack_sealed_into(sealed, rec, head, work, scratch, bst, res, mc, bc, cres, bases=work)

        dec = timed_wall({"reset_only": reset, "decompress_pack_into": unsealed,
                          "decompress_pack_sealed_into": sealed_decode})
        sealed_decode()
        torch.cuda.synchronize()
        ok = ok and cres.tolist() == [0, 0, 0, 0] and all(torch.equal(w, x) for w, x in zip(work, ints))
        # a wrong old checkpoint: refused, untouched
        reset()
        work[n // 2][0] ^= 1
        before = work[n // 2].clone()
        codec.decompress_pack_sealed_into(sealed, rec, head, work, scratch, bst, res, mc, bc, cres, bases=work)
        torch.cuda.synchronize()
        ok = ok and cres.tolist()[2] == 1 and int(bc[n // 2]) == -21 and torch.equal(work[n // 2], before) \
            and torch.equal(work[0], olds[0])

        def net(k):
            return round(dec[k]["median_ms"] - dec["reset_only"]["median_ms"], 4)

        return {"members": n, "raw_bytes": raw, "bytes": {"vpack": plain.numel(), "sealed": sealed.numel(),
                                                          "record": 32 + 8 * n},
                "compress": comp, "decompress_in_place": dec,
                "sealed_of_unsealed_compress_time": round(comp["compress_pack_sealed_into"]["median_ms"]
                                                          / comp["compress_pack_into"]["median_ms"], 4),
                "decompress_net_of_reset_ms": {"unsealed": net("decompress_pack_into"),
                                               "sealed": net("decompress_pack_sealed_into")},
                "sealed_of_unsealed_decompress_time": round(net("decompress_pack_sealed_into")
                                                            / net("decompress_pack_into"), 4),
                "outputs_ok": bool(ok)}

    torch.manual_seed(1)
    result = {"device": torch.cuda.get_device_name(dev), "block_size": codec.block_size, "ckpt_interval": a.ckpt,
              "rounds": a.rounds, "warmup": a.warmup}
    result["one_large_member"] = one_large_member()
    torch.cuda.empty_cache()
    xs = checkpoint_tensors()
    result["record_of_checkpoint"] = record_of_checkpoint(xs)
    result["checkpoint_update"] = checkpoint_update(xs)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
