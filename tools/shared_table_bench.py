"""Shared-table coding against own-table streams on many small messages
(diagnostics): N messages of 512 B and of 2 KiB from the bench generator (LUT
p = 0.155 and 0.05), all on the device.

  shared  fsehip_compress_shared / fsehip_decompress_shared (known lengths)
          against one table trained on a separate 64 KiB sample (counts + 1 on
          all 256 symbols, normalised at L = 11)
  own     fsehip_compress_streams / fsehip_decompress_streams: each message
          its own table and header (the routes small records had before)

HIP-event times (median of --reps calls after warm-up), total compressed bytes
each way, both decodes compared with the source.  One JSON document to
profiles/shared_table/ and a table to stdout.

    python tools/shared_table_bench.py [--msgs N] [--reps R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from entropy_coders_amd import SharedTable, load  # noqa: E402
from entropy_coders_amd._lib import StreamDesc  # noqa: E402

TABLE_LOG, SAMPLE = 11, 65536


def ptr(t):
    return C.c_void_p(t.data_ptr())


def event_ms(torch, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t), min(t), max(t)


def descs(torch, rows):
    a = (StreamDesc * len(rows))(*[StreamDesc(*r) for r in rows])
    return torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()


def case(torch, lib, size, prob, n, reps):
    hs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    sample = torch.empty(SAMPLE, dtype=torch.uint8, device="cuda")
    assert lib.fsehip_generate(0, prob, 0x5EED0C00, size, ptr(src), n * size, hs) == 0      # block i = message i
    assert lib.fsehip_generate(0, prob, 0x5EED0C01, SAMPLE, ptr(sample), SAMPLE, hs) == 0   # another seed
    table = SharedTable.train([sample.cpu().numpy()], TABLE_LOG, 1)
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    ok = lambda st: not bool(st.any())  # noqa: E731
    row = {"message_bytes": size, "prob": prob, "messages": n, "raw_bytes": n * size}

    # shared table
    cap = int(lib.fsehip_shared_out_bytes(size, TABLE_LOG))
    enc = descs(torch, [(i * size, i * cap, size, cap) for i in range(n)])
    out, clen, bits, st = torch.empty(n * cap, dtype=torch.uint8, device="cuda"), i32(), i32(), i32()
    comp = lambda: lib.fsehip_compress_shared(2, ptr(table.image), ptr(src), ptr(enc), n, ptr(out), ptr(clen),  # noqa: E731
                                              ptr(bits), ptr(st), hs)
    assert comp() == 0
    row["shared_compress_ms"] = event_ms(torch, comp, reps)
    assert ok(st)
    lens = clen.cpu().numpy()
    row["shared_bytes"] = int(lens.sum())
    dec = descs(torch, [(i * cap, i * size, int(lens[i]), size) for i in range(n)])
    raw_len = torch.full((n,), size, dtype=torch.int32, device="cuda")
    back, olen, dst = torch.empty(n * size, dtype=torch.uint8, device="cuda"), i32(), i32()
    decomp = lambda: lib.fsehip_decompress_shared(2, ptr(table.image), ptr(out), ptr(dec), n, ptr(back), ptr(raw_len),  # noqa: E731
                                                  ptr(olen), ptr(dst), hs)
    assert decomp() == 0
    row["shared_decompress_ms"] = event_ms(torch, decomp, reps)
    assert ok(dst) and torch.equal(back, src), "shared-table round trip"

    # own tables: one stream per message
    stride = (int(lib.fsehip_stream_out_bytes(size, 11)) + 255) // 256 * 256
    enc = descs(torch, [(i * size, i * stride, size, stride) for i in range(n)])
    out2 = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    comp = lambda: lib.fsehip_compress_streams(2, 0, 11, ptr(src), ptr(enc), n, ptr(out2), ptr(clen), ptr(bits),  # noqa: E731
                                               ptr(st), hs)
    assert comp() == 0
    row["own_compress_ms"] = event_ms(torch, comp, reps)
    assert ok(st)
    row["own_bytes"] = int(clen.cpu().numpy().sum())
    back.zero_()
    decomp = lambda: lib.fsehip_decompress_streams(2, 11, ptr(out2), stride, ptr(clen), n, ptr(back), size, ptr(olen),  # noqa: E731
                                                   ptr(dst), hs)
    assert decomp() == 0
    row["own_decompress_ms"] = event_ms(torch, decomp, reps)
    assert ok(dst) and torch.equal(back, src), "own-table round trip"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_table", "shared_table_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("shared_table_bench: no GPU (there is no CPU path to time)")
    lib = load()
    rows = [case(torch, lib, size, prob, a.msgs, a.reps) for size in (512, 2048) for prob in (0.155, 0.05)]
    doc = {"tool": "tools/shared_table_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "times": "HIP events, ms: median, min, max", "table_log": TABLE_LOG, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("bytes    p    messages | shared: compress ms  decompress ms  bytes | own: compress ms  decompress ms  bytes")
    for r in rows:
        print(f"{r['message_bytes']:5d} {r['prob']:5.3f} {r['messages']:8d} | {r['shared_compress_ms'][0]:9.3f} "
              f"{r['shared_decompress_ms'][0]:9.3f} {r['shared_bytes']:12d} | {r['own_compress_ms'][0]:9.3f} "
              f"{r['own_decompress_ms'][0]:9.3f} {r['own_bytes']:12d}", flush=True)


if __name__ == "__main__":
    main()
