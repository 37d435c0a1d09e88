"""Batch against loop for compression (diagnostics): N host buffers compressed
by fse_compress2_many (one call, host buffers in and out), by a loop of
fse_compress2 calls, and by the C restatement of the crate on one host core.
64 KiB and 4 KiB C2 buffers; median of repeated calls after warm-up, the
argument arrays and the output buffer built once (the C call is what is
timed).  "batch(1)" forces one buffer through the batch path (a second, empty
buffer is answered on the host) to place the crossover to the single call.

    python tools/many_compress.py [--reps R] [SIZE:N ...]
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from entropy_coders_amd import load  # noqa: E402
from oracle import oracle as O  # noqa: E402


def med(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    args = sys.argv[1:]
    reps = 9
    if args[:1] == ["--reps"]:
        reps = int(args[1])
        args = args[2:]
    cases = [tuple(int(x) for x in a.split(":")) for a in args] or (
        [(65536, n) for n in (1, 2, 3, 16, 256, 1000, 4000)] + [(4096, 1000), (4096, 16000)])
    lib = load()
    olib = O.lib()
    pool = {sz: [O.generate(0, 0.155, 0x5EED0002, i, sz) for i in range(256)] for sz in sorted({c[0] for c in cases})}
    print("size      N   many ms  (min..max)        us/stream  GiB/s |  loop ms  us/call | one core ms  us/stream")
    for size, n in cases:
        bufs = [pool[size][i % 256] for i in range(n)]
        stride = int(lib.fsehip_stream_out_bytes(size, 11))
        ptrs = np.array([b.ctypes.data for b in bufs] + [0], dtype=np.uintp)
        lens = np.array([size] * n + [0], dtype=np.uintp)
        dst = np.empty((n + 1) * stride, dtype=np.uint8)
        out_lens = np.zeros(n + 1, dtype=np.uintp)
        bits = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(n + 1, dtype=np.int32)

        def many(k=n):
            rc = lib.fse_compress2_many(p(ptrs), p(lens), k, p(dst), stride, p(out_lens), p(bits), p(st))
            assert rc == 0 and not st[:n].any()

        many()
        want = O.compress2(bufs[n - 1])
        assert dst[(n - 1) * stride: (n - 1) * stride + int(out_lens[n - 1])].tobytes() == want[0]
        t_many = med(many, reps)
        t_b1 = med(lambda: many(2), reps) if n == 1 else None  # one buffer + one empty: the batch path
        one_len, one_bits = C.c_size_t(0), C.c_uint64(0)

        def loop():
            for i in range(n):
                one_len.value = 0
                rc = lib.fse_compress2(C.c_void_p(int(ptrs[i])), size, p(dst), stride, C.byref(one_len),
                                       C.byref(one_bits))
                assert rc == 0

        t_loop = med(loop, max(3, reps // 3) if n >= 1000 else reps)
        cap = O.compress_bound(size)
        odst = np.zeros(cap, dtype=np.uint8)

        def core():
            for i in range(n):
                olib.fo_compress2(C.c_void_p(int(ptrs[i])), size, p(odst), cap, C.byref(one_len), C.byref(one_bits))

        t_core = med(core, 3, warm=1)
        print(f"{size:6d} {n:6d} {t_many[0] * 1e3:9.3f}  ({t_many[1] * 1e3:.3f}..{t_many[2] * 1e3:.3f})"
              f" {t_many[0] / n * 1e6:10.2f} {n * size / t_many[0] / 2**30:6.2f} |"
              f" {t_loop[0] * 1e3:9.3f} {t_loop[0] / n * 1e6:8.2f} |"
              f" {t_core[0] * 1e3:9.3f} {t_core[0] / n * 1e6:8.2f}"
              + (f" | batch(1) {t_b1[0] * 1e3:.3f} ms" if t_b1 else ""), flush=True)


if __name__ == "__main__":
    main()
