"""A fixed mix of C ABI calls (host calls, _many, building blocks, bit calls, block and frame calls), three
times over, for comparing two builds of the library call for call:
    [FSEHIP_LIB=libfsehip_NAME.so] rocprofv3 --hip-runtime-trace --stats --output-format csv -d OUT -- \\
        python tools/capi_call_mix.py
and compare the Calls column of OUT's hip_api_stats.csv (profiles/capi_split/hip_calls/)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import entropy_coders_amd as E
from entropy_coders_amd import fse as F
from oracle import oracle as O

torch.cuda.set_device(0)
src = O.generate(0, 0.155, 0x5EED0002, 0, 65536)
bufs = [O.generate(0, 0.155, 0x5EED0002, i, 3000 + 977 * i) for i in range(40)]
for rep in range(3):
    c2, _ = F.compress2(src); assert F.decompress2(c2) == src.tobytes()
    c1, _ = F.compress(src); assert F.decompress(c1) == src.tobytes()
    cl, _ = F.compress2_log(src, 12); assert F.decompress2(cl) == src.tobytes()
    cl, _ = F.compress2_log(src, 14); assert F.decompress2(cl) == src.tobytes()
    comps = F.compress2_many(bufs)
    streams = [c[0] if isinstance(c, tuple) else c for c in comps]
    outs = F.decompress2_many(streams, 65536)
    assert [bytes(o) for o in outs] == [b.tobytes() for b in bufs]
    F.decompress2_many(streams[:2], 65536)
    h = F.histogram_new(src); nh = F.normalize_optimal(h); F.normalize(h, 9); F.norm_histogram_new(src)
    w, _ = F.norm_histogram_write(nh); F.norm_histogram_read(w); F.encode_table_new(nh); F.decode_table_new(nh)
    F.compress_nh(src)
    bits, nb = F.bitstack_write([1, 2, 3, 4], [3, 4, 5, 6])
    for call in (lambda: F.bitstack_read(bits, [6, 5, 4, 3]), lambda: F.bitstream_read(bits, nb, [3, 4], ops=[0, 1])):
        try:
            call()
        except E.FseError as e:  # a status is as good as a value here: the same HIP calls either way
            print("bit call:", e)
    for ns in (2, 1):
        codec = E.BlockCodec(device="cuda:0", nstates=ns, ckpt_interval=64)
        d = codec.generate(0, 0.155, 7, 40 * 65536 + 777)
        cb = codec.compress(d); out, st = codec.decompress(cb); out2, st2 = codec.decompress(cb, use_sidecar=False)
        assert torch.equal(out, d) and torch.equal(out2, d)
        fr = codec.compress_frame(d, chunk_blocks=16)
        o, s = codec.decompress_frame(fr, chunk_blocks=16); assert torch.equal(o, d)
        views, rs = codec.decompress_frame_ranges(fr, [(100, 5000), (3 * 65536, 6 * 65536), (20 * 65536 + 5, 70000)], chunk_blocks=4)
        host = d.cpu()
        assert torch.equal(views[1].cpu(), host[3 * 65536: 9 * 65536]) and torch.equal(views[2].cpu(), host[20 * 65536 + 5: 20 * 65536 + 5 + 70000])
        torch.cuda.synchronize()
print("hip_calls ok")
