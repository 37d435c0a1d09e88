"""The delta frame's host side (include/fsehip.h section 2e), no GPU: header
write / read, every reject case, the bound, scratch and range-scratch formulas,
and every argument check the five device calls make before they ask for a
device (fake non-null pointers, never dereferenced, as in
tests/test_planes_format.py).  Expected bytes come from tests/delta_ref.py."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import frame_ref as R
from entropy_coders_amd import _lib

OK = C.c_void_p(4096)
ODD8 = C.c_void_p(4096 + 8)
ODD4 = C.c_void_p(4096 + 4)
ODD2 = C.c_void_p(4096 + 2)
ODD1 = C.c_void_p(4096 + 1)
U64_MAX = (1 << 64) - 1
N = 100003


def st(rc):
    return _lib.STATUS[rc]


def read(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    info, inner = _lib.DeltaInfo(), _lib.FrameInfo()
    rc = _lib.load().fsehip_delta_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                              C.byref(info), C.byref(inner))
    return rc, info, inner


def head(w=2, n=N, block=4096, version=1, reserved=0, magic=DR.MAGIC, n_total=None, **inner):
    n_total = w * DR.stride_of(n) if n_total is None else n_total
    return DR.header(w, n, version, reserved, magic) + R.header(2, 11, block, 128, n_total, **inner)


# ---------------------------------------------------------------- header
@pytest.mark.parametrize("w", DR.WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, N, 1 << 40])
def test_header_round_trip(w, n):
    lib = _lib.load()
    info = _lib.DeltaInfo(1, w, 0, 0, n, 0)
    out = (C.c_uint8 * 16)()
    assert lib.fsehip_delta_write_header(C.byref(info), out) == 0
    assert bytes(out) == DR.header(w, n)
    rc, got, inner = read(head(w, n, block=65536))
    assert rc == 0
    assert (got.version, got.elem_bytes, got.reserved, got.n_elems, got.stride) == (1, w, 0, n, DR.stride_of(n))
    assert (inner.n_total, inner.block_size, inner.nstates) == (w * DR.stride_of(n), 65536, 2)
    assert inner.n_blocks == (w * DR.stride_of(n) + 65535) // 65536


def test_empty_delta_frame_is_48_bytes():
    for w in DR.WIDTHS:
        buf = DR.build(np.zeros(0, DR.UINT[w]), 65536, 128, 2)
        assert len(buf) == 48 and read(buf)[0] == 0


def test_restart_constant():
    assert _lib.DELTA_RESTART == DR.RESTART == 4096
    src = open(_lib.HERE + "/../include/fsehip.h").read()
    assert "#define FSEHIP_DELTA_RESTART 4096u" in src


REJECTS = {
    "short-47": head()[:47],
    "short-0": b"",
    "magic-FSEP": head(magic=b"FSEP"),
    "magic-FSEF": head(magic=b"FSEF"),
    "version-2": head(version=2),
    "elem_bytes-0": head(w=2)[:5] + b"\x00" + head(w=2)[6:],
    "elem_bytes-3": head(w=2)[:5] + b"\x03" + head(w=2)[6:],
    "elem_bytes-16": head(w=2)[:5] + b"\x10" + head(w=2)[6:],
    "reserved-low": head(reserved=1),
    "reserved-high": head(reserved=0x100),
    "stride-overflows": DR.header(1, U64_MAX - 3) + R.header(2, 11, 65536, 128, 0),
    "image-overflows": DR.header(8, 1 << 62) + R.header(2, 11, 65536, 128, 0),
    "inner-magic": head()[:16] + b"FSED" + head()[20:],
    "inner-version-2": head()[:16] + R.header(2, 11, 4096, 128, 2 * DR.stride_of(N), version=2),
    "inner-n_total-plus-16": head(n_total=2 * DR.stride_of(N) + 16),
    "inner-n_total-minus-16": head(n_total=2 * DR.stride_of(N) - 16),
    "inner-n_total-unpadded": head(n_total=2 * N),
    "inner-n_total-unpadded-width-1": head(w=1, n_total=N),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_header_rejects(name):
    rc, info, inner = read(REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.version, info.elem_bytes, info.n_elems, info.stride, inner.n_total, inner.n_blocks) == (0,) * 6


def test_a_plane_frame_is_no_delta_frame_and_back():
    import planes_ref as PR

    a = np.arange(1000, dtype=np.int32)
    assert st(read(PR.build(a, 4096, 128, 2))[0]) == "BAD_FRAME"
    info, inner = _lib.PlanesInfo(), _lib.FrameInfo()
    buf = np.frombuffer(DR.build(a, 4096, 128, 2), dtype=np.uint8)
    rc = _lib.load().fsehip_planes_read_header(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(info), C.byref(inner))
    assert st(rc) == "BAD_FRAME"


def test_write_header_rejects():
    lib = _lib.load()
    out = (C.c_uint8 * 16)()
    for info in (_lib.DeltaInfo(2, 2, 0, 0, 5, 0), _lib.DeltaInfo(1, 3, 0, 0, 5, 0), _lib.DeltaInfo(1, 0, 0, 0, 5, 0),
                 _lib.DeltaInfo(1, 2, 1, 0, 5, 0), _lib.DeltaInfo(1, 8, 0, 0, 1 << 62, 0)):
        assert st(lib.fsehip_delta_write_header(C.byref(info), out)) == "BAD_ARG"
    assert st(lib.fsehip_delta_write_header(None, out)) == "BAD_ARG"
    assert st(lib.fsehip_delta_read_header(None, 48, C.byref(_lib.DeltaInfo()), C.byref(_lib.FrameInfo()))) == "BAD_ARG"


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("w", DR.WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 16, 17, N, 131072])
@pytest.mark.parametrize("block", [4096, 65536])
def test_bound_and_scratch(w, n, block):
    lib = _lib.load()
    assert lib.fsehip_delta_scratch_bytes(n, w) == w * DR.stride_of(n)
    assert lib.fsehip_delta_bound(n, w, block) == DR.bound(n, w, block) == 16 + lib.fsehip_frame_bound(
        w * DR.stride_of(n), block)


def test_bound_and_scratch_reject():
    lib = _lib.load()
    for w in (0, 3, 5, 16):
        assert lib.fsehip_delta_bound(100, w, 65536) == 0 and lib.fsehip_delta_scratch_bytes(100, w) == 0
    assert lib.fsehip_delta_scratch_bytes(U64_MAX - 3, 1) == 0
    assert lib.fsehip_delta_scratch_bytes(1 << 62, 8) == 0
    assert lib.fsehip_delta_bound(1 << 62, 8, 65536) == 0
    assert lib.fsehip_delta_bound((1 << 63) - 16, 2, 16) == 0  # the image fits 64 bits, its frame bound does not
    assert lib.fsehip_delta_bound(0, 1, 0) == 48  # block_size 0 = 65536


def pranges(*r):
    return (_lib.PlanesRange * max(len(r), 1))(*[_lib.PlanesRange(*x) for x in r])


def ranges_scratch(w, ranges):
    """per range w * roundup16(elem_off + n - e0), then roundup16(4 * w * n_ranges)"""
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return sum(w * r16(s % 4096 + n) for s, n, _ in ranges) + r16(4 * w * len(ranges))


def test_ranges_scratch_bytes():
    lib = _lib.load()
    f = lib.fsehip_delta_ranges_scratch_bytes
    assert f(2, pranges(), 0) == 0
    assert f(2, pranges((0, 0, 0)), 1) == 16                       # the statuses alone
    assert f(1, pranges((5, 3, 0)), 1) == 16 + 16                  # 5 + 3 bytes -> 16
    assert f(2, pranges((4095, 3, 0)), 1) == 2 * 4112 + 16         # from element 0 on
    assert f(2, pranges((4096, 3, 0)), 1) == 2 * 16 + 16           # from its own restart on
    assert f(8, pranges((3 * 4096 + 7, 1 << 20, 0)), 1) == 8 * ((1 << 20) + 16) + 32
    for w in DR.WIDTHS:
        rs = [(5, 3, 0), (9000, 100, 3), (4095, 2, 200), (8192, 0, 0), (8191, 0, 0)]
        assert f(w, pranges(*rs), len(rs)) == ranges_scratch(w, rs)
    assert f(3, pranges((0, 1, 0)), 1) == 0
    assert f(8, pranges((0, 1 << 62, 0)), 1) == 0
    assert f(1, pranges((4095, U64_MAX - 4000, 0)), 1) == 0
    assert f(2, None, 1) == 0


# ---------------------------------------------------------------- argument checks before any device use
def fparams(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2, chunk=0):
    return C.byref(_lib.FrameParams(block, table_log, ckpt, mtl, nstates, chunk))


def infos(w=2, n=N, block=4096, n_total=None, n_blocks=None):
    n_total = w * DR.stride_of(n) if n_total is None else n_total
    n_blocks = (n_total + block - 1) // block if n_blocks is None else n_blocks
    return (C.byref(_lib.DeltaInfo(1, w, 0, 0, n, DR.stride_of(n))),
            C.byref(_lib.FrameInfo(1, 2, 11, 0, block, 0, n_blocks, 0, n_total, 0)))


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


# fsehip_delta_encode(w, d_src, n, d_dst, stream) / fsehip_delta_decode(w, d_src, n, d_dst, stream)
for name in ("encode", "decode"):
    fn = "fsehip_delta_" + name
    row(f"{name}-width-0", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(0, OK, 100, OK, None))
    row(f"{name}-width-3", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(3, OK, 100, OK, None))
    row(f"{name}-width-before-null", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(16, None, 100, None, None))
    row(f"{name}-image-overflows", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(8, OK, 1 << 62, OK, None))
    row(f"{name}-null-src", "BAD_ARG", lambda lib, fn=fn: getattr(lib, fn)(2, None, 100, OK, None))
    row(f"{name}-null-dst", "BAD_ARG", lambda lib, fn=fn: getattr(lib, fn)(2, OK, 100, None, None))
    row(f"{name}-empty", "OK", lambda lib, fn=fn: getattr(lib, fn)(1, None, 0, None, None))
row("encode-image-misaligned", "BAD_ARG", lambda lib: lib.fsehip_delta_encode(1, OK, 100, ODD8, None))
row("encode-src-odd-address-width-2", "BAD_ARG", lambda lib: lib.fsehip_delta_encode(2, ODD1, 100, OK, None))
row("encode-src-2-of-4", "BAD_ARG", lambda lib: lib.fsehip_delta_encode(4, ODD2, 100, OK, None))
row("encode-src-4-of-8", "BAD_ARG", lambda lib: lib.fsehip_delta_encode(8, ODD4, 100, OK, None))
row("decode-image-misaligned", "BAD_ARG", lambda lib: lib.fsehip_delta_decode(2, ODD8, 100, OK, None))
row("decode-dst-misaligned", "BAD_ARG", lambda lib: lib.fsehip_delta_decode(2, OK, 100, ODD8, None))
row("decode-dst-misaligned-width-1", "BAD_ARG", lambda lib: lib.fsehip_delta_decode(1, OK, 100, ODD1, None))


# fsehip_delta_compress(p, w, d_src, n, d_scratch, scratch_cap, d_out, out_cap, d_out_len, d_result, stream)
def dc(p=None, w=2, src=OK, n=1000, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, olen=OK, res=OK):
    p = fparams() if p is None else p
    return lambda lib: lib.fsehip_delta_compress(p, w, src, n, scratch, scap, out, ocap, olen, res, None)


row("compress-null-p", "BAD_ARG", lambda lib: lib.fsehip_delta_compress(None, 2, OK, 1000, OK, 1 << 20, OK, 1 << 20, OK, OK, None))
row("compress-null-src", "BAD_ARG", dc(src=None))
row("compress-null-scratch", "BAD_ARG", dc(scratch=None))
row("compress-null-out", "BAD_ARG", dc(out=None))
row("compress-null-out-len", "BAD_ARG", dc(olen=None))
row("compress-null-result", "BAD_ARG", dc(res=None))
row("compress-width-0", "UNSUPPORTED", dc(w=0))
row("compress-width-3", "UNSUPPORTED", dc(w=3))
row("compress-image-overflows", "UNSUPPORTED", dc(w=8, n=1 << 62))
row("compress-block-limit", "UNSUPPORTED", dc(p=fparams(block=1 << 29)))
row("compress-two-blocks-of-1000", "BAD_ARG", dc(p=fparams(block=1000)))
row("compress-nstates-3", "BAD_ARG", dc(p=fparams(nstates=3)))
row("compress-interval-24", "BAD_ARG", dc(p=fparams(ckpt=24)))
row("compress-interval-8-one-state", "BAD_ARG", dc(p=fparams(ckpt=8, nstates=1)))
row("compress-src-odd-address", "BAD_ARG", dc(src=ODD1))
row("compress-src-2-of-4", "BAD_ARG", dc(w=4, src=ODD2))
row("compress-scratch-misaligned", "BAD_ARG", dc(scratch=ODD8))
row("compress-scratch-too-small", "DST_TOO_SMALL", dc(scap=2 * 1008 - 1))
row("compress-scratch-too-small-width-1", "DST_TOO_SMALL", dc(w=1, scap=1007))
row("compress-out-too-small", "DST_TOO_SMALL", dc(ocap=DR.bound(1000, 2, 65536) - 1))
row("compress-misaligned-before-too-small", "BAD_ARG", dc(scratch=ODD8, ocap=0))


# fsehip_delta_decompress(info, inner, chunk, d_in, in_len, d_scratch, scratch_cap, d_out, out_cap, d_block_status,
#                         d_result, stream)
def dd(pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, res=OK):
    info, inner = infos() if pair is None else pair
    return lambda lib: lib.fsehip_delta_decompress(info, inner, 0, d_in, in_len, scratch, scap, out, ocap, None, res,
                                                   None)


row("decompress-null-info", "BAD_ARG", dd(pair=(None, infos()[1])))
row("decompress-null-inner", "BAD_ARG", dd(pair=(infos()[0], None)))
row("decompress-null-in", "BAD_ARG", dd(d_in=None))
row("decompress-null-result", "BAD_ARG", dd(res=None))
row("decompress-null-out", "BAD_ARG", dd(out=None))
row("decompress-null-scratch", "BAD_ARG", dd(scratch=None))
row("decompress-in-len-47", "BAD_ARG", dd(in_len=47))
row("decompress-width-3", "BAD_ARG", dd(pair=infos(w=3, n_total=6 * 16)))
row("decompress-inner-n_total-off-by-16", "BAD_ARG", dd(pair=infos(n_total=2 * DR.stride_of(N) + 16)))
row("decompress-inner-n_blocks-wrong", "BAD_ARG", dd(pair=infos(n_blocks=7)))
row("decompress-block-limit", "BAD_ARG", dd(pair=infos(block=1 << 29)))  # the inner header itself is invalid
row("decompress-out-misaligned", "BAD_ARG", dd(out=ODD8))
row("decompress-out-misaligned-width-1", "BAD_ARG", dd(pair=infos(w=1), out=ODD1))
row("decompress-scratch-misaligned", "BAD_ARG", dd(scratch=ODD8))
row("decompress-scratch-too-small", "DST_TOO_SMALL", dd(scap=2 * DR.stride_of(N) - 1))
row("decompress-out-too-small", "DST_TOO_SMALL", dd(ocap=2 * N - 1))


# fsehip_delta_decompress_ranges(info, inner, chunk, d_in, in_len, ranges, n_ranges, d_scratch, scratch_cap, d_out,
#                                out_cap, d_range_status, d_result, stream)
def dr(r=((0, 10, 0),), pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, res=OK,
       null_ranges=False):
    info, inner = infos() if pair is None else pair
    arr = None if null_ranges else pranges(*r)
    return lambda lib: lib.fsehip_delta_decompress_ranges(info, inner, 0, d_in, in_len, arr, len(r), scratch, scap,
                                                          out, ocap, None, res, None)


row("ranges-null-info", "BAD_ARG", dr(pair=(None, infos()[1])))
row("ranges-null-in", "BAD_ARG", dr(d_in=None))
row("ranges-null-result", "BAD_ARG", dr(res=None))
row("ranges-null-ranges", "BAD_ARG", dr(null_ranges=True))
row("ranges-null-out", "BAD_ARG", dr(out=None))
row("ranges-null-scratch", "BAD_ARG", dr(scratch=None))
row("ranges-in-len-47", "BAD_ARG", dr(in_len=47))
row("ranges-bad-pair", "BAD_ARG", dr(pair=infos(n_total=2 * DR.stride_of(N) - 16)))
row("ranges-scratch-misaligned", "BAD_ARG", dr(scratch=ODD8))
row("ranges-past-the-end", "BAD_ARG", dr(r=((N - 5, 6, 0),)))
row("ranges-offset-past-the-end", "BAD_ARG", dr(r=((N + 1, 0, 0),)))
row("ranges-source-overflows", "BAD_ARG", dr(r=((U64_MAX, 2, 0),)))
row("ranges-destination-overflows", "BAD_ARG", dr(r=((0, 2, U64_MAX),)))
row("ranges-overlapping-destinations", "BAD_ARG", dr(r=((0, 10, 0), (50, 10, 9))))
row("ranges-overlap-out-of-order", "BAD_ARG", dr(r=((0, 10, 20), (50, 10, 0), (70, 5, 24))))
row("ranges-overlap-before-too-small", "BAD_ARG", dr(r=((0, 10, 0), (50, 10, 9)), ocap=4))
row("ranges-destination-past-out-cap", "DST_TOO_SMALL", dr(r=((0, 10, 0),), ocap=19))
row("ranges-empty-range-past-out-cap", "DST_TOO_SMALL", dr(r=((0, 0, 11),), ocap=20))
row("ranges-scratch-too-small", "DST_TOO_SMALL", dr(r=((0, 10, 0),), scap=47))
row("ranges-scratch-counts-the-restart-group", "DST_TOO_SMALL", dr(r=((4095, 10, 0),), scap=2 * 4112 + 15))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_valid_calls_reach_the_device_check():
    """The same calls with valid arguments reach the device check: NO_DEVICE
    without a GPU; with one they would run on fake pointers, so only then
    skipped."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    for call in (dr(r=((0, 10, 0), (50, 10, 10), (7, 0, 5))), dr(r=()), dr(r=((4095, 10, 0),), scap=2 * 4112 + 16),
                 dc(), dc(w=1, src=ODD1), dd(), dd(pair=infos(w=1)), dd(pair=infos(w=8)),
                 lambda lib: lib.fsehip_delta_encode(1, ODD1, 100, OK, None),
                 lambda lib: lib.fsehip_delta_encode(8, ODD8, 100, OK, None),
                 lambda lib: lib.fsehip_delta_decode(8, OK, 100, OK, None)):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from entropy_coders_amd import BlockCodec, FseError

    with pytest.raises(FseError) as e:
        BlockCodec.delta_info(b"\0" * 48)
    assert e.value.code == "BAD_FRAME"
    info, inner = BlockCodec.delta_info(DR.build(np.arange(100, dtype=np.uint8), 4096, 128, 2))
    assert (info.elem_bytes, info.n_elems, info.stride, inner.n_total) == (1, 100, 112, 112)
