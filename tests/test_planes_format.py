"""The plane frame's host side (include/fsehip.h section 2d), no GPU: header
write / read, every reject case, the bound and scratch formulas, and every
argument check the device calls make before they ask for a device (fake
non-null pointers, never dereferenced, as in tests/test_abi_args.py).
Expected bytes come from tests/planes_ref.py."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as R
import planes_ref as PR
from entropy_coders_amd import _lib

OK = C.c_void_p(4096)
ODD8 = C.c_void_p(4096 + 8)
ODD2 = C.c_void_p(4096 + 2)
ODD1 = C.c_void_p(4096 + 1)
U64_MAX = (1 << 64) - 1


def st(rc):
    return _lib.STATUS[rc]


def read(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    info, inner = _lib.PlanesInfo(), _lib.FrameInfo()
    rc = _lib.load().fsehip_planes_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                               C.byref(info), C.byref(inner))
    return rc, info, inner


def head(w=2, n=100003, block=4096, version=1, reserved=0, magic=PR.MAGIC, n_total=None, **inner):
    n_total = w * PR.stride_of(n) if n_total is None else n_total
    return PR.header(w, n, version, reserved, magic) + R.header(2, 11, block, 128, n_total, **inner)


# ---------------------------------------------------------------- header
@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 100003, 1 << 40])
def test_header_round_trip(w, n):
    lib = _lib.load()
    info = _lib.PlanesInfo(1, w, 0, 0, n, 0)
    out = (C.c_uint8 * 16)()
    assert lib.fsehip_planes_write_header(C.byref(info), out) == 0
    assert bytes(out) == PR.header(w, n)
    rc, got, inner = read(head(w, n, block=65536))
    assert rc == 0
    assert (got.version, got.elem_bytes, got.reserved, got.n_elems, got.stride) == (1, w, 0, n, PR.stride_of(n))
    assert (inner.n_total, inner.block_size, inner.nstates) == (w * PR.stride_of(n), 65536, 2)
    assert inner.n_blocks == (w * PR.stride_of(n) + 65535) // 65536


def test_empty_plane_frame_is_48_bytes():
    buf = PR.build(np.zeros(0, np.int16), 65536, 128, 2)
    assert len(buf) == 48 and read(buf)[0] == 0


REJECTS = {
    "short-47": head()[:47],
    "short-0": b"",
    "magic": head(magic=b"FSEF"),
    "version-2": head(version=2),
    "elem_bytes-0": head(w=2)[:5] + b"\x00" + head(w=2)[6:],
    "elem_bytes-1": head(w=2)[:5] + b"\x01" + head(w=2)[6:],
    "elem_bytes-3": head(w=2)[:5] + b"\x03" + head(w=2)[6:],
    "elem_bytes-16": head(w=2)[:5] + b"\x10" + head(w=2)[6:],
    "reserved-low": head(reserved=1),
    "reserved-high": head(reserved=0x100),
    "stride-overflows": PR.header(2, U64_MAX - 3) + R.header(2, 11, 65536, 128, 0),
    "image-overflows": PR.header(8, 1 << 62) + R.header(2, 11, 65536, 128, 0),
    "inner-magic": head(magic=PR.MAGIC)[:16] + b"FSEP" + head()[20:],
    "inner-version-2": head(version=1)[:16] + R.header(2, 11, 4096, 128, 2 * PR.stride_of(100003), version=2),
    "inner-n_total-plus-16": head(n_total=2 * PR.stride_of(100003) + 16),
    "inner-n_total-minus-16": head(n_total=2 * PR.stride_of(100003) - 16),
    "inner-n_total-unpadded": head(n_total=2 * 100003),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_header_rejects(name):
    rc, info, inner = read(REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.elem_bytes, info.n_elems, inner.n_total) == (0, 0, 0)  # outputs zeroed


def test_write_header_rejects():
    lib = _lib.load()
    out = (C.c_uint8 * 16)()
    for info in (_lib.PlanesInfo(2, 2, 0, 0, 5, 0), _lib.PlanesInfo(1, 3, 0, 0, 5, 0), _lib.PlanesInfo(1, 2, 1, 0, 5, 0),
                 _lib.PlanesInfo(1, 8, 0, 0, 1 << 62, 0)):
        assert st(lib.fsehip_planes_write_header(C.byref(info), out)) == "BAD_ARG"
    assert st(lib.fsehip_planes_write_header(None, out)) == "BAD_ARG"
    assert st(lib.fsehip_planes_read_header(None, 48, C.byref(_lib.PlanesInfo()), C.byref(_lib.FrameInfo()))) == "BAD_ARG"


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 16, 17, 100003, 131072])
@pytest.mark.parametrize("block", [4096, 65536])
def test_bound_and_scratch(w, n, block):
    lib = _lib.load()
    assert lib.fsehip_planes_scratch_bytes(n, w) == w * PR.stride_of(n)
    assert lib.fsehip_planes_bound(n, w, block) == PR.bound(n, w, block) == 16 + lib.fsehip_frame_bound(
        w * PR.stride_of(n), block)


def test_bound_and_scratch_reject():
    lib = _lib.load()
    for w in (0, 1, 3, 16):
        assert lib.fsehip_planes_bound(100, w, 65536) == 0 and lib.fsehip_planes_scratch_bytes(100, w) == 0
    assert lib.fsehip_planes_scratch_bytes(U64_MAX - 3, 2) == 0
    assert lib.fsehip_planes_scratch_bytes(1 << 62, 8) == 0
    assert lib.fsehip_planes_bound(1 << 62, 8, 65536) == 0
    assert lib.fsehip_planes_bound((1 << 63) - 16, 2, 16) == 0  # the image fits 64 bits, its frame bound does not
    assert lib.fsehip_planes_bound(0, 2, 0) == 48  # block_size 0 = 65536


def pranges(*r):
    return (_lib.PlanesRange * max(len(r), 1))(*[_lib.PlanesRange(*x) for x in r])


def test_ranges_scratch_bytes():
    lib = _lib.load()
    f = lib.fsehip_planes_ranges_scratch_bytes
    assert f(2, pranges(), 0) == 0
    assert f(2, pranges((0, 0, 0)), 1) == 16                       # the statuses alone: 4 * 2, rounded up
    assert f(2, pranges((5, 3, 0)), 1) == 16 + 16                  # 6 bytes -> 16
    assert f(4, pranges((5, 3, 0), (9, 100, 3)), 2) == 16 + 400 + 32
    assert f(8, pranges((0, 1 << 20, 0)), 1) == (8 << 20) + 32
    assert f(3, pranges((0, 1, 0)), 1) == 0
    assert f(8, pranges((0, 1 << 62, 0)), 1) == 0
    assert f(2, None, 1) == 0


# ---------------------------------------------------------------- argument checks before any device use
def fparams(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2, chunk=0):
    return C.byref(_lib.FrameParams(block, table_log, ckpt, mtl, nstates, chunk))


def infos(w=2, n=100003, block=4096, n_total=None, n_blocks=None):
    n_total = w * PR.stride_of(n) if n_total is None else n_total
    n_blocks = (n_total + block - 1) // block if n_blocks is None else n_blocks
    return (C.byref(_lib.PlanesInfo(1, w, 0, 0, n, PR.stride_of(n))),
            C.byref(_lib.FrameInfo(1, 2, 11, 0, block, 0, n_blocks, 0, n_total, 0)))


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


# fsehip_planes_split(w, d_src, n, d_dst, stream) / fsehip_planes_merge(w, d_src, n, d_dst, stream)
for name in ("split", "merge"):
    fn = "fsehip_planes_" + name
    row(f"{name}-width-1", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(1, OK, 100, OK, None))
    row(f"{name}-width-3", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(3, OK, 100, OK, None))
    row(f"{name}-width-before-null", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(16, None, 100, None, None))
    row(f"{name}-image-overflows", "UNSUPPORTED", lambda lib, fn=fn: getattr(lib, fn)(8, OK, 1 << 62, OK, None))
    row(f"{name}-null-src", "BAD_ARG", lambda lib, fn=fn: getattr(lib, fn)(2, None, 100, OK, None))
    row(f"{name}-null-dst", "BAD_ARG", lambda lib, fn=fn: getattr(lib, fn)(2, OK, 100, None, None))
    row(f"{name}-empty", "OK", lambda lib, fn=fn: getattr(lib, fn)(2, None, 0, None, None))
row("split-image-misaligned", "BAD_ARG", lambda lib: lib.fsehip_planes_split(2, OK, 100, ODD8, None))
row("split-src-odd-address", "BAD_ARG", lambda lib: lib.fsehip_planes_split(2, ODD1, 100, OK, None))
row("split-src-2-of-4", "BAD_ARG", lambda lib: lib.fsehip_planes_split(4, ODD2, 100, OK, None))
row("split-src-8-of-16-is-fine-for-8-but-not-4-of-8", "BAD_ARG",
    lambda lib: lib.fsehip_planes_split(8, C.c_void_p(4096 + 4), 100, OK, None))
row("merge-image-misaligned", "BAD_ARG", lambda lib: lib.fsehip_planes_merge(2, ODD8, 100, OK, None))
row("merge-dst-misaligned", "BAD_ARG", lambda lib: lib.fsehip_planes_merge(2, OK, 100, ODD8, None))


# fsehip_planes_compress(p, w, d_src, n, d_scratch, scratch_cap, d_out, out_cap, d_out_len, d_result, stream)
def pc(p=None, w=2, src=OK, n=1000, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, olen=OK, res=OK):
    p = fparams() if p is None else p
    return lambda lib: lib.fsehip_planes_compress(p, w, src, n, scratch, scap, out, ocap, olen, res, None)


row("compress-null-p", "BAD_ARG", lambda lib: lib.fsehip_planes_compress(None, 2, OK, 1000, OK, 1 << 20, OK, 1 << 20, OK, OK, None))
row("compress-null-src", "BAD_ARG", pc(src=None))
row("compress-null-scratch", "BAD_ARG", pc(scratch=None))
row("compress-null-out", "BAD_ARG", pc(out=None))
row("compress-null-out-len", "BAD_ARG", pc(olen=None))
row("compress-null-result", "BAD_ARG", pc(res=None))
row("compress-width-1", "UNSUPPORTED", pc(w=1))
row("compress-width-3", "UNSUPPORTED", pc(w=3))
row("compress-image-overflows", "UNSUPPORTED", pc(w=8, n=1 << 62))
row("compress-block-limit", "UNSUPPORTED", pc(p=fparams(block=1 << 29)))
row("compress-two-blocks-of-1000", "BAD_ARG", pc(p=fparams(block=1000)))
row("compress-nstates-3", "BAD_ARG", pc(p=fparams(nstates=3)))
row("compress-interval-24", "BAD_ARG", pc(p=fparams(ckpt=24)))
row("compress-interval-8-one-state", "BAD_ARG", pc(p=fparams(ckpt=8, nstates=1)))
row("compress-src-odd-address", "BAD_ARG", pc(src=ODD1))
row("compress-src-2-of-4", "BAD_ARG", pc(w=4, src=ODD2))
row("compress-scratch-misaligned", "BAD_ARG", pc(scratch=ODD8))
row("compress-scratch-too-small", "DST_TOO_SMALL", pc(scap=2 * 1008 - 1))
row("compress-out-too-small", "DST_TOO_SMALL", pc(ocap=PR.bound(1000, 2, 65536) - 1))
row("compress-misaligned-before-too-small", "BAD_ARG", pc(scratch=ODD8, ocap=0))


# fsehip_planes_decompress(info, inner, chunk, d_in, in_len, d_scratch, scratch_cap, d_out, out_cap, d_block_status,
#                          d_result, stream)
def pd(pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, res=OK):
    info, inner = infos() if pair is None else pair
    return lambda lib: lib.fsehip_planes_decompress(info, inner, 0, d_in, in_len, scratch, scap, out, ocap, None, res,
                                                    None)


row("decompress-null-info", "BAD_ARG", pd(pair=(None, infos()[1])))
row("decompress-null-inner", "BAD_ARG", pd(pair=(infos()[0], None)))
row("decompress-null-in", "BAD_ARG", pd(d_in=None))
row("decompress-null-result", "BAD_ARG", pd(res=None))
row("decompress-null-out", "BAD_ARG", pd(out=None))
row("decompress-null-scratch", "BAD_ARG", pd(scratch=None))
row("decompress-in-len-47", "BAD_ARG", pd(in_len=47))
row("decompress-width-3", "BAD_ARG", pd(pair=infos(w=3, n_total=6 * 16)))
row("decompress-inner-n_total-off-by-16", "BAD_ARG", pd(pair=infos(n_total=2 * PR.stride_of(100003) + 16)))
row("decompress-inner-n_blocks-wrong", "BAD_ARG", pd(pair=infos(n_blocks=7)))
row("decompress-block-limit", "BAD_ARG", pd(pair=infos(block=1 << 29)))  # the inner header itself is invalid
row("decompress-out-misaligned", "BAD_ARG", pd(out=ODD8))
row("decompress-scratch-misaligned", "BAD_ARG", pd(scratch=ODD8))
row("decompress-scratch-too-small", "DST_TOO_SMALL", pd(scap=2 * PR.stride_of(100003) - 1))
row("decompress-out-too-small", "DST_TOO_SMALL", pd(ocap=2 * 100003 - 1))


# fsehip_planes_decompress_ranges(info, inner, chunk, d_in, in_len, ranges, n_ranges, d_scratch, scratch_cap, d_out,
#                                 out_cap, d_range_status, d_result, stream)
def pr(r=((0, 10, 0),), pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, res=OK,
       null_ranges=False):
    info, inner = infos() if pair is None else pair
    arr = None if null_ranges else pranges(*r)
    return lambda lib: lib.fsehip_planes_decompress_ranges(info, inner, 0, d_in, in_len, arr, len(r), scratch, scap,
                                                           out, ocap, None, res, None)


N = 100003
row("ranges-null-info", "BAD_ARG", pr(pair=(None, infos()[1])))
row("ranges-null-in", "BAD_ARG", pr(d_in=None))
row("ranges-null-result", "BAD_ARG", pr(res=None))
row("ranges-null-ranges", "BAD_ARG", pr(null_ranges=True))
row("ranges-null-out", "BAD_ARG", pr(out=None))
row("ranges-null-scratch", "BAD_ARG", pr(scratch=None))
row("ranges-in-len-47", "BAD_ARG", pr(in_len=47))
row("ranges-bad-pair", "BAD_ARG", pr(pair=infos(n_total=2 * PR.stride_of(N) - 16)))
row("ranges-scratch-misaligned", "BAD_ARG", pr(scratch=ODD8))
row("ranges-past-the-end", "BAD_ARG", pr(r=((N - 5, 6, 0),)))
row("ranges-offset-past-the-end", "BAD_ARG", pr(r=((N + 1, 0, 0),)))
row("ranges-source-overflows", "BAD_ARG", pr(r=((U64_MAX, 2, 0),)))
row("ranges-destination-overflows", "BAD_ARG", pr(r=((0, 2, U64_MAX),)))
row("ranges-overlapping-destinations", "BAD_ARG", pr(r=((0, 10, 0), (50, 10, 9))))
row("ranges-overlap-out-of-order", "BAD_ARG", pr(r=((0, 10, 20), (50, 10, 0), (70, 5, 24))))
row("ranges-overlap-before-too-small", "BAD_ARG", pr(r=((0, 10, 0), (50, 10, 9)), ocap=4))
row("ranges-destination-past-out-cap", "DST_TOO_SMALL", pr(r=((0, 10, 0),), ocap=19))
row("ranges-empty-range-past-out-cap", "DST_TOO_SMALL", pr(r=((0, 0, 11),), ocap=20))
row("ranges-scratch-too-small", "DST_TOO_SMALL", pr(r=((0, 10, 0),), scap=47))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_adjacent_and_empty_ranges_pass_the_checks():
    """The same calls with valid lists reach the device check: NO_DEVICE
    without a GPU; with one they would run on fake pointers, so only then
    skipped."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    for call in (pr(r=((0, 10, 0), (50, 10, 10), (7, 0, 5))), pr(r=()), pc(), pd(),
                 lambda lib: lib.fsehip_planes_split(2, OK, 100, OK, None),
                 lambda lib: lib.fsehip_planes_merge(8, OK, 100, OK, None)):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from entropy_coders_amd import BlockCodec, FseError

    with pytest.raises(FseError) as e:
        BlockCodec.planes_info(b"\0" * 48)
    assert e.value.code == "BAD_FRAME"
    info, inner = BlockCodec.planes_info(PR.build(np.arange(100, dtype=np.int32), 4096, 128, 2))
    assert (info.elem_bytes, info.n_elems, info.stride, inner.n_total) == (4, 100, 112, 448)
