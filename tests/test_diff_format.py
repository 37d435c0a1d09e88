"""The diff frame's host side (include/fsehip.h section 2h), no GPU: header
write / read, every reject case by name, the bound, scratch and range-scratch
formulas, the container kind and the sealed head of a diff container, and
every argument check the five device calls make before they ask for a device
-- the base pointer's and the three overlap rules included (fake non-null
pointers, never dereferenced, as in tests/test_delta_format.py).  Expected
bytes come from tests/diff_ref.py."""
import ctypes as C

import numpy as np
import pytest

import check_ref as CR
import diff_ref as DF
import frame_ref as R
from entropy_coders_amd import _lib

OK = C.c_void_p(4096)
ODD8 = C.c_void_p(4096 + 8)
ODD4 = C.c_void_p(4096 + 4)
ODD2 = C.c_void_p(4096 + 2)
ODD1 = C.c_void_p(4096 + 1)
BASE = C.c_void_p(1 << 30)  # clear of every other fake pointer
U64_MAX = (1 << 64) - 1
N = 100003


def at(addr):
    return C.c_void_p(addr)


def st(rc):
    return _lib.STATUS[rc]


def read(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    info, inner = _lib.DiffInfo(), _lib.FrameInfo()
    rc = _lib.load().fsehip_diff_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                             C.byref(info), C.byref(inner))
    return rc, info, inner


def head(w=2, n=N, block=4096, version=1, reserved=0, magic=DF.MAGIC, n_total=None, **inner):
    n_total = w * DF.stride_of(n) if n_total is None else n_total
    return DF.header(w, n, version, reserved, magic) + R.header(2, 11, block, 128, n_total, **inner)


# ---------------------------------------------------------------- header
@pytest.mark.parametrize("w", DF.WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, N, 1 << 40])
def test_header_round_trip(w, n):
    lib = _lib.load()
    info = _lib.DiffInfo(1, w, 0, 0, n, 0)
    out = (C.c_uint8 * 16)()
    assert lib.fsehip_diff_write_header(C.byref(info), out) == 0
    assert bytes(out) == DF.header(w, n) and bytes(out)[:4] == b"FSEB"
    rc, got, inner = read(head(w, n, block=65536))
    assert rc == 0
    assert (got.version, got.elem_bytes, got.reserved, got.n_elems, got.stride) == (1, w, 0, n, DF.stride_of(n))
    assert (inner.n_total, inner.block_size, inner.nstates) == (w * DF.stride_of(n), 65536, 2)
    assert inner.n_blocks == (w * DF.stride_of(n) + 65535) // 65536


def test_empty_diff_frame_is_48_bytes():
    for w in DF.WIDTHS:
        e = np.zeros(0, DF.UINT[w])
        buf = DF.build(e, e, 65536, 128, 2)
        assert len(buf) == 48 and read(buf)[0] == 0


def test_the_header_says_what_the_container_does_not_do():
    src = open(_lib.HERE + "/../include/fsehip.h").read()
    assert "#define FSEHIP_KIND_DIFF 4u" in src and "#define FSEHIP_SEALED_DIFF 3u" in src
    assert "THE CONTAINER DOES NOT IDENTIFY THE BASE" in src and "IN-PLACE DECODE" in src


REJECTS = {
    "short-47": head()[:47],
    "short-0": b"",
    "magic-FSEP": head(magic=b"FSEP"),
    "magic-FSED": head(magic=b"FSED"),
    "magic-FSEF": head(magic=b"FSEF"),
    "magic-FSEX": head(magic=b"FSEX"),
    "version-2": head(version=2),
    "version-0": head(version=0),
    "elem_bytes-0": head(w=2)[:5] + b"\x00" + head(w=2)[6:],
    "elem_bytes-3": head(w=2)[:5] + b"\x03" + head(w=2)[6:],
    "elem_bytes-16": head(w=2)[:5] + b"\x10" + head(w=2)[6:],
    "reserved-low": head(reserved=1),
    "reserved-high": head(reserved=0x100),
    "stride-overflows": DF.header(1, U64_MAX - 3) + R.header(2, 11, 65536, 128, 0),
    "image-overflows": DF.header(8, 1 << 62) + R.header(2, 11, 65536, 128, 0),
    "inner-magic-FSEB": head()[:16] + b"FSEB" + head()[20:],
    "inner-magic-FSED": head()[:16] + b"FSED" + head()[20:],
    "inner-version-2": head()[:16] + R.header(2, 11, 4096, 128, 2 * DF.stride_of(N), version=2),
    "inner-n_total-plus-16": head(n_total=2 * DF.stride_of(N) + 16),
    "inner-n_total-minus-16": head(n_total=2 * DF.stride_of(N) - 16),
    "inner-n_total-unpadded": head(n_total=2 * N),
    "inner-n_total-unpadded-width-1": head(w=1, n_total=N),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_header_rejects(name):
    rc, info, inner = read(REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.version, info.elem_bytes, info.n_elems, info.stride, inner.n_total, inner.n_blocks) == (0,) * 6


def test_neither_existing_reader_takes_a_diff_frame():
    lib = _lib.load()
    a = np.arange(1000, dtype=np.int32)
    buf = np.frombuffer(DF.build(a + 1, a, 4096, 128, 2), dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for fn in (lib.fsehip_planes_read_header, lib.fsehip_delta_read_header):
        assert st(fn(p, len(buf), C.byref(_lib.PlanesInfo()), C.byref(_lib.FrameInfo()))) == "BAD_FRAME"
    assert st(lib.fsehip_frame_read_header(p, len(buf), C.byref(_lib.FrameInfo()))) == "BAD_FRAME"
    assert read(buf)[0] == 0


def test_write_header_rejects():
    lib = _lib.load()
    out = (C.c_uint8 * 16)()
    for info in (_lib.DiffInfo(2, 2, 0, 0, 5, 0), _lib.DiffInfo(1, 3, 0, 0, 5, 0), _lib.DiffInfo(1, 0, 0, 0, 5, 0),
                 _lib.DiffInfo(1, 2, 1, 0, 5, 0), _lib.DiffInfo(1, 8, 0, 0, 1 << 62, 0)):
        assert st(lib.fsehip_diff_write_header(C.byref(info), out)) == "BAD_ARG"
    assert st(lib.fsehip_diff_write_header(None, out)) == "BAD_ARG"
    assert st(lib.fsehip_diff_read_header(None, 48, C.byref(_lib.DiffInfo()), C.byref(_lib.FrameInfo()))) == "BAD_ARG"


# ---------------------------------------------------------------- kinds
def test_container_kind_of_a_diff_frame():
    from entropy_coders_amd import container_kind

    lib = _lib.load()
    for magic, want in ((b"FSEB", 4), (b"FSEF", 0), (b"FSEP", 1), (b"FSED", 2), (b"FSEK", 3)):
        a = np.frombuffer(magic, dtype=np.uint8)
        assert lib.fsehip_container_kind(a.ctypes.data_as(C.c_void_p), 4) == want
    for magic in (b"FSEX", b"FSEG", b"FSEb", b"FSE"):
        a = np.frombuffer(magic, dtype=np.uint8)
        assert st(lib.fsehip_container_kind(a.ctypes.data_as(C.c_void_p), len(a))) == "BAD_FRAME"
    assert container_kind(head()) == "diff" and _lib.KIND_DIFF == 4


def test_no_estimate_takes_the_diff_kind():
    lib = _lib.load()
    for kind in (3, 4):
        assert lib.fsehip_estimate_image_bytes(kind, 1000, 2) == 0
        assert st(lib.fsehip_image_histogram(kind, 2, OK, 1000, 65536, OK, None)) == "BAD_ARG"
    for mask in (8, 16):
        assert lib.fsehip_estimate_scratch_bytes(1000, 2, mask, 65536) == 0
        p = C.byref(_lib.FrameParams(65536, 0, 0, 11, 2, 0))
        assert st(lib.fsehip_estimate(p, mask, 2, OK, 1000, OK, 1 << 20, OK, None)) == "BAD_ARG"
    assert _lib.KINDS == ("frame", "planes", "delta")


def sealed_head(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    info, kind, off = _lib.CheckInfo(), C.c_uint32(77), C.c_uint64(77)
    rc = _lib.load().fsehip_sealed_read_header(a.ctypes.data_as(C.c_void_p), len(a), C.byref(info), C.byref(kind),
                                               C.byref(off))
    return rc, info, kind.value, off.value


@pytest.mark.parametrize("w", DF.WIDTHS)
def test_sealed_read_header_on_a_diff_container(w):
    n = 1000
    x = np.arange(n).astype(DF.UINT[w])
    b = (x + 3).astype(DF.UINT[w])
    container = DF.build(x, b, 4096, 128, 2)
    record = CR.record(DF.raw_bytes(x), 8)
    rc, info, kind, off = sealed_head(record + container)
    assert rc == 0 and kind == 3 and _lib.SEALED_KINDS[kind] == "diff"
    assert off == len(record) == 32 + 4 * info.n_cb and info.n_content == n * w  # the content rule of P and D
    assert st(sealed_head(record + container[:47])[0]) == "BAD_FRAME"           # a diff head is 48 bytes
    longer = DF.header(w, n + 1) + container[16:]
    assert st(sealed_head(record + longer)[0]) == "BAD_FRAME"                    # n_elems * w is not n_content
    other = b"FSEX" + container[4:]
    assert st(sealed_head(record + other)[0]) == "BAD_FRAME"


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("w", DF.WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 16, 17, N, 131072])
@pytest.mark.parametrize("block", [4096, 65536])
def test_bound_and_scratch(w, n, block):
    lib = _lib.load()
    assert lib.fsehip_diff_scratch_bytes(n, w) == w * DF.stride_of(n)
    assert lib.fsehip_diff_bound(n, w, block) == DF.bound(n, w, block) == 16 + lib.fsehip_frame_bound(
        w * DF.stride_of(n), block)


def test_bound_and_scratch_reject():
    lib = _lib.load()
    for w in (0, 3, 5, 16):
        assert lib.fsehip_diff_bound(100, w, 65536) == 0 and lib.fsehip_diff_scratch_bytes(100, w) == 0
    assert lib.fsehip_diff_scratch_bytes(U64_MAX - 3, 1) == 0
    assert lib.fsehip_diff_scratch_bytes(1 << 62, 8) == 0
    assert lib.fsehip_diff_bound(1 << 62, 8, 65536) == 0
    assert lib.fsehip_diff_bound((1 << 63) - 16, 2, 16) == 0  # the image fits 64 bits, its frame bound does not
    assert lib.fsehip_diff_bound(0, 1, 0) == 48  # block_size 0 = 65536


def pranges(*r):
    return (_lib.PlanesRange * max(len(r), 1))(*[_lib.PlanesRange(*x) for x in r])


def ranges_scratch(w, ranges):
    """per range roundup16(w * n), the pieces back to back; then roundup16(4 * w * n_ranges)"""
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return sum(r16(w * n) for _, n, _ in ranges) + r16(4 * w * len(ranges))


def test_ranges_scratch_bytes():
    lib = _lib.load()
    f = lib.fsehip_diff_ranges_scratch_bytes
    assert f(2, pranges(), 0) == 0
    assert f(2, pranges((0, 0, 0)), 1) == 16                       # the statuses alone
    assert f(1, pranges((5, 3, 0)), 1) == 16 + 16                  # 3 bytes -> 16
    assert f(2, pranges((4095, 3, 0)), 1) == 16 + 16               # no restart group to decode first
    assert f(8, pranges((3 * 4096 + 7, 1 << 20, 0)), 1) == 8 * (1 << 20) + 32
    for w in DF.WIDTHS:
        rs = [(5, 3, 0), (9000, 100, 3), (4095, 2, 200), (8192, 0, 0), (8191, 0, 0)]
        assert f(w, pranges(*rs), len(rs)) == ranges_scratch(w, rs)
        if w > 1:
            assert f(w, pranges(*rs), len(rs)) == lib.fsehip_planes_ranges_scratch_bytes(w, pranges(*rs), len(rs))
    assert f(3, pranges((0, 1, 0)), 1) == 0
    assert f(8, pranges((0, 1 << 62, 0)), 1) == 0
    assert f(2, None, 1) == 0


# ---------------------------------------------------------------- argument checks before any device use
def fparams(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2, chunk=0):
    return C.byref(_lib.FrameParams(block, table_log, ckpt, mtl, nstates, chunk))


def infos(w=2, n=N, block=4096, n_total=None, n_blocks=None):
    n_total = w * DF.stride_of(n) if n_total is None else n_total
    n_blocks = (n_total + block - 1) // block if n_blocks is None else n_blocks
    return (C.byref(_lib.DiffInfo(1, w, 0, 0, n, DF.stride_of(n))),
            C.byref(_lib.FrameInfo(1, 2, 11, 0, block, 0, n_blocks, 0, n_total, 0)))


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


# fsehip_diff_encode(w, d_src, d_base, n, d_dst, stream)
def en(w=2, src=OK, base=BASE, n=100, dst=OK):
    return lambda lib: lib.fsehip_diff_encode(w, src, base, n, dst, None)


# fsehip_diff_decode(w, d_src, n, d_dst, d_base, stream)
def de(w=2, src=OK, n=100, dst=OK, base=BASE):
    return lambda lib: lib.fsehip_diff_decode(w, src, n, dst, base, None)


for name, f in (("encode", en), ("decode", de)):
    row(f"{name}-width-0", "UNSUPPORTED", f(w=0))
    row(f"{name}-width-3", "UNSUPPORTED", f(w=3))
    row(f"{name}-width-before-null", "UNSUPPORTED", f(w=16, src=None, dst=None, base=None))
    row(f"{name}-image-overflows", "UNSUPPORTED", f(w=8, n=1 << 62))
    row(f"{name}-null-src", "BAD_ARG", f(src=None))
    row(f"{name}-null-dst", "BAD_ARG", f(dst=None))
    row(f"{name}-null-base", "BAD_ARG", f(base=None))
    row(f"{name}-base-odd-address-width-2", "BAD_ARG", f(base=at((1 << 30) + 1)))
    row(f"{name}-base-2-of-4", "BAD_ARG", f(w=4, base=at((1 << 30) + 2)))
    row(f"{name}-base-4-of-8", "BAD_ARG", f(w=8, base=at((1 << 30) + 4)))
    row(f"{name}-empty", "OK", f(w=1, src=None, n=0, dst=None, base=None))
row("encode-image-misaligned", "BAD_ARG", en(w=1, dst=ODD8))
row("encode-src-odd-address-width-2", "BAD_ARG", en(src=ODD1))
row("encode-src-2-of-4", "BAD_ARG", en(w=4, src=ODD2))
row("encode-src-4-of-8", "BAD_ARG", en(w=8, src=ODD4))
row("decode-image-misaligned", "BAD_ARG", de(src=ODD8))
row("decode-dst-misaligned", "BAD_ARG", de(dst=ODD8))
row("decode-dst-misaligned-width-1", "BAD_ARG", de(w=1, dst=ODD1))
# the in-place rule of the bare decode: the base itself, or clear of it
row("decode-dst-overlaps-base-from-below", "BAD_ARG", de(dst=at(1 << 20), base=at((1 << 20) + 16)))
row("decode-dst-overlaps-base-from-above", "BAD_ARG", de(dst=at((1 << 20) + 192), base=at(1 << 20)))
row("decode-dst-overlaps-base-last-byte", "BAD_ARG", de(w=1, n=100, dst=at((1 << 20) + 96), base=at((1 << 20) - 3)))


# fsehip_diff_compress(p, w, d_src, d_base, n, d_scratch, scratch_cap, d_out, out_cap, d_out_len, d_result, stream)
def dc(p=None, w=2, src=OK, base=BASE, n=1000, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20, olen=OK, res=OK):
    p = fparams() if p is None else p
    return lambda lib: lib.fsehip_diff_compress(p, w, src, base, n, scratch, scap, out, ocap, olen, res, None)


row("compress-null-p", "BAD_ARG",
    lambda lib: lib.fsehip_diff_compress(None, 2, OK, BASE, 1000, OK, 1 << 20, OK, 1 << 20, OK, OK, None))
row("compress-null-src", "BAD_ARG", dc(src=None))
row("compress-null-base", "BAD_ARG", dc(base=None))
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
row("compress-base-odd-address", "BAD_ARG", dc(base=at((1 << 30) + 1)))
row("compress-base-2-of-4", "BAD_ARG", dc(w=4, base=at((1 << 30) + 2)))
row("compress-base-4-of-8", "BAD_ARG", dc(w=8, base=at((1 << 30) + 4)))
row("compress-scratch-misaligned", "BAD_ARG", dc(scratch=ODD8))
row("compress-scratch-too-small", "DST_TOO_SMALL", dc(scap=2 * 1008 - 1))
row("compress-scratch-too-small-width-1", "DST_TOO_SMALL", dc(w=1, scap=1007))
row("compress-out-too-small", "DST_TOO_SMALL", dc(ocap=DF.bound(1000, 2, 65536) - 1))
row("compress-misaligned-before-too-small", "BAD_ARG", dc(scratch=ODD8, ocap=0))
row("compress-null-base-before-too-small", "BAD_ARG", dc(base=None, ocap=0))


# fsehip_diff_decompress(info, inner, chunk, d_in, in_len, d_scratch, scratch_cap, d_out, d_base, out_cap,
#                        d_block_status, d_result, stream)
def dd(pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=at(1 << 24), base=BASE, ocap=1 << 20, res=OK):
    info, inner = infos() if pair is None else pair
    return lambda lib: lib.fsehip_diff_decompress(info, inner, 0, d_in, in_len, scratch, scap, out, base, ocap, None,
                                                  res, None)


row("decompress-null-info", "BAD_ARG", dd(pair=(None, infos()[1])))
row("decompress-null-inner", "BAD_ARG", dd(pair=(infos()[0], None)))
row("decompress-null-in", "BAD_ARG", dd(d_in=None))
row("decompress-null-result", "BAD_ARG", dd(res=None))
row("decompress-null-out", "BAD_ARG", dd(out=None))
row("decompress-null-base", "BAD_ARG", dd(base=None))
row("decompress-null-scratch", "BAD_ARG", dd(scratch=None))
row("decompress-in-len-47", "BAD_ARG", dd(in_len=47))
row("decompress-width-3", "BAD_ARG", dd(pair=infos(w=3, n_total=6 * 16)))
row("decompress-inner-n_total-off-by-16", "BAD_ARG", dd(pair=infos(n_total=2 * DF.stride_of(N) + 16)))
row("decompress-inner-n_blocks-wrong", "BAD_ARG", dd(pair=infos(n_blocks=7)))
row("decompress-block-limit", "BAD_ARG", dd(pair=infos(block=1 << 29)))  # the inner header itself is invalid
row("decompress-out-misaligned", "BAD_ARG", dd(out=at((1 << 24) + 8)))
row("decompress-out-misaligned-width-1", "BAD_ARG", dd(pair=infos(w=1), out=at((1 << 24) + 1)))
row("decompress-base-odd-address", "BAD_ARG", dd(base=at((1 << 30) + 1)))
row("decompress-base-4-of-8", "BAD_ARG", dd(pair=infos(w=8), base=at((1 << 30) + 4)))
row("decompress-scratch-misaligned", "BAD_ARG", dd(scratch=ODD8))
row("decompress-scratch-too-small", "DST_TOO_SMALL", dd(scap=2 * DF.stride_of(N) - 1))
row("decompress-out-too-small", "DST_TOO_SMALL", dd(ocap=2 * N - 1))
# the in-place rule: out == base, or no byte shared (N elements of 2 bytes each)
row("decompress-out-overlaps-base-by-16", "BAD_ARG", dd(out=at(1 << 24), base=at((1 << 24) + 16)))
row("decompress-out-overlaps-base-last-element", "BAD_ARG", dd(out=at(1 << 24), base=at((1 << 24) + 2 * N - 2)))
row("decompress-out-overlaps-base-from-above", "BAD_ARG", dd(out=at((1 << 24) + 2 * N - 6), base=at(1 << 24)))
row("decompress-overlap-before-too-small", "BAD_ARG", dd(out=at(1 << 24), base=at((1 << 24) + 16), ocap=0))


# fsehip_diff_decompress_ranges(info, inner, chunk, d_in, in_len, ranges, n_ranges, d_scratch, scratch_cap, d_out,
#                               d_base, out_cap, d_range_status, d_result, stream)
def dr(r=((0, 10, 0),), pair=None, d_in=OK, in_len=1 << 20, scratch=OK, scap=1 << 20, out=at(1 << 24), base=BASE,
       ocap=1 << 20, res=OK, null_ranges=False):
    info, inner = infos() if pair is None else pair
    arr = None if null_ranges else pranges(*r)
    return lambda lib: lib.fsehip_diff_decompress_ranges(info, inner, 0, d_in, in_len, arr, len(r), scratch, scap,
                                                         out, base, ocap, None, res, None)


row("ranges-null-info", "BAD_ARG", dr(pair=(None, infos()[1])))
row("ranges-null-in", "BAD_ARG", dr(d_in=None))
row("ranges-null-result", "BAD_ARG", dr(res=None))
row("ranges-null-ranges", "BAD_ARG", dr(null_ranges=True))
row("ranges-null-out", "BAD_ARG", dr(out=None))
row("ranges-null-base", "BAD_ARG", dr(base=None))
row("ranges-base-odd-address", "BAD_ARG", dr(base=at((1 << 30) + 1)))
row("ranges-null-scratch", "BAD_ARG", dr(scratch=None))
row("ranges-in-len-47", "BAD_ARG", dr(in_len=47))
row("ranges-bad-pair", "BAD_ARG", dr(pair=infos(n_total=2 * DF.stride_of(N) - 16)))
row("ranges-scratch-misaligned", "BAD_ARG", dr(scratch=ODD8))
row("ranges-past-the-end", "BAD_ARG", dr(r=((N - 5, 6, 0),)))
row("ranges-offset-past-the-end", "BAD_ARG", dr(r=((N + 1, 0, 0),)))
row("ranges-source-overflows", "BAD_ARG", dr(r=((U64_MAX, 2, 0),)))
row("ranges-destination-overflows", "BAD_ARG", dr(r=((0, 2, U64_MAX),)))
row("ranges-overlapping-destinations", "BAD_ARG", dr(r=((0, 10, 0), (50, 10, 9))))
row("ranges-overlap-before-too-small", "BAD_ARG", dr(r=((0, 10, 0), (50, 10, 9)), ocap=4))
row("ranges-destination-past-out-cap", "DST_TOO_SMALL", dr(r=((0, 10, 0),), ocap=19))
row("ranges-empty-range-past-out-cap", "DST_TOO_SMALL", dr(r=((0, 0, 11),), ocap=20))
row("ranges-scratch-too-small", "DST_TOO_SMALL", dr(r=((0, 10, 0),), scap=47))
# no overlap of the destinations with the base at all, the base itself included
row("ranges-out-is-the-base", "BAD_ARG", dr(out=BASE))
row("ranges-out-ends-inside-the-base", "BAD_ARG", dr(r=((0, 10, 0),), out=at((1 << 30) - 18)))
row("ranges-out-starts-at-the-last-base-element", "BAD_ARG", dr(r=((0, 10, 0),), out=at((1 << 30) + 2 * N - 2)))
row("ranges-far-destination-reaches-the-base", "BAD_ARG", dr(r=((0, 10, 100),), out=at((1 << 30) - 210)))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_valid_calls_reach_the_device_check():
    """The same calls with valid arguments -- the in-place forms, destinations
    that touch the base's ends without sharing a byte, a source that is the
    base -- reach the device check: NO_DEVICE without a GPU; with one they
    would run on fake pointers, so only then skipped."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    for call in (dr(r=((0, 10, 0), (50, 10, 10), (7, 0, 5))), dr(r=()), dr(r=((4095, 10, 0),), scap=48),
                 dr(r=((0, 10, 0),), out=at((1 << 30) - 20)), dr(r=((0, 10, 0),), out=at((1 << 30) + 2 * N)),
                 dr(r=((0, 0, 0),), out=BASE, base=None),
                 dc(), dc(w=1, src=ODD1, base=at((1 << 30) + 3)), dc(src=BASE),
                 dd(), dd(pair=infos(w=1)), dd(pair=infos(w=8)), dd(out=BASE),
                 dd(out=at(1 << 24), base=at((1 << 24) + 2 * N)), dd(out=at(1 << 24), base=at((1 << 24) - 2 * N)),
                 en(w=1, src=ODD1, base=at((1 << 30) + 7)), en(w=8, src=ODD8), en(src=BASE),
                 de(w=8), de(dst=BASE), de(dst=at(1 << 20), base=at((1 << 20) + 200)),
                 de(dst=at(1 << 20), base=at((1 << 20) - 200))):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from entropy_coders_amd import BlockCodec, FseError, auto_decompress

    with pytest.raises(FseError) as e:
        BlockCodec.diff_info(b"\0" * 48)
    assert e.value.code == "BAD_FRAME"
    a = np.arange(100, dtype=np.uint8)
    buf = DF.build(a, a[::-1], 4096, 128, 2)
    info, inner = BlockCodec.diff_info(buf)
    assert (info.elem_bytes, info.n_elems, info.stride, inner.n_total) == (1, 100, 112, 112)
    with pytest.raises(ValueError, match="base"):
        auto_decompress(buf, np.uint8)
