"""The check record's host side (include/fsehip.h section 2f), no GPU: the
CRC-32 and its combine against zlib, header write / read, every reject case,
the sealed head, the range planner against a per-byte model, and every
argument check the device calls make before they ask for a device (fake
non-null pointers, never dereferenced, as in tests/test_planes_format.py).
Expected bytes come from tests/check_ref.py."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import check_ref as K
import delta_ref as DR
import frame_ref as R
import planes_ref as PR
from entropy_coders_amd import _lib

OK = C.c_void_p(4096)
ODD = C.c_void_p(4096 + 3)
U64_MAX = (1 << 64) - 1


def st(rc):
    return _lib.STATUS[rc]


def arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def read(buf):
    a = arr(buf)
    info = _lib.CheckInfo()
    rc = _lib.load().fsehip_check_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), C.byref(info))
    return rc, info


def info_of(n=100003, check_log=12, crc=0x12345678):
    rc, info = read(K.header(check_log, n, K.n_cb_of(n, check_log), crc if n else 0))
    assert rc == 0
    return info


# ---------------------------------------------------------------- CRC-32
def test_crc32_and_combine_equal_zlib():
    lib = _lib.load()
    rng = np.random.default_rng(0xC3C)
    assert lib.fsehip_crc32(0, None, 0) == 0
    for _ in range(300):
        la, lb = (int(x) for x in rng.choice([0, 1, 2, 3, 15, 16, 17, 255, 256, 1000, 70001], 2))
        a, b = rng.integers(0, 256, la, dtype=np.uint8), rng.integers(0, 256, lb, dtype=np.uint8)
        pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
        ca, cb = zlib.crc32(a.tobytes()), zlib.crc32(b.tobytes())
        assert lib.fsehip_crc32(0, pa, la) == ca
        assert lib.fsehip_crc32(ca, pb, lb) == zlib.crc32(b.tobytes(), ca) == zlib.crc32(a.tobytes() + b.tobytes())
        assert lib.fsehip_crc32_combine(ca, cb, lb) == zlib.crc32(a.tobytes() + b.tobytes())
    assert lib.fsehip_crc32_combine(0xDEADBEEF, 0, 0) == 0xDEADBEEF
    big = 5 << 32  # a length above 32 bits: against the reference's written-out combine
    assert lib.fsehip_crc32_combine(0x12345678, 0x9ABCDEF0, big) == K.combine(0x12345678, 0x9ABCDEF0, big)


def test_python_crc32():
    from entropy_coders_amd import crc32, crc32_combine

    assert crc32(b"") == 0 and crc32(b"123456789") == 0xCBF43926
    assert crc32(b"6789", crc32(b"12345")) == 0xCBF43926
    assert crc32_combine(crc32(b"12345"), crc32(b"6789"), 4) == 0xCBF43926


# ---------------------------------------------------------------- header
@pytest.mark.parametrize("check_log", [8, 12, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003, 1 << 39])
def test_header_round_trip(check_log, n):
    lib = _lib.load()
    n_cb = K.n_cb_of(n, check_log)
    crc = 0xCAFEF00D if n else 0
    info = _lib.CheckInfo(1, 1, check_log, 0, n, n_cb, crc, 0xBAD, 0)  # header_crc is not read
    out = (C.c_uint8 * 32)()
    assert lib.fsehip_check_write_header(C.byref(info), out) == 0
    assert bytes(out) == K.header(check_log, n, n_cb, crc)
    rc, got = read(bytes(out) + b"\x00" * 5)
    assert rc == 0
    assert (got.version, got.algorithm, got.check_log, got.reserved, got.n_content, got.n_cb, got.content_crc,
            got.header_crc) == (1, 1, check_log, 0, n, n_cb, crc, zlib.crc32(bytes(out)[:28]))
    assert lib.fsehip_check_bytes(n, check_log) == 32 + 4 * n_cb == K.record_bytes(n, check_log)


def test_check_bytes():
    lib = _lib.load()
    assert lib.fsehip_check_bytes(0, 16) == 32 and lib.fsehip_check_bytes(1, 0) == 36  # 0 = the default, 16
    assert lib.fsehip_check_bytes(65537, 0) == 40
    for bad in (1, 7, 17, 32):
        assert lib.fsehip_check_bytes(1000, bad) == 0
    assert lib.fsehip_check_bytes(1 << 40, 8) == 0  # 2^32 blocks: one too many


def test_check_bytes_block_count_limit():
    lib = _lib.load()
    assert lib.fsehip_check_bytes(((1 << 32) - 1) << 8, 8) == 32 + 4 * ((1 << 32) - 1)
    assert lib.fsehip_check_bytes((((1 << 32) - 1) << 8) + 1, 8) == 0  # n_cb would be 2^32
    assert lib.fsehip_check_bytes(U64_MAX, 16) == 0


def hdr(n=100003, check_log=12, n_cb=None, crc=0x12345678, **kw):
    return K.header(check_log, n, K.n_cb_of(n, check_log) if n_cb is None else n_cb, crc, **kw)


REJECTS = {
    "short-31": hdr()[:31],
    "short-0": b"",
    "magic": hdr(magic=b"FSEF"),
    "version-0": hdr(version=0),
    "version-2": hdr(version=2),
    "algorithm-0": hdr(algorithm=0),
    "algorithm-2": hdr(algorithm=2),
    "check_log-7": hdr(check_log=7),
    "check_log-17": hdr(check_log=17),
    "byte-7": hdr(byte7=1),
    "reserved-word": hdr(reserved=1),
    "reserved-word-high": hdr(reserved=1 << 31),
    "n_cb-plus-1": hdr(n_cb=K.n_cb_of(100003, 12) + 1),
    "n_cb-minus-1": hdr(n_cb=K.n_cb_of(100003, 12) - 1),
    "n_cb-zero": hdr(n_cb=0),
    "n_cb-overflows": hdr(n=U64_MAX, check_log=8, n_cb=0),
    "empty-with-a-crc": hdr(n=0, crc=5),
    "header_crc-bit-0": hdr(header_crc=zlib.crc32(hdr()[:28]) ^ 1),
    "header_crc-bit-31": hdr(header_crc=zlib.crc32(hdr()[:28]) ^ (1 << 31)),
    "content_crc-flipped-header_crc-kept": hdr()[:20] + struct.pack("<I", 0x12345679) + hdr()[24:],
}


def test_the_reject_bases_are_valid():
    assert read(hdr())[0] == 0 and read(hdr(n=0, crc=0))[0] == 0


@pytest.mark.parametrize("name", list(REJECTS))
def test_header_rejects(name):
    rc, info = read(REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.version, info.check_log, info.n_content, info.n_cb) == (0, 0, 0, 0)  # outputs zeroed


def test_write_header_rejects():
    lib = _lib.load()
    out = (C.c_uint8 * 32)()
    for info in (_lib.CheckInfo(2, 1, 12, 0, 5, 1, 0, 0, 0), _lib.CheckInfo(1, 2, 12, 0, 5, 1, 0, 0, 0),
                 _lib.CheckInfo(1, 1, 7, 0, 5, 1, 0, 0, 0), _lib.CheckInfo(1, 1, 17, 0, 5, 1, 0, 0, 0),
                 _lib.CheckInfo(1, 1, 12, 1, 5, 1, 0, 0, 0), _lib.CheckInfo(1, 1, 12, 0, 5, 2, 0, 0, 0),
                 _lib.CheckInfo(1, 1, 12, 0, 0, 0, 9, 0, 0)):
        assert st(lib.fsehip_check_write_header(C.byref(info), out)) == "BAD_ARG"
    assert st(lib.fsehip_check_write_header(None, out)) == "BAD_ARG"
    assert st(lib.fsehip_check_write_header(C.byref(_lib.CheckInfo(1, 1, 12, 0, 5, 1, 0, 0, 0)), None)) == "BAD_ARG"
    assert st(lib.fsehip_check_read_header(None, 32, C.byref(_lib.CheckInfo()))) == "BAD_ARG"
    assert st(lib.fsehip_check_read_header(OK, 32, None)) == "BAD_ARG"


# ---------------------------------------------------------------- the sealed head
def sealed_read(buf):
    a = arr(buf)
    info, kind, off = _lib.CheckInfo(), C.c_uint32(9), C.c_uint64(9)
    rc = _lib.load().fsehip_sealed_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                               C.byref(info), C.byref(kind), C.byref(off))
    return rc, info, kind.value, off.value


ELEMS = {"frame": np.arange(5000, dtype=np.uint8), "planes": np.arange(3001, dtype=np.int32),
         "delta": np.arange(2003, dtype=np.int64)}


@pytest.mark.parametrize("kind", ["frame", "planes", "delta"])
@pytest.mark.parametrize("check_log", [8, 16])
def test_sealed_head_of_each_kind(kind, check_log):
    a = ELEMS[kind]
    buf = K.seal(a, kind, 4096, 128, 2, check_log)
    rc, info, k, off = sealed_read(buf)
    assert rc == 0 and _lib.SEALED_KINDS[k] == kind
    assert off == K.record_bytes(a.nbytes, check_log) and info.n_content == a.nbytes
    assert info.content_crc == zlib.crc32(a.tobytes())
    inner = buf[off:]
    assert inner[:4] == {"frame": R.MAGIC, "planes": PR.MAGIC, "delta": DR.MAGIC}[kind]
    # the head alone is enough: the record and the container's first 32 / 48 bytes
    need = off + (32 if kind == "frame" else 48)
    assert sealed_read(buf[:need])[0] == 0
    assert st(sealed_read(buf[:need - 1])[0]) == "BAD_FRAME"
    assert st(sealed_read(buf[:off])[0]) == "BAD_FRAME" and st(sealed_read(buf[:31])[0]) == "BAD_FRAME"


@pytest.mark.parametrize("kind", ["frame", "planes", "delta"])
def test_sealed_head_rejects(kind):
    a = ELEMS[kind]
    rec = K.record(a.tobytes(), 12)
    shorter = K.seal(a[:-1], kind, 4096, 128, 2, 12)[K.record_bytes(a[:-1].nbytes, 12):]
    longer = K.seal(np.concatenate([a, a[:1]]), kind, 4096, 128, 2, 12)[K.record_bytes(a.nbytes + a.itemsize, 12):]
    good = K.seal(a, kind, 4096, 128, 2, 12)[len(rec):]
    assert sealed_read(rec + good)[0] == 0
    for name, inner in (("shorter", shorter), ("longer", longer), ("another-magic", b"FSEX" + good[4:]),
                        ("a-record-again", rec + good), ("nothing", b"")):
        rc, info, k, off = sealed_read(rec + inner)
        assert st(rc) == "BAD_FRAME", name
        assert (info.n_content, k, off) == (0, 0, 0), name  # outputs zeroed
    bad_record = K.header(12, a.nbytes, K.n_cb_of(a.nbytes, 12), 1, version=2) + rec[32:]
    assert st(sealed_read(bad_record + good)[0]) == "BAD_FRAME"
    lib = _lib.load()
    assert st(lib.fsehip_sealed_read_header(OK, 100, None, C.byref(C.c_uint32()), C.byref(C.c_uint64()))) == "BAD_ARG"
    assert st(lib.fsehip_sealed_read_header(None, 100, C.byref(_lib.CheckInfo()), C.byref(C.c_uint32()),
                                            C.byref(C.c_uint64()))) == "BAD_ARG"


# ---------------------------------------------------------------- the range planner
def franges(*r):
    return (_lib.FrameRange * max(len(r), 1))(*[_lib.FrameRange(*x) for x in r])


def verified(info, r):
    out = C.c_uint64(77)
    rc = _lib.load().fsehip_check_ranges_verified_bytes(C.byref(info), franges(*r), len(r), C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("check_log", [8, 9])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 1024, 1300])
def test_verified_bytes_against_the_per_byte_model(check_log, n):
    info = info_of(n, check_log)
    B = 1 << check_log
    rng = np.random.default_rng(n + check_log)
    edges = sorted({0, n, *(k * B + d for k in range(n // B + 2) for d in (-1, 0, 1) if 0 <= k * B + d <= n)})
    ranges = [(s, e - s, 0) for s in edges for e in edges if e >= s]
    for r in ranges:
        assert verified(info, [r]) == (0, K.verified_bytes(n, check_log, [r])), r
    some = [ranges[i] for i in rng.integers(0, len(ranges), 40)]
    assert verified(info, some) == (0, K.verified_bytes(n, check_log, some))
    assert verified(info, []) == (0, 0)


def test_verified_bytes_rejects():
    info = info_of(1000, 8)
    assert st(verified(info, [(999, 2, 0)])[0]) == "BAD_ARG"
    assert st(verified(info, [(1001, 0, 0)])[0]) == "BAD_ARG"
    assert st(verified(info, [(U64_MAX, 2, 0)])[0]) == "BAD_ARG"
    lib = _lib.load()
    out = C.c_uint64()
    assert st(lib.fsehip_check_ranges_verified_bytes(None, franges((0, 1, 0)), 1, C.byref(out))) == "BAD_ARG"
    assert st(lib.fsehip_check_ranges_verified_bytes(C.byref(info), None, 1, C.byref(out))) == "BAD_ARG"
    assert st(lib.fsehip_check_ranges_verified_bytes(C.byref(info), franges((0, 1, 0)), 1, None)) == "BAD_ARG"
    bad = info_of(1000, 8)
    bad.n_cb = 5
    assert st(verified(bad, [(0, 1, 0)])[0]) == "BAD_ARG"
    assert verified(info_of((1 << 40), 16), [(0, 1 << 40, 0), (65536, (1 << 40) - 65536, 0)]) == (0, (2 << 40) - 65536)


# ---------------------------------------------------------------- argument checks before any device use
ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


# fsehip_check_build(check_log, d_content, n_content, d_record, stream)
row("build-null-record", "BAD_ARG", lambda lib: lib.fsehip_check_build(16, OK, 100, None, None))
row("build-null-content", "BAD_ARG", lambda lib: lib.fsehip_check_build(16, None, 100, OK, None))
row("build-check_log-7", "UNSUPPORTED", lambda lib: lib.fsehip_check_build(7, OK, 100, OK, None))
row("build-check_log-17", "UNSUPPORTED", lambda lib: lib.fsehip_check_build(17, OK, 100, OK, None))
row("build-too-many-blocks", "UNSUPPORTED", lambda lib: lib.fsehip_check_build(8, OK, 1 << 41, OK, None))
row("build-null-before-check_log", "BAD_ARG", lambda lib: lib.fsehip_check_build(7, OK, 100, None, None))


# fsehip_check_verify(info, d_record, d_content, n_content, d_check_status, d_result, stream)
def cv(info=None, rec=OK, content=OK, n=100003, status=OK, res=OK, null_info=False):
    info = info_of() if info is None else info
    ref = None if null_info else C.byref(info)
    return lambda lib: lib.fsehip_check_verify(ref, rec, content, n, status, res, None)


def broken(**fields):
    info = info_of()
    for k, v in fields.items():
        setattr(info, k, v)
    return info


row("verify-null-info", "BAD_ARG", cv(null_info=True))
row("verify-null-record", "BAD_ARG", cv(rec=None))
row("verify-null-content", "BAD_ARG", cv(content=None))
row("verify-null-status", "BAD_ARG", cv(status=None))
row("verify-null-result", "BAD_ARG", cv(res=None))
row("verify-length-differs", "BAD_ARG", cv(n=100002))
row("verify-info-version-2", "BAD_ARG", cv(info=broken(version=2)))
row("verify-info-check_log-17", "BAD_ARG", cv(info=broken(check_log=17)))
row("verify-info-n_cb-wrong", "BAD_ARG", cv(info=broken(n_cb=3)))
row("verify-info-reserved", "BAD_ARG", cv(info=broken(reserved=1)))
row("verify-info-header_crc-wrong", "BAD_ARG", cv(info=broken(header_crc=1)))


# fsehip_check_verify_ranges(info, d_record, ranges, n_ranges, d_out, out_cap, d_range_status, d_result, stream)
def vr(r=((0, 10, 0),), info=None, rec=OK, out=OK, ocap=1 << 20, status=OK, res=OK, null_info=False,
       null_ranges=False):
    info = info_of() if info is None else info
    ref = None if null_info else C.byref(info)
    a = None if null_ranges else franges(*r)
    return lambda lib: lib.fsehip_check_verify_ranges(ref, rec, a, len(r), out, ocap, status, res, None)


N = 100003
row("ranges-null-info", "BAD_ARG", vr(null_info=True))
row("ranges-null-record", "BAD_ARG", vr(rec=None))
row("ranges-null-result", "BAD_ARG", vr(res=None))
row("ranges-null-ranges", "BAD_ARG", vr(null_ranges=True))
row("ranges-null-out", "BAD_ARG", vr(out=None))
row("ranges-null-status", "BAD_ARG", vr(status=None))
row("ranges-bad-info", "BAD_ARG", vr(info=broken(n_cb=3)))
row("ranges-past-the-end", "BAD_ARG", vr(r=((N - 5, 6, 0),)))
row("ranges-offset-past-the-end", "BAD_ARG", vr(r=((N + 1, 0, 0),)))
row("ranges-source-overflows", "BAD_ARG", vr(r=((U64_MAX, 2, 0),)))
row("ranges-destination-overflows", "BAD_ARG", vr(r=((0, 2, U64_MAX),)))
row("ranges-overlapping-destinations", "BAD_ARG", vr(r=((0, 10, 0), (50, 10, 9))))
row("ranges-overlap-out-of-order", "BAD_ARG", vr(r=((0, 10, 20), (50, 10, 0), (70, 5, 24))))
row("ranges-overlap-before-too-small", "BAD_ARG", vr(r=((0, 10, 0), (50, 10, 9)), ocap=4))
row("ranges-destination-past-out-cap", "DST_TOO_SMALL", vr(r=((0, 10, 0),), ocap=9))
row("ranges-empty-range-past-out-cap", "DST_TOO_SMALL", vr(r=((0, 0, 11),), ocap=10))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_valid_calls_reach_the_device_check():
    """The same calls with valid arguments reach the device check: NO_DEVICE
    without a GPU (with one they would run on fake pointers: nothing to do)."""
    import torch

    if torch.cuda.is_available():
        return
    lib = _lib.load()
    for call in (cv(), cv(content=ODD, rec=ODD), cv(info=info_of(0, 16), n=0, content=None, status=None),
                 vr(r=((0, 10, 0), (50, 10, 10), (7, 0, 5))), vr(r=()), vr(r=(), out=None, status=None),
                 vr(r=((5, 0, 0),), out=None),
                 lambda lib: lib.fsehip_check_build(16, ODD, 100, ODD, None),
                 lambda lib: lib.fsehip_check_build(0, None, 0, OK, None),
                 lambda lib: lib.fsehip_check_build(8, OK, ((1 << 32) - 1) << 8, OK, None)):
        assert st(call(lib)) == "NO_DEVICE"


def test_python_api_without_gpu():
    from entropy_coders_amd import BlockCodec, FseError, sealed_decompress

    with pytest.raises(FseError) as e:
        BlockCodec.check_info(b"\0" * 32)
    assert e.value.code == "BAD_FRAME"
    a = np.arange(1000, dtype=np.int32)
    buf = K.seal(a, "planes", 4096, 128, 2, 8)
    info, kind, off = BlockCodec.sealed_info(buf)
    assert (info.n_content, info.n_cb, info.check_log, kind, off) == (4000, 16, 8, "planes", 32 + 64)
    assert BlockCodec.check_info(buf).content_crc == zlib.crc32(a.tobytes())
    with pytest.raises(FseError) as e:
        BlockCodec.sealed_info(buf[:off] + b"FSEX" + buf[off + 4:])
    assert e.value.code == "BAD_FRAME"
    with pytest.raises(FseError) as e:
        sealed_decompress(buf[:40])  # not a sealed buffer: BAD_FRAME before any device work
    assert e.value.code == "BAD_FRAME"
    with pytest.raises(ValueError):
        BlockCodec._check_log(1000)
    assert BlockCodec._check_log(256) == 8 and BlockCodec._check_log(65536) == 16
