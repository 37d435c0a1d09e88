"""The member check record's and the sealed pack's host side (include/fsehip.h
section 2l), no GPU: header write / read against tests/spack_ref.py over
valid heads and every reject rule, the sealed pack's head reader (flag bit 0
in front of "FSEM", n_members or content_bytes that differ from the pack's),
the two-way magic rejections against every other reader, the container kind,
the size formulas, and the argument checks the device calls make before they
ask for a device (fake non-null pointers, never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as R
import pack_ref as KR
import spack_ref as SR
import vpack_ref as VR
from entropy_coders_amd import _lib

U64_MAX = (1 << 64) - 1
SPECS = [("diff", 2, 100003), ("delta", 8, 17), ("planes", 1, 5), ("diff", 4, 0), ("planes", 4, 4096), ("diff", 8, 33)]
PLAIN = [("planes" if k == "diff" else k, w, n) for k, w, n in SPECS]
N = len(SPECS)
CONTENT = VR.sums(SPECS)[1]
UNIT = 65536


def st(rc):
    return _lib.STATUS[rc]


def arr_of(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def members(specs=SPECS, ptrs=None):
    arr = (_lib.PackMember * max(len(specs), 1))()
    for m, (kind, w, n) in enumerate(specs):
        arr[m] = _lib.PackMember(((m + 1) << 32) if ptrs is None else ptrs[m], n, w, VR.KIND.get(kind, kind))
    return arr


def base_array(specs=SPECS):
    arr = (C.c_void_p * max(len(specs), 1))()
    for m in range(len(specs)):
        arr[m] = ((m + 1) << 32) + (1 << 48)
    return arr


def read_header(buf):
    a = arr_of(buf)
    info = _lib.McheckInfo()
    rc = _lib.load().fsehip_mcheck_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), C.byref(info))
    return rc, info


def spack_head(specs=SPECS, versioned=True, flags=None, n=None, content=None, inner_magic=None, **kw):
    """A sealed pack's head: the record (a zero table), the pack's head and the inner frame's header."""
    flags = int(versioned) if flags is None else flags
    rec = SR.header(len(specs) if n is None else n, VR.sums(specs)[1] if content is None else content, flags, **kw)
    pack = (VR if versioned else KR).header(specs) + R.header(2, 11, 4096, 128, VR.sums(specs)[0])
    if inner_magic:
        pack = inner_magic + pack[4:]
    return rec + bytes(8 * len(specs)) + pack


def read_spack(buf):
    a = arr_of(buf)
    info, v, off = _lib.McheckInfo(), C.c_uint32(7), C.c_uint64(7)
    rc = _lib.load().fsehip_spack_read_header(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), C.byref(info),
                                              C.byref(v), C.byref(off))
    return rc, info, v.value, off.value


def zeroed(info):
    return bytes(info) == bytes(C.sizeof(_lib.McheckInfo))


# ---------------------------------------------------------------- the record's header
def test_constants_and_sizes():
    L = _lib.load()
    assert _lib.KIND_SPACK == 7 and _lib.MCHECK_BASES == 1 and C.sizeof(_lib.McheckInfo) == 32
    assert [L.fsehip_mcheck_bytes(n) for n in (0, 1, 5, 1 << 20)] == [32, 40, 72, 32 + 8 * (1 << 20)]
    assert L.fsehip_mcheck_bytes((1 << 20) + 1) == 0


@pytest.mark.parametrize("n,content,flags", [(0, 0, 0), (1, 1, 1), (N, CONTENT, 1), (1 << 20, U64_MAX, 0)])
def test_valid_headers_round_trip(n, content, flags):
    want = SR.header(n, content, flags)
    rc, info = read_header(want)
    assert rc == 0
    f = SR.parse_header(want)
    assert (info.version, info.algorithm, info.flags, info.n_members, info.content_bytes, info.header_crc,
            info.reserved) == (1, 1, flags, n, content, f["header_crc"], 0)
    out = (C.c_uint8 * 32)()
    info.header_crc = 0  # computed, not read
    assert _lib.load().fsehip_mcheck_write_header(C.byref(info), out) == 0 and bytes(out) == want


REJECTS = {
    "magic": dict(magic=b"FSEK"), "version": dict(version=2), "version-0": dict(version=0),
    "algorithm": dict(algorithm=0), "flags": dict(flags=2), "flags-high": dict(flags=0x81), "spare": dict(spare=1),
    "reserved0": dict(reserved0=1), "reserved1": dict(reserved1=1 << 31), "header_crc": dict(header_crc=0x12345678),
    "n_members": dict(n=(1 << 20) + 1),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_header_reject_rules(name):
    kw = dict(REJECTS[name])
    bad = SR.header(kw.pop("n", N), CONTENT, kw.pop("flags", 1), **kw)
    with pytest.raises(SR.SpackError):
        SR.parse_header(bad)
    rc, info = read_header(bad)
    assert st(rc) == "BAD_FRAME" and zeroed(info)


def test_header_truncated_null_and_writer_rejects():
    L = _lib.load()
    good = SR.header(N, CONTENT, 1)
    for k in (0, 1, 4, 31):
        rc, info = read_header(good[:k])
        assert st(rc) == "BAD_FRAME" and zeroed(info)
    assert st(L.fsehip_mcheck_read_header(None, 32, C.byref(_lib.McheckInfo()))) == "BAD_ARG"
    a = arr_of(good)
    assert st(L.fsehip_mcheck_read_header(a.ctypes.data_as(C.c_void_p), 32, None)) == "BAD_ARG"
    out = (C.c_uint8 * 32)()
    for field, val in (("version", 2), ("algorithm", 3), ("flags", 2), ("n_members", (1 << 20) + 1), ("reserved", 1)):
        info = _lib.McheckInfo(1, 1, 1, N, CONTENT, 0, 0)
        setattr(info, field, val)
        assert st(L.fsehip_mcheck_write_header(C.byref(info), out)) == "BAD_ARG", field
    assert st(L.fsehip_mcheck_write_header(None, out)) == "BAD_ARG"
    assert st(L.fsehip_mcheck_write_header(C.byref(_lib.McheckInfo(1, 1, 1, N, CONTENT, 0, 0)), None)) == "BAD_ARG"


# ---------------------------------------------------------------- the sealed pack's head
@pytest.mark.parametrize("versioned,flags", [(True, 1), (True, 0), (False, 0)])
def test_sealed_pack_head(versioned, flags):
    specs = SPECS if versioned else PLAIN
    rc, info, v, off = read_spack(spack_head(specs, versioned, flags))
    assert rc == 0 and v == int(versioned) and off == 32 + 8 * N
    assert (info.flags, info.n_members, info.content_bytes) == (flags, N, CONTENT)
    rc, info, v, off = read_spack(spack_head([], versioned, flags))
    assert rc == 0 and off == 32 and info.n_members == 0


@pytest.mark.parametrize("name,buf", [
    ("base CRCs in front of a pack frame", lambda: spack_head(PLAIN, False, flags=1)),
    ("n_members", lambda: SR.header(N - 1, CONTENT, 1) + bytes(8 * (N - 1)) + spack_head()[32 + 8 * N:]),
    ("content_bytes", lambda: spack_head(content=CONTENT + 1)),
    ("a frame behind the record", lambda: spack_head(inner_magic=b"FSEF")),
    ("a sealed buffer behind the record", lambda: spack_head(inner_magic=b"FSEK")),
    ("a record behind the record", lambda: spack_head(inner_magic=b"FSES")),
    ("a damaged pack header", lambda: spack_head()[: 32 + 8 * N + 5] + b"\x01" + spack_head()[32 + 8 * N + 6:]),
    ("no pack", lambda: spack_head()[: 32 + 8 * N + 3]),
    ("a short pack header", lambda: spack_head()[: 32 + 8 * N + 31]),
    ("a short table", lambda: spack_head()[: 32 + 8 * N - 1]),
    ("the record's own rules", lambda: spack_head(version=3)),
])
def test_sealed_pack_head_rejects(name, buf):
    rc, info, v, off = read_spack(buf())
    assert st(rc) == "BAD_FRAME" and zeroed(info) and v == 0 and off == 0, name


def test_magics_crossed_with_every_other_reader():
    """"FSES" is BAD_FRAME to every existing reader, and their magics are BAD_FRAME to this one."""
    L = _lib.load()
    sealed = spack_head()
    a = arr_of(sealed)
    p, n = a.ctypes.data_as(C.c_void_p), len(a)
    fi, pi, ci, ki = _lib.FrameInfo(), _lib.PlanesInfo(), _lib.CheckInfo(), _lib.PackInfo()
    kind, off = C.c_uint32(), C.c_uint64()
    arr = (_lib.PackMember * 64)()
    assert st(L.fsehip_frame_read_header(p, n, C.byref(fi))) == "BAD_FRAME"
    for prefix in ("planes", "delta", "diff"):
        assert st(getattr(L, f"fsehip_{prefix}_read_header")(p, n, C.byref(pi), C.byref(fi))) == "BAD_FRAME", prefix
    assert st(L.fsehip_check_read_header(p, n, C.byref(ci))) == "BAD_FRAME"
    assert st(L.fsehip_sealed_read_header(p, n, C.byref(ci), C.byref(kind), C.byref(off))) == "BAD_FRAME"
    for prefix in ("pack", "vpack"):
        assert st(getattr(L, f"fsehip_{prefix}_read_header")(p, n, C.byref(ki))) == "BAD_FRAME", prefix
        assert st(getattr(L, f"fsehip_{prefix}_read_members")(p, n, arr, 64, C.byref(ki), C.byref(fi))) == "BAD_FRAME"
    assert L.fsehip_container_kind(p, n) == _lib.KIND_SPACK
    for magic in (b"FSEF", b"FSEP", b"FSED", b"FSEB", b"FSEK", b"FSEM", b"FSEV", b"FSEX"):
        other = magic + sealed[4:]
        rc, info = read_header(other)
        assert st(rc) == "BAD_FRAME" and zeroed(info), magic
        assert st(read_spack(other)[0]) == "BAD_FRAME", magic
    # a sealed buffer (section 2f) does not take a pack, sealed or not, as its container
    from entropy_coders_amd import container_kind

    assert container_kind(sealed) == "spack"


# ---------------------------------------------------------------- sizes
def test_bound_and_scratch_sizes():
    L = _lib.load()
    for specs, versioned in ((SPECS, 1), (PLAIN, 0), ([], 1), ([], 0)):
        arr, n = members(specs), len(specs)
        prefix = "fsehip_vpack_" if versioned else "fsehip_pack_"
        for block in (4096, 65536):
            assert L.fsehip_spack_bound(arr, n, versioned, block) == 32 + 8 * n + getattr(L, prefix + "bound")(arr, n, block)
        pack = getattr(L, prefix + "scratch_bytes")(arr, n)
        units = sum(-(-(w * cnt) // UNIT) for _, w, cnt in specs)
        base_units = sum(-(-(w * cnt) // UNIT) for k, w, cnt in specs if k == "diff")
        need = L.fsehip_spack_scratch_bytes(arr, n, versioned)
        # the pack's scratch, then at least the gate, the descriptors, a CRC per unit and per span of each list
        lists = 2 if versioned else 1
        assert need >= -(-pack // 16) * 16 + 64 + 40 * n * lists + 4 * (units + base_units * versioned) + 4 * n * lists
        assert need <= -(-pack // 16) * 16 + 64 + 40 * n * lists + 4 * (units + base_units) + 4 * n * lists + 128
        assert need % 16 == 0
        assert L.fsehip_mcheck_scratch_bytes(arr, n, None, 0, versioned) == need - -(-pack // 16) * 16
    arr = members()
    sel = (C.c_uint32 * 3)(5, 0, 2)
    need = L.fsehip_spack_members_scratch_bytes(arr, N, 1, sel, 3)
    pack = L.fsehip_vpack_members_scratch_bytes(arr, N, sel, 3)
    assert need == -(-pack // 16) * 16 + L.fsehip_mcheck_scratch_bytes(arr, N, sel, 3, 1)
    assert L.fsehip_mcheck_scratch_bytes(arr, N, sel, 3, 0) < L.fsehip_mcheck_scratch_bytes(arr, N, sel, 3, 1)
    bad = (C.c_uint32 * 1)(N)
    assert L.fsehip_spack_members_scratch_bytes(arr, N, 1, bad, 1) == 0
    assert L.fsehip_mcheck_scratch_bytes(arr, N, bad, 1, 0) == 0
    # an invalid list: a diff member in front of a pack frame, a width outside the list
    assert L.fsehip_spack_bound(arr, N, 0, 4096) == 0 and L.fsehip_spack_scratch_bytes(arr, N, 0) == 0
    odd = members([("planes", 3, 10)])
    assert L.fsehip_spack_bound(odd, 1, 1, 4096) == 0 and L.fsehip_mcheck_scratch_bytes(odd, 1, None, 0, 0) == 0


# ---------------------------------------------------------------- the device calls' checks, no device needed
def test_device_calls_reject_before_any_device_use():
    L = _lib.load()
    arr, barr = members(), base_array()
    ok = C.c_void_p(1 << 20)
    p = _lib.FrameParams(4096, 0, 128, 0, 2, 0)
    need, bound = L.fsehip_spack_scratch_bytes(arr, N, 1), L.fsehip_spack_bound(arr, N, 1, 4096)
    f = L.fsehip_spack_compress
    assert st(f(None, arr, N, barr, 1, ok, need, ok, bound, ok, ok, None)) == "BAD_ARG"
    assert st(f(C.byref(p), arr, N, barr, 1, C.c_void_p((1 << 20) + 8), need, ok, bound, ok, ok, None)) == "BAD_ARG"
    assert st(f(C.byref(p), arr, N, barr, 1, ok, need - 1, ok, bound, ok, ok, None)) == "DST_TOO_SMALL"
    assert st(f(C.byref(p), arr, N, barr, 1, ok, need, ok, bound - 1, ok, ok, None)) == "DST_TOO_SMALL"
    assert st(f(C.byref(p), arr, N, None, 1, ok, need, ok, bound, ok, ok, None)) == "UNSUPPORTED"
    mneed = L.fsehip_mcheck_scratch_bytes(arr, N, None, 0, 1)
    assert st(L.fsehip_mcheck_build(arr, barr, N, None, ok, mneed, None)) == "BAD_ARG"
    assert st(L.fsehip_mcheck_build(arr, barr, N, ok, ok, mneed - 1, None)) == "DST_TOO_SMALL"
    nobase = base_array()
    nobase[0] = None
    assert st(L.fsehip_mcheck_build(arr, nobase, N, ok, ok, mneed, None)) == "BAD_ARG"
    misaligned = members(ptrs=[((m + 1) << 32) + (1 if m == 5 else 0) for m in range(N)])
    assert st(L.fsehip_mcheck_build(misaligned, barr, N, ok, ok, mneed, None)) == "BAD_ARG"
    info = _lib.McheckInfo(1, 1, 1, N, CONTENT, 0, 0)
    g = L.fsehip_mcheck_verify
    assert st(g(C.byref(info), ok, arr, None, 0, 2, None, ok, mneed, ok, ok, None)) == "BAD_ARG"
    assert st(g(C.byref(info), ok, arr, None, 0, 1, None, ok, mneed, ok, ok, None)) == "BAD_ARG"
    assert st(g(C.byref(info), ok, arr, None, 0, 0, None, ok, 16, ok, ok, None)) == "DST_TOO_SMALL"
    assert st(g(C.byref(_lib.McheckInfo(1, 1, 1, N, CONTENT + 1, 0, 0)), ok, arr, None, 0, 0, None, ok, mneed, ok, ok,
                None)) == "BAD_ARG"
    twice = (C.c_uint32 * 2)(3, 3)
    assert st(g(C.byref(info), ok, arr, twice, 2, 0, None, ok, mneed, ok, ok, None)) == "BAD_ARG"
