"""The versioned pack's host side (include/fsehip.h section 2k), no GPU:
header and table write / read, every reject rule of section 2j under the
magic "FSEV", kind 4 accepted and kinds 0, 3 and 5 rejected, the two-way magic
rejections against the seven other readers, the container kind, the size
formulas, and every argument check the device calls make before they ask for
a device (fake non-null pointers, never dereferenced, as in
tests/test_pack_format.py): the pack calls' checks, the base pointers', and
the decode side's overlap rules.  Expected bytes come from tests/vpack_ref.py."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import diff_ref as FR
import frame_ref as R
import pack_ref as KR
import planes_ref as PR
import vpack_ref as VR
from entropy_coders_amd import _lib

OK = C.c_void_p(4096)
ODD8 = C.c_void_p(4096 + 8)
U64_MAX = (1 << 64) - 1
SPECS = [("diff", 2, 100003), ("delta", 8, 17), ("planes", 1, 5), ("diff", 4, 0), ("planes", 4, 4096), ("diff", 8, 33)]
N = len(SPECS)


def st(rc):
    return _lib.STATUS[rc]


def members(specs=SPECS, ptrs=None):
    """The PackMember array of specs; ptrs: per member an address (default: (m + 1) << 32, aligned and disjoint)."""
    arr = (_lib.PackMember * max(len(specs), 1))()
    for m, (kind, w, n) in enumerate(specs):
        ptr = ((m + 1) << 32) if ptrs is None else ptrs[m]
        arr[m] = _lib.PackMember(ptr, n, w, VR.KIND.get(kind, kind))
    return arr


def base_array(specs=SPECS, ptrs=None):
    """The host array of base pointers; default: (m + 1) << 32 plus 1 << 48, aligned, disjoint from the members."""
    arr = (C.c_void_p * max(len(specs), 1))()
    for m in range(len(specs)):
        arr[m] = (((m + 1) << 32) + (1 << 48)) if ptrs is None else ptrs[m]
    return arr


def head(specs=SPECS, block=4096, n_total=None, inner_magic=None, **kw):
    image = VR.sums(specs)[0] if n_total is None else n_total
    inner = R.header(2, 11, block, 128, image)
    if inner_magic:
        inner = inner_magic + inner[4:]
    return VR.header(specs, **kw) + inner


def read_header(buf, fn="fsehip_vpack_read_header"):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    info = _lib.PackInfo()
    rc = getattr(_lib.load(), fn)(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), C.byref(info))
    return rc, info


def read_members(buf, cap=64, fn="fsehip_vpack_read_members"):
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    arr, info, inner = (_lib.PackMember * max(cap, 1))(), _lib.PackInfo(), _lib.FrameInfo()
    rc = getattr(_lib.load(), fn)(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), arr, cap, C.byref(info),
                                  C.byref(inner))
    return rc, arr, info, inner


def patch(buf, at, val):
    b = bytearray(buf)
    b[at] = val
    return bytes(b)


# ---------------------------------------------------------------- header and table
def test_constants():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "fsehip.h")).read()
    assert "#define FSEHIP_KIND_VPACK 6u" in src and "(2k) Versioned pack" in src
    assert "THE CONTAINER DOES NOT IDENTIFY ITS BASES" in src
    assert _lib.KIND_VPACK == 6 and C.sizeof(_lib.PackMember) == 24


def test_head_round_trip():
    lib = _lib.load()
    out = np.zeros(32 + 16 * N, np.uint8)
    assert lib.fsehip_vpack_write_header(members(), N, out.ctypes.data_as(C.c_void_p)) == 0
    assert out.tobytes() == VR.header(SPECS) and out[:4].tobytes() == b"FSEV"
    rc, info = read_header(head())
    image, content = VR.sums(SPECS)
    assert rc == 0 and (info.version, info.n_members, info.image_bytes, info.content_bytes) == (1, N, image, content)
    rc, arr, info, inner = read_members(head(block=65536))
    assert rc == 0 and info.n_members == N and inner.n_total == image and inner.block_size == 65536
    got = [(VR.KIND_NAME[arr[m].kind], arr[m].elem_bytes, arr[m].n_elems, arr[m].d_ptr) for m in range(N)]
    assert got == [s + (None,) for s in SPECS]


def test_empty_versioned_pack_is_64_bytes():
    buf = VR.build([], 65536, 128, 2)
    rc, arr, info, inner = read_members(buf, cap=0)
    assert len(buf) == 64 and rc == 0 and (info.n_members, info.image_bytes, inner.n_total, inner.n_blocks) == (0, 0, 0, 0)


HEADER_REJECTS = {
    "short-31": head()[:31],
    "short-0": b"",
    "magic-FSEM": head(magic=b"FSEM"),
    "magic-FSEF": head(magic=b"FSEF"),
    "magic-FSEP": head(magic=b"FSEP"),
    "magic-FSED": head(magic=b"FSED"),
    "magic-FSEB": head(magic=b"FSEB"),
    "magic-FSEK": head(magic=b"FSEK"),
    "version-0": head(version=0),
    "version-2": head(version=2),
    "reserved-byte-5": patch(head(), 5, 1),
    "reserved-byte-7": patch(head(), 7, 0x80),
    "reserved-byte-12": patch(head(), 12, 1),
    "reserved-byte-15": patch(head(), 15, 1),
    "n_members-above-the-cap": head(n_members=(1 << 20) + 1),
}
TABLE_REJECTS = {
    "table-truncated": head()[: 32 + 16 * N - 1],
    "inner-header-truncated": head()[: 32 + 16 * N + 31],
    "kind-0": patch(head(), 32, 0),
    "kind-3": patch(head(), 32, 3),
    "kind-5": patch(head(), 32, 5),
    "kind-6": patch(head(), 32 + 16, 6),
    "width-0": patch(head(), 33, 0),
    "width-3": patch(head(), 33, 3),
    "width-16": patch(head(), 33, 16),
    "member-reserved-2": patch(head(), 34, 1),
    "member-reserved-7": patch(head(), 32 + 16 + 7, 1),
    "image_bytes-differs": head(image_bytes=VR.sums(SPECS)[0] + 16),
    "content_bytes-differs": head(content_bytes=VR.sums(SPECS)[1] - 1),
    "n_elems-differs": patch(head(), 32 + 8, head()[32 + 8] ^ 1),
    "stride-overflows": head([("diff", 2, U64_MAX - 3)], image_bytes=0, content_bytes=0, n_total=0),
    "member-image-overflows": head([("diff", 8, 1 << 62)], image_bytes=0, content_bytes=0, n_total=0),
    "sum-overflows": head([("planes", 4, 1 << 61), ("diff", 4, 1 << 61)], image_bytes=0, content_bytes=0, n_total=0),
    "inner-magic-FSEV": head(inner_magic=b"FSEV"),
    "inner-magic-FSEM": head(inner_magic=b"FSEM"),
    "inner-n_total-plus-16": head(n_total=VR.sums(SPECS)[0] + 16),
    "inner-n_total-content": head(n_total=VR.sums(SPECS)[1]),
}


@pytest.mark.parametrize("name", list(HEADER_REJECTS))
def test_header_rejects(name):
    rc, info = read_header(HEADER_REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.version, info.n_members, info.image_bytes, info.content_bytes) == (0, 0, 0, 0)  # zeroed
    assert st(read_members(HEADER_REJECTS[name])[0]) == "BAD_FRAME"


@pytest.mark.parametrize("name", list(TABLE_REJECTS))
def test_table_rejects(name):
    rc, arr, info, inner = read_members(TABLE_REJECTS[name])
    assert st(rc) == "BAD_FRAME", name
    assert (info.n_members, info.image_bytes, inner.n_total) == (0, 0, 0)  # outputs zeroed


def test_kind_4_is_accepted_here_and_nowhere_else():
    one = [("planes", 2, 5)]
    for kind in (1, 2, 4):
        rc, arr, info, _ = read_members(patch(head(one), 32, kind))
        assert rc == 0 and arr[0].kind == kind
    for kind in (0, 3, 5, 6, 255):
        assert st(read_members(patch(head(one), 32, kind))[0]) == "BAD_FRAME"
    # the same table under the pack frame's magic: kind 4 stays BAD_FRAME there
    as_pack = patch(head(one), 32, 4)
    as_pack = b"FSEM" + as_pack[4:]
    assert st(read_members(as_pack, fn="fsehip_pack_read_members")[0]) == "BAD_FRAME"


def test_read_members_argument_checks():
    lib = _lib.load()
    assert st(read_members(head(), cap=N - 1)[0]) == "DST_TOO_SMALL"
    assert st(lib.fsehip_vpack_read_header(None, 32, C.byref(_lib.PackInfo()))) == "BAD_ARG"
    assert st(lib.fsehip_vpack_read_header(OK, 32, None)) == "BAD_ARG"
    assert st(lib.fsehip_vpack_read_members(None, 64, None, 0, C.byref(_lib.PackInfo()), C.byref(_lib.FrameInfo()))) \
        == "BAD_ARG"
    assert st(lib.fsehip_vpack_write_header(members(), N, None)) == "BAD_ARG"
    assert st(lib.fsehip_vpack_write_header(members([("diff", 3, 5)]), 1, OK)) == "BAD_ARG"
    assert st(lib.fsehip_vpack_write_header(members([(3, 2, 5)]), 1, OK)) == "BAD_ARG"
    assert st(lib.fsehip_vpack_write_header(members([(5, 2, 5)]), 1, OK)) == "BAD_ARG"
    out = np.zeros(48, np.uint8)
    assert st(lib.fsehip_vpack_write_header(members([(4, 2, 5)]), 1, out.ctypes.data_as(C.c_void_p))) == "OK"
    assert out[32] == 4


def test_the_seven_other_readers_reject_a_versioned_pack_and_this_one_their_frames():
    lib = _lib.load()
    x = np.arange(100, dtype=np.int32)
    vpack = VR.build([("diff", x, x + 1), ("planes", x, None)], 4096, 128, 2)
    a = np.frombuffer(vpack, np.uint8)
    p, n = a.ctypes.data_as(C.c_void_p), len(a)
    pi, fi, ci = _lib.PlanesInfo(), _lib.FrameInfo(), _lib.CheckInfo()
    assert st(lib.fsehip_frame_read_header(p, n, C.byref(fi))) == "BAD_FRAME"
    for prefix in ("planes", "delta", "diff"):
        assert st(getattr(lib, f"fsehip_{prefix}_read_header")(p, n, C.byref(pi), C.byref(fi))) == "BAD_FRAME"
    assert st(lib.fsehip_check_read_header(p, n, C.byref(ci))) == "BAD_FRAME"
    kind, off = C.c_uint32(), C.c_uint64()
    assert st(lib.fsehip_sealed_read_header(p, n, C.byref(ci), C.byref(kind), C.byref(off))) == "BAD_FRAME"
    assert st(read_header(vpack, fn="fsehip_pack_read_header")[0]) == "BAD_FRAME"
    assert st(read_members(vpack, fn="fsehip_pack_read_members")[0]) == "BAD_FRAME"
    # a versioned pack without diff members too: the magic alone decides
    plain = VR.build([("planes", x, None)], 4096, 128, 2)
    assert st(read_members(plain, fn="fsehip_pack_read_members")[0]) == "BAD_FRAME" and read_members(plain)[0] == 0
    others = (R.build_frame(PR.raw_bytes(x), 4096, 128, 2), PR.build(x, 4096, 128, 2), DR.build(x, 4096, 128, 2),
              FR.build(x, x + 1, 4096, 128, 2), KR.build([x], 4096, 128, 2))
    for other in others:
        assert st(read_header(other)[0]) == "BAD_FRAME" and st(read_members(other)[0]) == "BAD_FRAME"


def test_container_kind_of_a_versioned_pack():
    from entropy_coders_amd import BlockCodec, auto_decompress, container_kind, pack_info

    lib = _lib.load()
    a = np.frombuffer(head(), np.uint8)
    assert lib.fsehip_container_kind(a.ctypes.data_as(C.c_void_p), 4) == 6
    assert container_kind(head()) == "vpack"
    with pytest.raises(ValueError, match="pack_decompress"):  # the message a pack gets
        auto_decompress(head(), np.int16)
    for magic, want in ((b"FSEF", 0), (b"FSEP", 1), (b"FSED", 2), (b"FSEK", 3), (b"FSEB", 4), (b"FSEM", 5)):  # as before
        b = np.frombuffer(magic + bytes(28), np.uint8)
        assert lib.fsehip_container_kind(b.ctypes.data_as(C.c_void_p), 32) == want
    assert st(lib.fsehip_container_kind(np.frombuffer(b"FSEv", np.uint8).ctypes.data_as(C.c_void_p), 4)) == "BAD_FRAME"
    # pack_info reads either magic and says which it saw
    h = pack_info(head())
    assert h.container == "vpack" and h.kinds == [k for k, _, _ in SPECS]
    assert (h.elem_bytes, h.n_elems) == ([w for _, w, _ in SPECS], [n for _, _, n in SPECS])
    h = BlockCodec.pack_info(KR.build([np.arange(9, dtype=np.int16)], 4096, 0, 2))
    assert h.container == "pack" and h.kinds == ["planes"]


# ---------------------------------------------------------------- sizes
def test_sizes():
    lib = _lib.load()
    arr = members()
    image, _ = VR.sums(SPECS)
    assert lib.fsehip_vpack_image_bytes(arr, N) == image
    for block in (4096, 65536):
        assert lib.fsehip_vpack_bound(arr, N, block) == VR.bound(SPECS, block) == 32 + 16 * N + lib.fsehip_frame_bound(
            image, block)
    scratch = lib.fsehip_vpack_scratch_bytes(arr, N)
    assert scratch % 16 == 0 and scratch >= image + (104 + 8) * N + 32 + 16 * N  # descriptors, base pointers, head
    sel = (C.c_uint32 * 3)(1, 5, 0)
    need = lib.fsehip_vpack_members_scratch_bytes(arr, N, sel, 3)
    assert need % 16 == 0
    assert need >= 8 * 32 + 8 * 48 + 2 * PR.stride_of(100003) + 4 * 18 + 3 * (104 + 8) + 32 + 16 * N
    assert lib.fsehip_vpack_members_scratch_bytes(arr, N, sel, 0) >= 32 + 16 * N
    assert lib.fsehip_vpack_members_scratch_bytes(arr, N, (C.c_uint32 * 1)(N), 1) == 0
    assert lib.fsehip_vpack_members_scratch_bytes(arr, N, None, 1) == 0
    assert lib.fsehip_vpack_bound(None, 0, 0) == 64 and lib.fsehip_vpack_image_bytes(None, 0) == 0
    # the pack frame's own sizes of a list both containers take: the image and the bound are the same
    both = [s for s in SPECS if s[0] != "diff"]
    assert lib.fsehip_pack_image_bytes(members(both), len(both)) == lib.fsehip_vpack_image_bytes(members(both), len(both))
    assert lib.fsehip_pack_bound(members(both), len(both), 4096) == lib.fsehip_vpack_bound(members(both), len(both), 4096)


@pytest.mark.parametrize("specs", [[("diff", 3, 5)], [("diff", 0, 5)], [(0, 2, 5)], [(3, 2, 5)], [(5, 2, 5)],
                                   [("diff", 2, U64_MAX - 3)], [("diff", 8, 1 << 62)],
                                   [("planes", 4, 1 << 61), ("diff", 4, 1 << 61)]],
                         ids=["width-3", "width-0", "kind-0", "kind-3", "kind-5", "stride", "member-image", "sum"])
def test_sizes_reject(specs):
    lib = _lib.load()
    arr, n = members(specs), len(specs)
    assert lib.fsehip_vpack_image_bytes(arr, n) == 0 and lib.fsehip_vpack_bound(arr, n, 65536) == 0
    assert lib.fsehip_vpack_scratch_bytes(arr, n) == 0
    assert lib.fsehip_vpack_members_scratch_bytes(arr, n, (C.c_uint32 * 1)(0), 1) == 0
    assert lib.fsehip_vpack_plane_offset(arr, n, 0, 0) == U64_MAX


def test_sizes_reject_too_many_members():
    lib = _lib.load()
    many = (_lib.PackMember * ((1 << 20) + 1))()
    for m in range(len(many)):
        many[m].elem_bytes, many[m].kind = 1, 4
    assert lib.fsehip_vpack_bound(many, 1 << 20, 65536) == 32 + (16 << 20) + 32
    assert lib.fsehip_vpack_bound(many, (1 << 20) + 1, 65536) == 0
    assert lib.fsehip_vpack_scratch_bytes(many, (1 << 20) + 1) == 0


# ---------------------------------------------------------------- argument checks before any device use
def fparams(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2, chunk=0):
    return C.byref(_lib.FrameParams(block, table_log, ckpt, mtl, nstates, chunk))


SMALL = [("diff", 2, 1000), ("delta", 8, 17), ("diff", 1, 5), ("diff", 4, 0), ("planes", 2, 8)]
NS = len(SMALL)
IMAGE, CONTENT = VR.sums(SMALL)
A = 1 << 32          # member m's default address is (m + 1) * A
B = 1 << 48          # and its default base address B + (m + 1) * A
TAIL = (104 + 8) * NS + 32 + 16 * NS  # the transforms' scratch: descriptors, base pointers, head


def infos(specs=SMALL, block=4096, n_total=None, n_blocks=None, image=None, content=None, n_members=None, version=1):
    img, cont = VR.sums(specs)
    n_total = img if n_total is None else n_total
    n_blocks = (n_total + block - 1) // block if n_blocks is None else n_blocks
    return (C.byref(_lib.PackInfo(version, len(specs) if n_members is None else n_members,
                                  img if image is None else image, cont if content is None else content)),
            C.byref(_lib.FrameInfo(1, 2, 11, 0, block, 0, n_blocks, 0, n_total, 0)))


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


def bases_of(specs, bptrs, null_bases):
    return None if null_bases else base_array(specs, bptrs)


# fsehip_vpack_split / _merge(members, n, d_bases, d_image, d_scratch, scratch_cap, stream)
for name in ("split", "merge"):
    def tr(specs=SMALL, ptrs=None, bptrs=None, null_bases=False, image=OK, scratch=OK, scap=1 << 20, null_members=False,
           fn="fsehip_vpack_" + name):
        arr = None if null_members else members(specs, ptrs)
        bs = bases_of(specs, bptrs, null_bases)
        return lambda lib: getattr(lib, fn)(arr, len(specs), bs, image, scratch, scap, None)

    row(f"{name}-null-members", "BAD_ARG", tr(null_members=True))
    row(f"{name}-kind-0", "UNSUPPORTED", tr([(0, 2, 5)]))
    row(f"{name}-kind-3", "UNSUPPORTED", tr([(3, 2, 5)]))
    row(f"{name}-kind-5", "UNSUPPORTED", tr([(5, 2, 5)]))
    row(f"{name}-width-3", "UNSUPPORTED", tr([("diff", 3, 5)]))
    row(f"{name}-width-before-null", "UNSUPPORTED", tr([("diff", 16, 5)], ptrs=[0], image=None))
    row(f"{name}-image-overflows", "UNSUPPORTED", tr([("diff", 8, 1 << 62)]))
    row(f"{name}-null-member-pointer", "BAD_ARG", tr(ptrs=[A, 0, 3 * A, 0, 5 * A]))
    row(f"{name}-member-odd-address", "BAD_ARG", tr(ptrs=[A + 1, 2 * A, 3 * A, 0, 5 * A]))
    row(f"{name}-member-4-of-8", "BAD_ARG", tr(ptrs=[A, 2 * A + 4, 3 * A, 0, 5 * A]))
    row(f"{name}-null-base", "BAD_ARG", tr(bptrs=[0, 0, B + 3 * A, 0, 0]))
    row(f"{name}-null-base-of-a-later-member", "BAD_ARG", tr(bptrs=[B + A, 0, 0, 0, 0]))
    row(f"{name}-base-odd-address", "BAD_ARG", tr(bptrs=[B + A + 1, 0, B + 3 * A, 0, 0]))
    row(f"{name}-null-bases-with-diff-members", "BAD_ARG", tr(null_bases=True))
    row(f"{name}-null-image", "BAD_ARG", tr(image=None))
    row(f"{name}-image-misaligned", "BAD_ARG", tr(image=ODD8))
    row(f"{name}-null-scratch", "BAD_ARG", tr(scratch=None))
    row(f"{name}-scratch-misaligned", "BAD_ARG", tr(scratch=ODD8))
    row(f"{name}-scratch-too-small", "DST_TOO_SMALL", tr(scap=TAIL - 1))
    row(f"{name}-no-members", "OK", tr([], image=None, scratch=None, scap=0, null_bases=True))
    row(f"{name}-no-elements", "OK", tr([("diff", 4, 0), ("planes", 2, 0)], ptrs=[0, 0], null_bases=True, image=None,
                                        scratch=None, scap=0))
    if name == "merge":
        row("merge-overlapping-destinations", "BAD_ARG", tr(ptrs=[A, A + 1992, 3 * A, 0, 5 * A]))
        row("merge-overlap-out-of-order", "BAD_ARG", tr(ptrs=[3 * A + 2, 2 * A, 3 * A, 0, 5 * A]))
        row("merge-destination-one-byte-into-its-base", "BAD_ARG",
            tr(ptrs=[A, 2 * A, 3 * A, 0, 5 * A], bptrs=[B + A, 0, 3 * A + 4, 0, 0]))
        row("merge-destination-two-bytes-before-its-base-end", "BAD_ARG",
            tr(ptrs=[A, 2 * A, 3 * A, 0, 5 * A], bptrs=[A + 1998, 0, B + 3 * A, 0, 0]))
        row("merge-destination-in-another-members-base", "BAD_ARG",
            tr(ptrs=[A, 2 * A, 3 * A, 0, 5 * A], bptrs=[B + A, 0, 5 * A + 12, 0, 0]))
        row("merge-plane-destination-equal-to-another-members-base", "BAD_ARG",
            tr(ptrs=[A, 2 * A, 3 * A, 0, 5 * A], bptrs=[5 * A, 0, B + 3 * A, 0, 0]))
        row("merge-in-place-destination-is-another-members-base-too", "BAD_ARG",
            tr(ptrs=[A, 2 * A, 3 * A, 0, 5 * A], bptrs=[A, 0, A + 100, 0, 0]))
        row("merge-swapped-bases", "BAD_ARG",
            tr([("diff", 2, 8), ("diff", 2, 8)], ptrs=[A, 2 * A], bptrs=[2 * A, A]))


# fsehip_vpack_compress(p, members, n, d_bases, d_scratch, scratch_cap, d_out, out_cap, d_out_len, d_result, stream)
def pc(p=None, specs=SMALL, ptrs=None, bptrs=None, null_bases=False, scratch=OK, scap=1 << 20, out=OK, ocap=1 << 20,
       olen=OK, res=OK, null_members=False, n=None):
    p = fparams() if p is None else p
    arr = None if null_members else members(specs, ptrs)
    bs = bases_of(specs, bptrs, null_bases)
    return lambda lib: lib.fsehip_vpack_compress(p, arr, len(specs) if n is None else n, bs, scratch, scap, out, ocap,
                                                 olen, res, None)


row("compress-null-p", "BAD_ARG", lambda lib: lib.fsehip_vpack_compress(None, members(SMALL), NS, base_array(SMALL), OK,
                                                                         1 << 20, OK, 1 << 20, OK, OK, None))
row("compress-null-members", "BAD_ARG", pc(null_members=True))
row("compress-null-scratch", "BAD_ARG", pc(scratch=None))
row("compress-null-out", "BAD_ARG", pc(out=None))
row("compress-null-out-len", "BAD_ARG", pc(olen=None))
row("compress-null-result", "BAD_ARG", pc(res=None))
row("compress-null-member-pointer", "BAD_ARG", pc(ptrs=[0, 2 * A, 3 * A, 0, 5 * A]))
row("compress-null-base", "BAD_ARG", pc(bptrs=[B + A, 0, 0, 0, 0]))
row("compress-base-odd-address", "BAD_ARG", pc(bptrs=[B + A + 1, 0, B, 0, 0]))
row("compress-null-bases-with-diff-members", "BAD_ARG", pc(null_bases=True))
row("compress-kind-0", "UNSUPPORTED", pc(specs=[("diff", 2, 9), (0, 2, 5)]))
row("compress-kind-3", "UNSUPPORTED", pc(specs=[(3, 2, 5)]))
row("compress-kind-5", "UNSUPPORTED", pc(specs=[(5, 2, 5)]))
row("compress-width-3", "UNSUPPORTED", pc(specs=[("diff", 3, 5)]))
row("compress-image-overflows", "UNSUPPORTED", pc(specs=[("diff", 8, 1 << 62)]))
row("compress-sum-overflows", "UNSUPPORTED", pc(specs=[("diff", 4, 1 << 61), ("diff", 4, 1 << 61)]))
row("compress-too-many-members", "UNSUPPORTED", pc(n=(1 << 20) + 1))
row("compress-block-limit", "UNSUPPORTED", pc(p=fparams(block=1 << 29)))
row("compress-two-blocks-of-1000", "BAD_ARG", pc(p=fparams(block=1000)))
row("compress-nstates-3", "BAD_ARG", pc(p=fparams(nstates=3)))
row("compress-interval-24", "BAD_ARG", pc(p=fparams(ckpt=24)))
row("compress-interval-8-one-state", "BAD_ARG", pc(p=fparams(ckpt=8, nstates=1)))
row("compress-member-odd-address", "BAD_ARG", pc(ptrs=[A + 1, 2 * A, 3 * A, 0, 5 * A]))
row("compress-scratch-misaligned", "BAD_ARG", pc(scratch=ODD8))
row("compress-scratch-too-small", "DST_TOO_SMALL", pc(scap=IMAGE + TAIL - 1))
row("compress-out-too-small", "DST_TOO_SMALL", pc(ocap=VR.bound(SMALL, 65536) - 1))
row("compress-misaligned-before-too-small", "BAD_ARG", pc(scratch=ODD8, ocap=0))


# fsehip_vpack_decompress(info, members, d_bases, inner, chunk, d_in, in_len, d_scratch, scratch_cap, d_block_status,
#                         d_result, stream)
def pd(pair=None, specs=SMALL, ptrs=None, bptrs=None, null_bases=False, d_in=OK, in_len=1 << 20, scratch=OK,
       scap=1 << 20, res=OK, null_members=False):
    info, inner = infos(specs) if pair is None else pair
    arr = None if null_members else members(specs, ptrs)
    bs = bases_of(specs, bptrs, null_bases)
    return lambda lib: lib.fsehip_vpack_decompress(info, arr, bs, inner, 0, d_in, in_len, scratch, scap, None, res, None)


# fsehip_vpack_decompress_members(info, members, d_bases, inner, chunk, d_in, in_len, sel, n_sel, d_scratch,
#                                 scratch_cap, d_member_status, d_result, stream)
def pm(sel=(0, 1, 2, 4), pair=None, specs=SMALL, ptrs=None, bptrs=None, null_bases=False, d_in=OK, in_len=1 << 20,
       scratch=OK, scap=1 << 20, res=OK, null_members=False, null_sel=False):
    info, inner = infos(specs) if pair is None else pair
    arr = None if null_members else members(specs, ptrs)
    bs = bases_of(specs, bptrs, null_bases)
    s = None if null_sel else (C.c_uint32 * max(len(sel), 1))(*sel)
    return lambda lib: lib.fsehip_vpack_decompress_members(info, arr, bs, inner, 0, d_in, in_len, s, len(sel), scratch,
                                                           scap, None, res, None)


P5 = [A, 2 * A, 3 * A, 0, 5 * A]
for name, f in (("decompress", pd), ("members", pm)):
    row(f"{name}-null-info", "BAD_ARG", f(pair=(None, infos()[1])))
    row(f"{name}-null-inner", "BAD_ARG", f(pair=(infos()[0], None)))
    row(f"{name}-null-members", "BAD_ARG", f(null_members=True))
    row(f"{name}-null-in", "BAD_ARG", f(d_in=None))
    row(f"{name}-null-result", "BAD_ARG", f(res=None))
    row(f"{name}-null-scratch", "BAD_ARG", f(scratch=None))
    row(f"{name}-in-len-short", "BAD_ARG", f(in_len=32 + 16 * NS + 31))
    row(f"{name}-version-2", "BAD_ARG", f(pair=infos(version=2)))
    row(f"{name}-kind-3", "UNSUPPORTED", f(specs=[(3, 2, 5)], pair=infos([("diff", 2, 5)])))
    row(f"{name}-kind-5", "UNSUPPORTED", f(specs=[(5, 2, 5)], pair=infos([("diff", 2, 5)])))
    row(f"{name}-width-3", "UNSUPPORTED", f(specs=[("diff", 3, 5)], pair=infos([("diff", 2, 5)])))
    row(f"{name}-too-many-members", "UNSUPPORTED", f(pair=infos(n_members=(1 << 20) + 1)))
    row(f"{name}-members-differ-from-the-table-count", "BAD_ARG", f(specs=[("diff", 2, 1001)] + SMALL[1:], pair=infos()))
    row(f"{name}-members-differ-from-the-table-width", "BAD_ARG", f(specs=[("diff", 4, 1000)] + SMALL[1:], pair=infos()))
    row(f"{name}-image_bytes-differs", "BAD_ARG", f(pair=infos(image=IMAGE + 16)))
    row(f"{name}-content_bytes-differs", "BAD_ARG", f(pair=infos(content=CONTENT + 1)))
    row(f"{name}-inner-n_total-off-by-16", "BAD_ARG", f(pair=infos(n_total=IMAGE + 16)))
    row(f"{name}-inner-n_blocks-wrong", "BAD_ARG", f(pair=infos(n_blocks=7)))
    row(f"{name}-scratch-misaligned", "BAD_ARG", f(scratch=ODD8))
    row(f"{name}-null-destination", "BAD_ARG", f(ptrs=[0, 2 * A, 3 * A, 0, 5 * A]))
    row(f"{name}-destination-odd-address", "BAD_ARG", f(ptrs=[A + 1, 2 * A, 3 * A, 0, 5 * A]))
    row(f"{name}-destination-4-of-8", "BAD_ARG", f(ptrs=[A, 2 * A + 4, 3 * A, 0, 5 * A]))
    row(f"{name}-overlapping-destinations", "BAD_ARG", f(ptrs=[A, A + 1992, 3 * A, 0, 5 * A]))
    row(f"{name}-null-base", "BAD_ARG", f(bptrs=[B + A, 0, 0, 0, 0]))
    row(f"{name}-base-odd-address", "BAD_ARG", f(bptrs=[B + A + 1, 0, B, 0, 0]))
    row(f"{name}-null-bases-with-diff-members", "BAD_ARG", f(null_bases=True))
    row(f"{name}-destination-one-byte-into-its-base", "BAD_ARG", f(ptrs=P5, bptrs=[B + A, 0, 3 * A + 4, 0, 0]))
    row(f"{name}-destination-overlaps-its-base-from-below", "BAD_ARG", f(ptrs=P5, bptrs=[A - 2, 0, B, 0, 0]))
    row(f"{name}-destination-in-another-members-base", "BAD_ARG", f(ptrs=P5, bptrs=[B + A, 0, 5 * A + 12, 0, 0]))
    row(f"{name}-delta-destination-in-a-diff-members-base", "BAD_ARG", f(ptrs=P5, bptrs=[2 * A - 1000, 0, B, 0, 0]))
    row(f"{name}-in-place-destination-is-another-members-base-too", "BAD_ARG", f(ptrs=P5, bptrs=[A, 0, A + 100, 0, 0]))
row("decompress-overlap-out-of-order", "BAD_ARG", pd(ptrs=[3 * A + 2, 2 * A, 3 * A, 0, 5 * A]))
row("decompress-scratch-too-small", "DST_TOO_SMALL", pd(scap=IMAGE + TAIL - 1))
row("decompress-misaligned-before-too-small", "BAD_ARG", pd(scratch=ODD8, scap=0))
row("members-null-selection", "BAD_ARG", pm(null_sel=True))
row("members-selection-out-of-range", "BAD_ARG", pm(sel=(0, NS)))
row("members-selection-twice", "BAD_ARG", pm(sel=(1, 0, 1)))
row("members-duplicate-before-too-small", "BAD_ARG", pm(sel=(2, 2), scap=0))
row("members-unselected-pointers-and-bases-are-not-looked-at", "DST_TOO_SMALL",
    pm(sel=(1, 2), ptrs=[1, 2 * A, 3 * A, 0, 5 * A], bptrs=[1, 0, B, 0, 0], scap=15))
row("members-an-unselected-members-base-may-overlap-a-destination", "DST_TOO_SMALL",
    pm(sel=(1, 2), ptrs=P5, bptrs=[2 * A, 0, B, 0, 0], scap=15))
row("members-null-bases-without-selected-diff-members", "DST_TOO_SMALL", pm(sel=(1, 3, 4), null_bases=True, scap=15))
row("members-null-bases-with-a-selected-diff-member", "BAD_ARG", pm(sel=(1, 2), null_bases=True, scap=15))
row("members-scratch-too-small", "DST_TOO_SMALL",
    pm(sel=(0, 1), scap=2 * 1008 + 8 * 32 + 48 + 2 * (104 + 8) + 32 + 16 * NS - 1))


@pytest.mark.parametrize("call,want", ROWS)
def test_argument_checks_come_before_any_device_use(call, want):
    assert st(call(_lib.load())) == want


def test_valid_calls_pass_the_checks():
    """The same calls with valid arguments reach the device check: NO_DEVICE
    without a GPU; with one they would run on fake pointers, so only then
    skipped.  Among them the in-place forms: a destination equal to its base."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run")
    lib = _lib.load()
    arr, bs = members(SMALL), base_array(SMALL)
    in_place = [A, 0, 3 * A, 0, 0]
    no_diff = [("planes", 2, 100), ("delta", 4, 7)]
    calls = [pc(), pd(), pm(), pm(sel=()), pm(sel=(3,)), pm(sel=(4, 3, 2, 1, 0)),
             pm(sel=(0, 1), scap=2 * 1008 + 8 * 32 + 48 + 2 * (104 + 8) + 32 + 16 * NS + 16),
             pd(ptrs=[A, A + 2000, 3 * A, 0, 5 * A]),  # adjacent destinations
             pd(bptrs=[A + 2000, 0, B, 0, 0]),  # a base adjacent to its destination
             pd(bptrs=in_place), pm(bptrs=in_place), pm(sel=(2, 0), bptrs=in_place),  # destination == base
             pd(bptrs=[A, 0, B, 0, 0]),  # one member in place, one not
             pd(bptrs=[B, 0, B, 0, 0]),  # two members against overlapping bases, read only
             pc(ptrs=P5, bptrs=[A, 0, 3 * A + 1, 0, 0]),  # the split side: sources and bases may overlap
             pc(specs=no_diff, null_bases=True), pd(specs=no_diff, pair=infos(no_diff), null_bases=True),
             pm(sel=(0, 1), specs=no_diff, pair=infos(no_diff), null_bases=True),
             pm(sel=(1, 4), null_bases=True),  # no selected diff member
             pc(specs=[], scap=32, null_bases=True), pd(specs=[], pair=infos([]), scap=32, null_bases=True),
             lambda lib: lib.fsehip_vpack_split(arr, NS, bs, OK, OK, 1 << 20, None),
             lambda lib: lib.fsehip_vpack_split(arr, NS, base_array(SMALL, in_place), OK, OK, TAIL, None),
             lambda lib: lib.fsehip_vpack_merge(arr, NS, bs, OK, OK, TAIL, None),
             lambda lib: lib.fsehip_vpack_merge(arr, NS, base_array(SMALL, in_place), OK, OK, TAIL, None)]
    for i, call in enumerate(calls):
        assert st(call(lib)) == "NO_DEVICE", i


def test_python_api_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from entropy_coders_amd import FseError, pack_info

    x = np.arange(100, dtype=np.int32)
    members_ = [("diff", x, x + 3), ("planes", np.arange(7, dtype=np.int8), None), ("delta", x.astype(np.int64), None)]
    head_ = pack_info(VR.build(members_, 4096, 128, 2))
    assert head_.container == "vpack"
    assert (head_.kinds, head_.elem_bytes, head_.n_elems) == (["diff", "planes", "delta"], [4, 1, 8], [100, 7, 100])
    assert head_.info.image_bytes == head_.inner.n_total == 4 * 112 + 16 + 8 * 112
    with pytest.raises(FseError) as e:
        pack_info(b"FSEV" + b"\0" * 60)
    assert e.value.code == "BAD_FRAME"
