"""The versioned pack's numpy restatement (tests/vpack_ref.py), no GPU: its
image round-trips every kind and width at the sizes round a group and a
restart, one image is checked by hand, its plane offsets are those of
fsehip_vpack_plane_offset, its parser rejects what the format rejects, a
versioned pack without diff members is the pack frame of the same list apart
from its magic, and the size conditions hold on the five member lists of
DESIGN.md section 5 "Versioned pack" (block 65536, 128-pair checkpoints, 2
states, torch generator seed 7).  The conditions are the issue's, with the
reference's own figures beside them:

  the versioned pack is at most 0.55 of the pack frame of the new tensors on
    every row (the reference's maximum: 0.495);
  it is at most the summed diff_ref.build frames of the members on every row
    (the reference's maximum: 0.964 of them);
  with every member equal to its base it is at most 1,024 bytes (429 to 709).
"""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import diff_ref as FR
import pack_ref as KR
import vpack_ref as VR

SIZES = [1, 15, 16, 17, 4095, 4096, 4097]
KINDS = ("planes", "delta", "diff")


def c_members(specs):
    from entropy_coders_amd import _lib

    arr = (_lib.PackMember * max(len(specs), 1))()
    for m, (kind, w, n) in enumerate(specs):
        arr[m] = _lib.PackMember(None, n, w, VR.KIND[kind])
    return arr


def test_the_library_has_the_versioned_pack_calls():
    from entropy_coders_amd import _lib

    assert _lib.KIND_VPACK == 6
    for name in ("image_bytes", "bound", "scratch_bytes", "members_scratch_bytes", "plane_offset", "read_header",
                 "read_members", "write_header", "split", "merge", "compress", "decompress", "decompress_members"):
        assert hasattr(_lib.load(), "fsehip_vpack_" + name), name


def test_no_members_and_one_empty_member():
    buf = VR.build([], 65536, 128, 2)
    assert len(buf) == 64 and buf[:4] == b"FSEV" and VR.decode(buf) == ([], [])
    z = np.zeros(0, np.int32)
    buf = VR.build([("diff", z, z)], 65536, 128, 2)
    specs, raws = VR.decode(buf, [z])
    assert len(buf) == 80 and specs == [("diff", 4, 0)] and raws[0].size == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", VR.WIDTHS)
def test_image_round_trips(kind, w):
    rng = np.random.default_rng(0x7AC4 + w)
    draw = lambda n: rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])  # noqa: E731
    members = [(kind, draw(n), draw(n)) for n in SIZES]
    members.insert(3, (kind, np.zeros(0, DR.UINT[w]), np.zeros(0, DR.UINT[w])))
    specs = VR.specs_of(members)
    img = VR.image(members)
    assert img.size == VR.sums(specs)[0] == sum(w * VR.stride_of(n) for n in SIZES)
    for (_, a, _), raw in zip(members, VR.unimage(img, specs, [b for _, _, b in members])):
        assert raw.tobytes() == a.tobytes()
    for (_, _, n), off in zip(specs, VR.plane_offsets(specs)):
        for k in range(w):
            assert off[k] % 16 == 0 and not img[off[k] + n: off[k] + VR.stride_of(n)].any(), "pads are zero"
    if kind == "diff":  # another base: other values
        other = VR.unimage(img, specs, [b + np.ones(1, b.dtype) for _, _, b in members])
        assert all(o.tobytes() != a.tobytes() for (_, a, _), o in zip(members, other) if a.size)


def test_an_image_by_hand():
    """Three members: a diff member of three 2-byte elements, a plane member
    of two bytes, a delta member of two 2-byte elements.  zigzag(x - b): 0 ->
    0, -1 -> 1, +1 -> 2, 0x0102 - 0x0001 = 0x0101 -> 0x0202; the differences
    wrap mod 2^16.  Segment 0 holds the top bytes of all three in member
    order, segment 1 the low bytes of the two 2-byte members."""
    x = np.array([5, 0, 0x0102], np.uint16)
    b = np.array([5, 1, 0x0001], np.uint16)
    p = np.array([7, 9], np.uint8)
    d = np.array([3, 1], np.uint16)  # deltas 3, -2 -> zigzag 6, 3
    img = VR.image([("diff", x, b), ("planes", p, None), ("delta", d, None)])
    assert img.size == 16 * 5
    want = np.zeros(80, np.uint8)
    want[0:3] = [0, 0, 2]      # diff member, byte 1
    want[16:18] = [7, 9]       # the plane member's bytes
    want[32:34] = [0, 0]       # delta member, byte 1
    want[48:51] = [0, 1, 2]    # diff member, byte 0
    want[64:66] = [6, 3]       # delta member, byte 0
    assert img.tobytes() == want.tobytes()
    wrap = VR.image([("diff", np.array([0, 0xFFFF], np.uint16), np.array([0xFFFF, 0], np.uint16))])
    assert wrap[16:18].tolist() == [2, 1] and not wrap[:16].any()  # +1 and -1 mod 2^16


def mixed_members(rng, sizes=SIZES):
    """Every width at every size, the three kinds alternating."""
    members = []
    for i, n in enumerate(sizes):
        for j, w in enumerate(VR.WIDTHS):
            kind = KINDS[(i + j) % 3]
            a = np.cumsum(rng.integers(-3, 40, n)).astype(DR.UINT[w])
            members.append((kind, a, (a + rng.integers(-2, 3, n).astype(DR.UINT[w])) if kind == "diff" else None))
    return members


def test_plane_offsets_are_the_librarys():
    from entropy_coders_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(0x0FF6)
    for trial in range(20):
        n = int(rng.integers(0, 40))
        specs = [(KINDS[int(rng.integers(3))], int(rng.choice(VR.WIDTHS)), int(rng.integers(0, 5000))) for _ in range(n)]
        arr = c_members(specs)
        image, content = VR.sums(specs)
        assert lib.fsehip_vpack_image_bytes(arr, n) == image
        assert lib.fsehip_vpack_bound(arr, n, 65536) == VR.bound(specs, 65536)
        for m, off in enumerate(VR.plane_offsets(specs)):
            for k, want in enumerate(off):
                assert lib.fsehip_vpack_plane_offset(arr, n, m, k) == want, (trial, m, k)
            assert lib.fsehip_vpack_plane_offset(arr, n, m, specs[m][1]) == (1 << 64) - 1
        assert lib.fsehip_vpack_plane_offset(arr, n, n, 0) == (1 << 64) - 1
        head = np.zeros(32 + 16 * n, np.uint8)
        assert lib.fsehip_vpack_write_header(arr, n, head.ctypes.data_as(C.c_void_p)) == 0
        assert head.tobytes() == VR.header(specs)


@pytest.mark.parametrize("nstates,ckpt", [(2, 128), (1, 0)])
def test_frames_round_trip(nstates, ckpt):
    members = mixed_members(np.random.default_rng(0xF4A3F))
    buf = VR.build(members, 4096, ckpt, nstates)
    specs, raws = VR.decode(buf, [b for _, _, b in members])
    assert specs == VR.specs_of(members) and len(buf) <= VR.bound(specs, 4096)
    for (_, a, _), raw in zip(members, raws):
        assert raw.tobytes() == a.tobytes()


def test_parse_rejects_what_the_format_rejects():
    members = mixed_members(np.random.default_rng(1), [17])
    good = VR.build(members, 4096, 0, 2)
    assert [k for k, _, _ in VR.parse(good)[0]] == ["planes", "delta", "diff", "planes"]
    for at, val in ((3, ord("M")), (3, ord("B")), (4, 2), (5, 1), (12, 1), (32, 0), (32, 3), (32, 5), (33, 3), (34, 1),
                    (16, good[16] ^ 16), (24, good[24] ^ 1), (40, good[40] ^ 1)):
        bad = bytearray(good)
        bad[at] = val
        with pytest.raises(VR.PackError):
            VR.parse(bad)
    with pytest.raises(VR.PackError):
        VR.parse(good[: 32 + 16 * len(members) + 31])
    with pytest.raises(KR.PackError):
        KR.parse(good)  # and the pack frame's parser refuses this magic


def test_without_diff_members_only_the_magic_differs():
    members = [(k, a) for k, a in KR.normalise([(k, a) for k, a, _ in mixed_members(np.random.default_rng(2))
                                                if k != "diff"])]
    for block, ckpt, nstates in ((4096, 128, 2), (65536, 0, 1)):
        pack = KR.build(members, block, ckpt, nstates)
        vpack = VR.build([(k, a, None) for k, a in members], block, ckpt, nstates)
        assert pack[:4] == b"FSEM" and vpack[:4] == b"FSEV" and vpack[4:] == pack[4:]


# ---------------------------------------------------------------- the size conditions
@pytest.fixture(scope="module")
def rows():
    return VR.table_rows()


ROW_NAMES = ["40 x 256 bf16, step 0.0001", "24 x 1024 bf16 + 8 x 300 fp32, step 0.0001",
             "24 x 1024 bf16 + 8 x 300 fp32, step 1e-05", "4 x 70000 bf16 + 16 x 100 bf16, step 0.0001",
             "4 x 70000 bf16 + 16 x 100 bf16, step 1e-05"]


def test_the_rows_are_the_five_lists(rows):
    assert list(rows) == ROW_NAMES


@pytest.mark.parametrize("name", ROW_NAMES)
def test_size_conditions(rows, name):
    new, base = rows[name]
    vpack = len(VR.build(new, 65536, 128, 2, bases=base))
    pack = len(KR.build(new, 65536, 128, 2))
    loop = sum(len(FR.build(a, b, 65536, 128, 2)) for a, b in zip(new, base))
    same = len(VR.build(base, 65536, 128, 2, bases=base))
    print(f"\n[vpack] {name}: versioned pack {vpack}, pack frame {pack} ({vpack / pack:.3f}), "
          f"loop of diff frames {loop} ({vpack / loop:.3f}), every member equal to its base {same}")
    assert vpack <= 0.55 * pack
    assert vpack <= loop
    assert same <= 1024
