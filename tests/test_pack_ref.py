"""The pack frame's numpy restatement (tests/pack_ref.py), no GPU: it
round-trips empty lists, empty members and every width of both kinds at the
sizes round a group and a restart; its plane offsets are those of
fsehip_pack_plane_offset; and on lists of small tensors the reference-built
pack is smaller than the reference-built plane frames of the same tensors
(DESIGN.md section 5 "Pack" has the table: 0.81 and 0.91 measured; the bounds
leave room for another seed), while one large member costs its own plane frame
and a few head bytes."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import pack_ref as KR
import planes_ref as PR

SIZES = [1, 15, 16, 17, 4095, 4096, 4097]


def c_members(specs):
    from entropy_coders_amd import _lib

    arr = (_lib.PackMember * max(len(specs), 1))()
    for m, (kind, w, n) in enumerate(specs):
        arr[m] = _lib.PackMember(None, n, w, KR.KIND[kind])
    return arr


def test_the_library_has_the_pack_calls():
    from entropy_coders_amd import BlockCodec, _lib, pack_compress, pack_decompress, pack_info  # noqa: F401

    assert _lib.KIND_PACK == 5 and _lib.PACK_MAX_MEMBERS == KR.MAX_MEMBERS
    assert hasattr(_lib.load(), "fsehip_pack_compress") and hasattr(BlockCodec, "compress_pack")
    assert hasattr(BlockCodec, "decompress_pack_members")


def test_no_members_and_one_empty_member():
    buf = KR.build([], 65536, 128, 2)
    assert len(buf) == 64 and KR.decode(buf) == ([], [])
    buf = KR.build([("delta", np.zeros(0, np.int32))], 65536, 128, 2)
    specs, raws = KR.decode(buf)
    assert len(buf) == 80 and specs == [("delta", 4, 0)] and raws[0].size == 0


@pytest.mark.parametrize("kind", ["planes", "delta"])
@pytest.mark.parametrize("w", KR.WIDTHS)
def test_image_round_trips(kind, w):
    rng = np.random.default_rng(0x9AC4 + w)
    members = [(kind, rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])) for n in SIZES]
    members.insert(3, (kind, np.zeros(0, DR.UINT[w])))
    specs = KR.specs_of(members)
    img = KR.image(members)
    assert img.size == KR.sums(specs)[0] == sum(w * KR.stride_of(n) for n in SIZES)
    for (_, a), raw in zip(members, KR.unimage(img, specs)):
        assert raw.tobytes() == a.tobytes()
    for (_, _, n), off in zip(specs, KR.plane_offsets(specs)):
        for k in range(w):
            assert off[k] % 16 == 0 and not img[off[k] + n: off[k] + KR.stride_of(n)].any(), "pads are zero"


def mixed_members(rng, sizes=SIZES):
    members = []
    for i, n in enumerate(sizes):
        for w in KR.WIDTHS:
            kind = ("planes", "delta")[(i + w) % 2]
            members.append((kind, np.cumsum(rng.integers(-3, 40, n)).astype(DR.UINT[w])))
    return members


def test_image_is_plane_major_from_the_top_byte():
    """One member alone: a plane member's image is the plane image with its
    planes in reverse order, a delta member's the delta image likewise."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 31, 100).astype(np.int32)
    assert KR.image([("planes", a)]).reshape(4, -1)[::-1].tobytes() == PR.image(PR.raw_bytes(a), 4).tobytes()
    assert KR.image([("delta", a)]).reshape(4, -1)[::-1].tobytes() == DR.image(PR.raw_bytes(a), 4).tobytes()
    # two members: the top bytes of both first
    b = rng.integers(0, 1 << 15, 20).astype(np.int16)
    img = KR.image([("planes", a), ("planes", b)])
    assert img[:112].tobytes() == PR.image(PR.raw_bytes(a), 4).reshape(4, -1)[3].tobytes()
    assert img[112:144].tobytes() == PR.image(PR.raw_bytes(b), 2).reshape(2, -1)[1].tobytes()


def test_plane_offsets_are_the_librarys():
    from entropy_coders_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(0x0FF5)
    for trial in range(20):
        n = int(rng.integers(0, 40))
        specs = [(("planes", "delta")[int(rng.integers(2))], int(rng.choice(KR.WIDTHS)), int(rng.integers(0, 5000)))
                 for _ in range(n)]
        arr = c_members(specs)
        image, content = KR.sums(specs)
        assert lib.fsehip_pack_image_bytes(arr, n) == image
        assert lib.fsehip_pack_bound(arr, n, 65536) == KR.bound(specs, 65536)
        for m, off in enumerate(KR.plane_offsets(specs)):
            for k, want in enumerate(off):
                assert lib.fsehip_pack_plane_offset(arr, n, m, k) == want, (trial, m, k)
            assert lib.fsehip_pack_plane_offset(arr, n, m, specs[m][1]) == (1 << 64) - 1
        assert lib.fsehip_pack_plane_offset(arr, n, n, 0) == (1 << 64) - 1
        head = np.zeros(32 + 16 * n, np.uint8)
        assert lib.fsehip_pack_write_header(arr, n, head.ctypes.data_as(C.c_void_p)) == 0
        assert head.tobytes() == KR.header(specs)


@pytest.mark.parametrize("nstates,ckpt", [(2, 128), (1, 0)])
def test_frames_round_trip(nstates, ckpt):
    members = mixed_members(np.random.default_rng(0xF4A3E))
    buf = KR.build(members, 4096, ckpt, nstates)
    specs, raws = KR.decode(buf)
    assert specs == KR.specs_of(members) and len(buf) <= KR.bound(specs, 4096)
    for (_, a), raw in zip(members, raws):
        assert raw.tobytes() == a.tobytes()


def test_parse_rejects_what_the_format_rejects():
    members = mixed_members(np.random.default_rng(1), [17])
    good = KR.build(members, 4096, 0, 2)
    KR.parse(good)
    for at, val in ((3, ord("P")), (4, 2), (5, 1), (12, 1), (32, 3), (33, 3), (34, 1), (16, good[16] ^ 16),
                    (24, good[24] ^ 1), (40, good[40] ^ 1)):
        bad = bytearray(good)
        bad[at] = val
        with pytest.raises(KR.PackError):
            KR.parse(bad)
    with pytest.raises(KR.PackError):
        KR.parse(good[: 32 + 16 * len(members) + 31])


@pytest.fixture(scope="module")
def rows():
    return KR.table_rows()


@pytest.mark.parametrize("name,limit", [("40 x 256 bf16", 0.90), ("24 x 1024 bf16 + 8 x 300 fp32", 0.97)])
def test_size_condition_on_small_tensors(rows, name, limit):
    arrays = rows[name]
    raw = sum(a.nbytes for a in arrays)
    pack = len(KR.build(arrays, 65536, 64, 2))
    separate = sum(len(PR.build(a, 65536, 64, 2)) for a in arrays)
    print(f"\n[pack] {name}: raw {raw}, separate plane frames {separate} ({separate / raw:.3f}), "
          f"pack {pack} ({pack / raw:.3f}), pack / separate {pack / separate:.3f}")
    assert pack <= limit * separate


def test_large_members_lose_nothing(rows):
    arrays = rows["4 x 70000 bf16 + 16 x 100 bf16"]
    pack = len(KR.build(arrays, 65536, 64, 2))
    separate = sum(len(PR.build(a, 65536, 64, 2)) for a in arrays)
    print(f"\n[pack] 4 x 70000 + 16 x 100 bf16: separate {separate}, pack {pack}, ratio {pack / separate:.3f}")
    assert pack <= separate


def test_one_large_member_costs_its_plane_frame():
    import torch

    a = KR.bf16(torch.randn(65541, generator=torch.Generator().manual_seed(3)).numpy())
    pack, planes = len(KR.build([a], 65536, 64, 2)), len(PR.build(a, 65536, 64, 2))
    print(f"\n[pack] one member of 65,541 bf16: pack {pack}, plane frame {planes}")
    assert abs(pack - planes) <= 64
