"""The versioned pack on the GPU (include/fsehip.h section 2k): the split and
merge kernels alone against tests/vpack_ref.py with the three kinds
alternating tile by tile, members and bases carved from arenas at element
alignment only with poison between them, a member whose tiles outnumber the
capped grid, wrapping data, container bytes against the reference at both
formats, reference-built packs decoded on the device, 3,000 members, the
in-place decode, selected members with only their bases given, damaged
buffers, the documented hazard of another base, the host forms and stream
order.  Expected bytes never come from the code under test; outputs sit
between the guard bands of tests/test_gpu_guard_bands.py or inside a poisoned
arena compared whole."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import frame_ref as R
import vpack_ref as VR
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_pack import (GUARD, SRC_POISON, Arena, codec_for, dev_u8, device_sidecars, lib, member_data, stream_of,
                           torch_cuda, torch_int)  # noqa: F401  (torch_cuda: the fixture)
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
BAD_FRAME = R.BAD_FRAME
BLOCK, CKPT = 4096, 128
KINDS = ("diff", "delta", "planes")
# in list order: a delta tile between two diff tiles and one between two planes tiles; the six rotations put
# every kind at every size and width
CYCLE = ("diff", "delta", "diff", "planes", "delta", "planes")
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8193]
# element alignment only: odd addresses at w = 1, 2 mod 4 at w = 2, 4 mod 8 at w = 4, 8 mod 16 at w = 8
OFF = {1: 1, 2: 2, 4: 4, 8: 8}


# ---------------------------------------------------------------- host data
def base_for(rng, a):
    """A base for the elements a: the tensor a few units of the last place earlier; every fourth unrelated."""
    w = a.dtype.itemsize
    if rng.integers(4) == 0:
        return rng.integers(0, 256, a.size * w, dtype=np.uint8).view(DR.UINT[w])
    return (a.astype(DR.UINT[w]) - rng.integers(-3, 4, a.size).astype(DR.UINT[w])).astype(DR.UINT[w])


def mixed_members(seed, sizes=SIZES, flip=0, widths=VR.WIDTHS):
    """All four widths at every size, (kind, array, base | None), the kinds following CYCLE rotated by `flip`."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        for w in widths:
            kind = CYCLE[(len(out) + flip) % 6]
            a = member_data(rng, "delta" if kind == "delta" else "planes", w, n).view(DR.UINT[w])
            out.append((kind, a, base_for(rng, a) if kind == "diff" else None))
    return out


def raws_of(members):
    return [VR.raw_bytes(a) for _, a, _ in members]


def base_raws_of(members):
    return [VR.raw_bytes(b) if b is not None else np.zeros(0, np.uint8) for _, _, b in members]


def offs_of(specs):
    return [OFF[w] for _, w, _ in specs]


class VArena(Arena):
    """tests/test_gpu_pack.py's arena with the versioned pack's kind numbers."""

    def members(self, only=None):
        from entropy_coders_amd import _lib

        arr = (_lib.PackMember * max(len(self.specs), 1))()
        for m, ((kind, w, n), p) in enumerate(zip(self.specs, self.pos)):
            keep = n and (only is None or m in only)
            arr[m] = _lib.PackMember(self.dev.data_ptr() + p if keep else None, n, w, VR.KIND[kind])
        return arr

    def pointers(self, only=None):
        """The host array of base pointers: the diff members' places in this arena, null everywhere else."""
        arr = (C.c_void_p * max(len(self.specs), 1))()
        for m, ((kind, _, n), p) in enumerate(zip(self.specs, self.pos)):
            if kind == "diff" and n and (only is None or m in only):
                arr[m] = self.dev.data_ptr() + p
        return arr


def base_arena(torch, members, offs=None):
    """The bases in an arena of their own, exact size between poison; planes and delta members get no bytes."""
    specs = [(k, w, n if k == "diff" else 0) for k, w, n in VR.specs_of(members)]
    return VArena(torch, specs, SRC_POISON, offs, base_raws_of(members))


def transform_scratch(torch, arr, n):
    L = lib()
    extra = L.fsehip_vpack_scratch_bytes(arr, n) - L.fsehip_vpack_image_bytes(arr, n)
    return g8(torch, max(extra, 16))


def split_on_device(torch, members, offs=None):
    """fsehip_vpack_split of members and bases in two source arenas: the image; guards and sources asserted."""
    specs = VR.specs_of(members)
    arena, bases = VArena(torch, specs, SRC_POISON, offs, raws_of(members)), base_arena(torch, members, offs)
    arr, n = arena.members(), len(specs)
    iw, img = g8(torch, VR.sums(specs)[0])
    sw, scratch = transform_scratch(torch, arr, n)
    rc = lib().fsehip_vpack_split(arr, n, bases.pointers(), ptr(img), ptr(scratch), scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(iw, img, A5, "split image")
    assert_guards(sw, scratch, A5, "split scratch")
    same(arena.dev.cpu().numpy(), arena.host, "the split's source arena")
    same(bases.dev.cpu().numpy(), bases.host, "the split's base arena")
    return img.cpu().numpy()


def merge_on_device(torch, members, image, offs=None):
    """fsehip_vpack_merge of a host image into a poisoned arena, compared whole; every base unchanged."""
    specs = VR.specs_of(members)
    arena, bases = VArena(torch, specs, A5, offs), base_arena(torch, members, offs)
    arr, n = arena.members(), len(specs)
    dimg = dev_u8(torch, image) if len(image) else torch.empty(16, dtype=torch.uint8, device="cuda")
    sw, scratch = transform_scratch(torch, arr, n)
    rc = lib().fsehip_vpack_merge(arr, n, bases.pointers(), ptr(dimg), ptr(scratch), scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(sw, scratch, A5, "merge scratch")
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the merge's destination arena")
    same(bases.dev.cpu().numpy(), bases.host, "the merge's base arena: an out-of-place decode leaves every base alone")


def merge_in_place(torch, members, image, offs=None):
    """fsehip_vpack_merge with every diff member's destination its base itself: one arena that holds the bases
    (poison where a planes or delta member goes) becomes the new tensors, poison everywhere else."""
    specs = VR.specs_of(members)
    arena = VArena(torch, specs, A5, offs)
    for (kind, _, _), p, raw in zip(specs, arena.pos, base_raws_of(members)):
        if kind == "diff":
            arena.host[p: p + raw.size] = raw
    arena.dev = torch.from_numpy(arena.host).cuda()
    arr, n = arena.members(), len(specs)
    dimg = dev_u8(torch, image)
    sw, scratch = transform_scratch(torch, arr, n)
    rc = lib().fsehip_vpack_merge(arr, n, arena.pointers(), ptr(dimg), ptr(scratch), scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(sw, scratch, A5, "merge scratch")
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the arena after the in-place merge")


# ---------------------------------------------------------------- split and merge alone
@gpu
@pytest.mark.parametrize("flip", range(6))
def test_split_and_merge_against_vpack_ref(torch_cuda, flip):
    members = mixed_members(0x7AC4 + flip, flip=flip)
    specs = VR.specs_of(members)
    kinds = [k for k, _, n in specs if n]
    assert any(kinds[i: i + 3] == ["diff", "delta", "diff"] for i in range(len(kinds)))  # the set flip
    want = VR.image(members)
    offs = offs_of(specs)
    same(split_on_device(torch_cuda, members, offs), want, "versioned pack image")  # pads included
    merge_on_device(torch_cuda, members, want, offs)
    merge_in_place(torch_cuda, members, want, offs)


@gpu
def test_a_delta_tile_between_two_diff_tiles(torch_cuda):
    """diff, delta, diff, delta, diff with whole tiles each, then a planes member: every delta tile flips the LDS
    set, no other tile does."""
    rng = np.random.default_rng(0x5E7)
    members = []
    for i, n in enumerate((4096, 8192, 4097, 4096, 8193, 100)):
        kind = "planes" if i == 5 else ("diff", "delta")[i % 2]
        a = member_data(rng, "delta" if kind == "delta" else "planes", 8 if i % 3 == 0 else 2, n)
        a = a.view(DR.UINT[a.dtype.itemsize])
        members.append((kind, a, base_for(rng, a) if kind == "diff" else None))
    want = VR.image(members)
    offs = offs_of(VR.specs_of(members))
    same(split_on_device(torch_cuda, members, offs), want, "image")
    merge_on_device(torch_cuda, members, want, offs)


@gpu
def test_split_and_merge_of_nothing(torch_cuda):
    L = lib()
    z4, z1 = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    for members in ([], [("diff", z4, z4), ("planes", z1, None), ("delta", z4, None)]):
        assert split_on_device(torch_cuda, members).size == 0
        merge_on_device(torch_cuda, members, np.zeros(0, np.uint8))
    assert L.fsehip_vpack_split(None, 0, None, None, None, 0, stream_of(torch_cuda)) == 0
    assert L.fsehip_vpack_merge(None, 0, None, None, None, 0, stream_of(torch_cuda)) == 0


@gpu
def test_more_tiles_than_the_capped_grid(torch_cuda):
    """One diff member of 2,049 x 4,096 + 5 one-byte elements, 2,050 tiles: the tile loop's second pass runs past
    the 2,048 workgroups of the capped grid; the delta member behind it starts at tile 2,050."""
    rng = np.random.default_rng(0x2049)
    n = 2049 * 4096 + 5
    a = rng.integers(0, 256, n, dtype=np.uint8)
    b = (a - rng.integers(-2, 3, n).astype(np.uint8)).astype(np.uint8)
    d = np.cumsum(rng.integers(-3, 40, 5000)).astype(np.uint16)
    members = [("diff", a, b), ("delta", d, None)]
    want = VR.image(members)
    offs = [1, 2]
    same(split_on_device(torch_cuda, members, offs), want, "image of 2,050 diff tiles and a delta member")
    merge_on_device(torch_cuda, members, want, offs)
    merge_in_place(torch_cuda, members, want, offs)


@gpu
@pytest.mark.parametrize("w", VR.WIDTHS)
def test_wrapping_data(torch_cuda, w):
    """x = 0 against b = 2^(8 w) - 1 and the reverse, the carry across the 64-bit halves, x == b: the difference
    wraps mod 2^(8 w) both ways."""
    top = (1 << (8 * w)) - 1
    u = DR.UINT[w]
    x = np.array([0, top, 0, top, 1 << (8 * w - 1), top >> 1, 5, top, 0, 1 << (4 * w), (1 << (4 * w)) - 1, 0x80, 0x7F,
                  top - 1, 1, 0, 3] * 3, dtype=np.uint64).astype(u)
    b = np.array([top, 0, 0, top, top >> 1, 1 << (8 * w - 1), 5, 1, top - 1, (1 << (4 * w)) - 1, 1 << (4 * w), 0x7F,
                  0x80, 1, top - 1, top, 3] * 3, dtype=np.uint64).astype(u)
    members = [("diff", x, b), ("diff", b.copy(), b.copy()), ("delta", x, None), ("diff", b, x)]
    want = VR.image(members)
    assert want.any() and not VR.image([("diff", b, b)]).any()  # x == b is the zero image
    offs = offs_of(VR.specs_of(members))
    same(split_on_device(torch_cuda, members, offs), want, f"wrapping image w={w}")
    merge_on_device(torch_cuda, members, want, offs)
    merge_in_place(torch_cuda, members, want, offs)


# ---------------------------------------------------------------- container bytes
def device_tensors(torch, arrays):
    return [None if a is None else
            torch.from_numpy(a.view(np.dtype(f"i{a.itemsize}") if a.itemsize > 1 else np.uint8).copy()).cuda()
            for a in arrays]


def on_device(torch, members):
    """(tensors, kinds, base tensors) of a member list."""
    return (device_tensors(torch, [a for _, a, _ in members]), [k for k, _, _ in members],
            device_tensors(torch, [b for _, _, b in members]))


def reference_vpack(torch, codec, members):
    img = VR.image(members)
    return VR.build(members, codec.block_size, codec.ckpt_interval, codec.nstates, codec.table_log,
                    sidecars=device_sidecars(torch, codec, img))


BYTES_MEMBERS = [0, 1, 17, 300, 4097, 20011]


@gpu
@pytest.mark.parametrize("nstates,ckpt,block,table_log,offset", [(2, 128, 65536, 0, 0), (2, 0, 1040, 0, 0),
                                                                 (1, 128, 1040, 0, 0), (1, 0, 65536, 0, 0),
                                                                 (2, 128, 65536, 13, 0), (2, 128, 1040, 0, 1)])
def test_bytes_against_vpack_ref(torch_cuda, nstates, ckpt, block, table_log, offset):
    """Device packs equal the reference's byte for byte, at an odd buffer address too (guard bands round every
    output; only out_len bytes are written), and decode on both sides."""
    torch = torch_cuda
    codec = codec_for(block, ckpt, nstates, table_log)
    members = mixed_members(0xB17E6 + block + nstates, BYTES_MEMBERS)
    xs, kinds, bs = on_device(torch, members)
    want = reference_vpack(torch, codec, members)
    names, barr = codec.pack_bases(xs, bs, kinds)
    arr, n = codec.pack_members(xs, names, versioned=True), len(xs)
    cap = codec.pack_bound(arr, n, versioned=True)
    assert cap == VR.bound(VR.specs_of(members), block) and len(want) <= cap
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.pack_scratch_bytes(arr, n, versioned=True))
    codec.compress_pack_into(arr, n, scratch, out, out_len, res, bases=barr)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0, (out_len.tolist(), len(want), res.tolist())
    same(out[: len(want)].cpu().numpy(), np.frombuffer(want, np.uint8), "versioned pack bytes")
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the pack"
    assert R.FSE in R.types_of(want[32 + 16 * n:])
    outs, st = codec_for().decompress_pack(out[: len(want)], [x.dtype for x in xs], bases=bs)
    assert not bool(st.any()) and all(torch.equal(o, x) for o, x in zip(outs, xs))
    assert all(torch.equal(b, device_tensors(torch, [m[2]])[0]) for b, m in zip(bs, members) if b is not None)
    specs, raws = VR.decode(bytes(out[: len(want)].cpu().numpy()), [b for _, _, b in members])
    assert specs == VR.specs_of(members) and all(r.tobytes() == a.tobytes() for r, (_, a, _) in zip(raws, members))


@gpu
def test_empty_and_diffless_packs(torch_cuda):
    """No members; members without elements; and a list with no diff member, whose versioned pack is the pack
    frame of the same list apart from its magic."""
    torch = torch_cuda
    codec = codec_for()
    buf = codec.compress_pack([], bases=[])
    assert bytes(buf.cpu().numpy()) == VR.build([], BLOCK, CKPT, 2) and buf.numel() == 64
    outs, st = codec.decompress_pack(buf, torch.int16)
    assert outs == [] and st.numel() == 0 and codec.pack_info(buf).container == "vpack"
    e4, e1 = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda")
    buf = codec.compress_pack([e4, e1], bases=[e4.clone(), None])
    z4, z1 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    assert bytes(buf.cpu().numpy()) == VR.build([("diff", z4, z4), ("planes", z1, None)], BLOCK, CKPT, 2)
    outs, st = codec.decompress_pack(buf, [torch.int32, torch.uint8], bases=[e4, None])
    assert [o.numel() for o in outs] == [0, 0]
    outs, mst = codec.decompress_pack_members(buf, [0], torch.int32, bases=[e4])
    assert outs[0].numel() == 0 and mst.tolist() == [0]
    members = [(k, a, None) for k, a, _ in mixed_members(0xD1FF, [17, 4097, 300]) if k != "diff"]
    xs, kinds, _ = on_device(torch, members)
    vpack = codec.compress_pack(xs, kinds, bases=[None] * len(xs))
    pack = codec.compress_pack(xs, kinds)
    assert bytes(vpack[:4].cpu().numpy()) == b"FSEV" and bytes(pack[:4].cpu().numpy()) == b"FSEM"
    assert torch.equal(vpack[4:], pack[4:])
    same(vpack.cpu().numpy(), np.frombuffer(reference_vpack(torch, codec, members), np.uint8), "diffless versioned pack")
    outs, st = codec.decompress_pack(vpack, [x.dtype for x in xs])  # no diff members: no bases needed
    assert not bool(st.any()) and all(torch.equal(o, x) for o, x in zip(outs, xs))


@gpu
def test_many_members(torch_cuda):
    """3,000 members of 1 to 40 elements with mixed kinds and bases: descriptors and base pointers outgrow one
    staging buffer; bytes against the reference, the whole decode into one poisoned arena out of place, and 500
    scattered members with only their own bases given."""
    torch = torch_cuda
    rng = np.random.default_rng(0x3001)
    members = []
    for m in range(3000):
        kind, w = KINDS[int(rng.integers(3))], int(rng.choice(VR.WIDTHS))
        a = member_data(rng, "delta" if kind == "delta" else "planes", w, int(rng.integers(1, 41))).view(DR.UINT[w])
        members.append((kind, a, base_for(rng, a) if kind == "diff" else None))
    codec = codec_for(65536, 128, 2)
    xs, kinds, bs = on_device(torch, members)
    buf = codec.compress_pack(xs, kinds, bases=bs)
    want = reference_vpack(torch, codec, members)
    same(buf.cpu().numpy(), np.frombuffer(want, np.uint8), "versioned pack of 3,000 members")
    specs, raws = VR.specs_of(members), raws_of(members)
    head = codec.pack_info(buf)
    assert head.container == "vpack"
    assert (head.kinds, head.elem_bytes, head.n_elems) == ([k for k, _, _ in specs], [w for _, w, _ in specs],
                                                           [n for _, _, n in specs])
    offs = [int(rng.integers(16 // w)) * w for _, w, _ in specs]
    arena, bases = VArena(torch, specs, A5, offs), base_arena(torch, members, offs)
    L = lib()
    sw, scratch = g8(torch, codec.pack_scratch_bytes(head.members, 3000, versioned=True))
    bw, bst = g32(torch, head.inner.n_blocks)
    rw, res = g32(torch, 2)
    rc = L.fsehip_vpack_decompress(C.byref(head.info), arena.members(), bases.pointers(), C.byref(head.inner), 0,
                                   ptr(buf), buf.numel(), ptr(scratch), scratch.numel(), ptr(bst), ptr(res),
                                   stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (bw, bst, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    assert res.tolist() == [0, 0] and not bool(bst.any())
    same(arena.dev.cpu().numpy(), arena.expect(raws), "3,000 members decoded")
    same(bases.dev.cpu().numpy(), bases.host, "the bases after the decode")
    pick = sorted(int(i) for i in rng.choice(3000, 500, replace=False))[::-1]
    outs, mst = codec.decompress_pack_members(buf, pick, [torch_int(torch, specs[m][1]) for m in pick],
                                              bases={m: bs[m] for m in pick if bs[m] is not None})
    assert not bool(mst.any())
    for o, m in zip(outs, pick):
        assert bytes(o.view(torch.uint8).cpu().numpy()) == raws[m].tobytes(), m


# ---------------------------------------------------------------- reference packs, in place, selected members
SHAPE = [("diff", 2, 5000), ("delta", 4, 9001), ("diff", 1, 777), ("diff", 8, 0), ("planes", 4, 4097),
         ("diff", 2, 12289), ("diff", 8, 33), ("delta", 1, 5000), ("planes", 2, 1), ("diff", 4, 4100)]


def shaped_members(seed, shape=SHAPE):
    rng = np.random.default_rng(seed)
    out = []
    for k, w, n in shape:
        a = member_data(rng, "delta" if k == "delta" else "planes", w, n).view(DR.UINT[w])
        out.append((k, a, base_for(rng, a) if k == "diff" else None))
    return out


@pytest.fixture(scope="module")
def ref_vpack():
    """A reference-built versioned pack at 4 KiB blocks: (members, bytes).  Member 5 is a diff member whose planes
    start mid-block; member 3 is an empty diff member."""
    members = shaped_members(0x5E1EC8)
    return members, VR.build(members, BLOCK, CKPT, 2)


@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, 128), (2, 0), (1, 128), (1, 0)])
def test_reference_packs_decode_on_the_device(torch_cuda, nstates, ckpt):
    torch = torch_cuda
    members = mixed_members(0x4F0 + nstates + ckpt, [0, 1, 17, 4097, 9000])
    blob = VR.build(members, BLOCK, ckpt, nstates)
    assert R.FSE in R.types_of(blob[32 + 16 * len(members):])
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    bs = device_tensors(torch, [b for _, _, b in members])
    outs, st = codec_for().decompress_pack(buf, [torch_int(torch, a.itemsize) for _, a, _ in members], bases=bs)
    assert not bool(st.any())
    for o, (_, a, _) in zip(outs, members):
        assert bytes(o.view(torch.uint8).cpu().numpy()) == a.tobytes()


def decode_call(torch, blob, members, head, in_place=False, other_bases=None):
    """fsehip_vpack_decompress of host bytes with the given head into a poisoned arena; the bases in an arena of
    their own, or (in_place) at the diff members' destinations: (arena, base arena | None, block statuses, result)."""
    specs = VR.specs_of(members)
    arena = VArena(torch, specs, A5, offs_of(specs))
    based = members if other_bases is None else [(k, a, ob) for (k, a, _), ob in zip(members, other_bases)]
    if in_place:
        for (kind, _, _), p, raw in zip(specs, arena.pos, base_raws_of(based)):
            if kind == "diff":
                arena.host[p: p + raw.size] = raw
        arena.dev = torch.from_numpy(arena.host).cuda()
        bases, barr = None, arena.pointers()
    else:
        bases = base_arena(torch, based, offs_of(specs))
        barr = bases.pointers()
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    arr = arena.members()
    sw, scratch = g8(torch, lib().fsehip_vpack_scratch_bytes(arr, len(specs)))
    bw, bst = g32(torch, head.inner.n_blocks)
    rw, res = g32(torch, 2)
    rc = lib().fsehip_vpack_decompress(C.byref(head.info), arr, barr, C.byref(head.inner), 0, ptr(buf), buf.numel(),
                                       ptr(scratch), scratch.numel(), ptr(bst), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (bw, bst, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    if bases is not None:
        same(bases.dev.cpu().numpy(), bases.host, "the base arena after an out-of-place decode")
    return arena, bases, bst.cpu().numpy(), res.cpu().numpy()


@gpu
def test_in_place_decode(torch_cuda, ref_vpack):
    """d_ptr == d_bases[m] for every diff member: the bases become the new tensors, poison stays poison; and
    through Python with outs=bases."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    members, blob = ref_vpack
    head = BlockCodec.pack_info(blob)
    arena, _, bst, res = decode_call(torch, blob, members, head, in_place=True)
    assert res.tolist() == [0, 0] and not bst.any()
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the arena after the in-place decode")
    arena, _, bst, res = decode_call(torch, blob, members, head)
    assert res.tolist() == [0, 0] and not bst.any()
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the arena after the out-of-place decode")
    # Python: the previous checkpoint's tensors are updated in place
    xs, kinds, bs = on_device(torch, members)
    state = [b if b is not None else torch.full_like(x, 0x55) for x, b in zip(xs, bs)]
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    outs, st = codec_for().decompress_pack(buf, [x.dtype for x in xs], bases=bs, outs=state)
    assert not bool(st.any()) and all(o is s for o, s in zip(outs, state))
    assert all(torch.equal(s, x) for s, x in zip(state, xs))


def members_call(torch, blob, members, sel, head=None, in_place=False):
    """fsehip_vpack_decompress_members of host bytes into a poisoned arena that holds EVERY member's destination;
    only the selected diff members' bases are given, the other entries are null: (arena, statuses, result)."""
    from entropy_coders_amd import BlockCodec

    specs = VR.specs_of(members)
    head = BlockCodec.pack_info(blob) if head is None else head
    arena = VArena(torch, specs, A5, offs_of(specs))
    if in_place:
        for m, ((kind, _, _), p, raw) in enumerate(zip(specs, arena.pos, base_raws_of(members))):
            if kind == "diff" and m in sel:
                arena.host[p: p + raw.size] = raw
        arena.dev = torch.from_numpy(arena.host).cuda()
        bases, barr = None, arena.pointers(only=set(sel))
    else:
        bases = base_arena(torch, members, offs_of(specs))
        barr = bases.pointers(only=set(sel))
    if not any(specs[m][0] == "diff" and specs[m][2] for m in sel):
        barr = None  # no selected diff member with elements: the array may be null
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    arr = arena.members()
    csel = (C.c_uint32 * max(len(sel), 1))(*sel)
    need = lib().fsehip_vpack_members_scratch_bytes(arr, len(specs), csel, len(sel))
    sw, scratch = g8(torch, need)
    mw, mst = g32(torch, len(sel))
    rw, res = g32(torch, 2)
    rc = lib().fsehip_vpack_decompress_members(C.byref(head.info), arr, barr, C.byref(head.inner), 0, ptr(buf),
                                               buf.numel(), csel, len(sel), ptr(scratch), scratch.numel(), ptr(mst),
                                               ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (mw, mst, F32, "d_member_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    if bases is not None:
        same(bases.dev.cpu().numpy(), bases.host, "the base arena after the members call")
    return arena, mst.cpu().numpy(), res.cpu().numpy()


@gpu
@pytest.mark.parametrize("sel", [[0], [9], [3], list(range(10)), [5], [7, 1, 5], [4, 8, 1], []],
                         ids=["first", "last", "empty-member", "every", "diff-mid-block", "out-of-order", "no-diff", "none"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_selected_members(torch_cuda, ref_vpack, sel, in_place):
    members, blob = ref_vpack
    off5 = VR.plane_offsets(VR.specs_of(members))[5]
    assert all(o % BLOCK for o in off5), "member 5's planes start mid-block"
    arena, mst, res = members_call(torch_cuda, blob, members, sel, in_place=in_place)
    assert res.tolist() == [0, 0] and not mst.any(), (res, mst)
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members), only=set(sel)),
         "the selected members' bytes, poison in every other destination")


@gpu
def test_selected_members_python(torch_cuda, ref_vpack):
    torch = torch_cuda
    members, blob = ref_vpack
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    bs = device_tensors(torch, [b for _, _, b in members])
    codec = codec_for()
    for bases in ({5: bs[5], 0: bs[0]}, [bs[5], None, bs[0]]):  # a dict by member, or a list beside the indices
        outs, mst = codec.decompress_pack_members(buf, [5, 1, 0], [torch.int16, torch.int32, torch.bfloat16], bases=bases)
        assert mst.tolist() == [0, 0, 0] and outs[2].dtype == torch.bfloat16
        for o, m in zip(outs, (5, 1, 0)):
            assert bytes(o.view(torch.uint8).cpu().numpy()) == members[m][1].tobytes()
    with pytest.raises(ValueError, match="member 5 is a diff member"):
        codec.decompress_pack_members(buf, [5, 1], [torch.int16, torch.int32], bases={0: bs[0]})
    outs, mst = codec.decompress_pack_members(buf, [1, 4], [torch.int32, torch.float32])  # no diff member: no bases
    assert mst.tolist() == [0, 0] and bytes(outs[0].view(torch.uint8).cpu().numpy()) == members[1][1].tobytes()


# ---------------------------------------------------------------- damage and the documented hazard
def flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x01]) + b[at + 1:]


HEAD_DAMAGE = {
    "magic-FSEM": lambda b: b"FSEM" + b[4:],
    "version": lambda b: flip(b, 4),
    "reserved": lambda b: flip(b, 13),
    "n_members": lambda b: flip(b, 8),
    "image_bytes": lambda b: flip(b, 17),
    "content_bytes": lambda b: flip(b, 24),
    "first-member-kind": lambda b: b[:32] + b"\x01" + b[33:],
    "last-member-count": lambda b: flip(b, 32 + 16 * 9 + 8),
    "member-reserved": lambda b: flip(b, 32 + 16 * 4 + 5),
    "inner-n_total": lambda b: flip(b, 32 + 16 * 10 + 17),
    "truncated": lambda b: b[:-1],
}


@gpu
@pytest.mark.parametrize("name", list(HEAD_DAMAGE))
def test_a_head_changed_on_the_device_only_is_bad_frame(torch_cuda, ref_vpack, name):
    """The device's own check, given the good buffer's head: BAD_FRAME, every status BAD_FRAME, nothing stored to
    any member -- out of place, in place (the bases survive) and for selected members."""
    from entropy_coders_amd import BlockCodec

    members, good = ref_vpack
    head = BlockCodec.pack_info(good)
    bad = HEAD_DAMAGE[name](good)
    for in_place in (False, True):
        arena, _, bst, res = decode_call(torch_cuda, bad, members, head, in_place=in_place)
        assert res.tolist() == [BAD_FRAME, head.inner.n_blocks] and (bst == BAD_FRAME).all(), (res, bst[:4])
        same(arena.dev.cpu().numpy(), arena.host, "a rejected pack must leave every destination untouched")
    arena, mst, res = members_call(torch_cuda, bad, members, [0, 5, 3], head=head)
    assert res.tolist() == [BAD_FRAME, 3] and (mst == BAD_FRAME).all(), (res, mst)
    same(arena.dev.cpu().numpy(), arena.host, "a rejected pack must leave the selected destinations untouched")


@gpu
def test_a_damaged_payload_byte_costs_the_elements_of_one_block(torch_cuda, ref_vpack):
    """The last payload byte of one FSE record of the inner frame, which holds the stream's end marker, set to
    zero: that block fails; a planes or diff member loses the elements with a byte in it, a delta member the rest
    of those restart groups as well; every other element of every member equals the source."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    members, good = ref_vpack
    specs = VR.specs_of(members)
    head_bytes = 32 + 16 * len(specs)
    finfo, directory, records = R.split_frame(good[head_bytes:])
    offsets = VR.plane_offsets(specs)
    lost_any = 0
    for b in [i for i, (t, _) in enumerate(directory) if t == R.FSE][1::5]:
        pos = finfo["records_off"] + sum(8 * len(c) + len(d) for c, d in records[:b])
        at = head_bytes + pos + 8 * len(records[b][0]) + len(records[b][1]) - 1
        assert good[at] != 0
        bad = good[:at] + b"\0" + good[at + 1:]
        arena, _, bst, res = decode_call(torch, bad, members, BlockCodec.pack_info(good))
        assert int(res[0]) == 0 and int(res[1]) >= 1 and bst[b] != 0 and not np.delete(bst, b).any(), (b, res, bst)
        got = arena.dev.cpu().numpy()
        same(got[: arena.pos[0]], arena.host[: arena.pos[0]], "the arena below the first member")
        touched = []
        for m, ((kind, w, n), p, (_, a, _)) in enumerate(zip(specs, arena.pos, members)):
            hit = np.zeros(n, dtype=bool)
            for k in range(w):  # the member's elements with byte k inside block b
                lo, hi = max(b * BLOCK - offsets[m][k], 0), min((b + 1) * BLOCK - offsets[m][k], n)
                if lo < hi:
                    hit[lo:hi] = True
            if kind == "delta" and hit.any():  # a wrong delta reaches the end of its restart group
                for e in np.flatnonzero(hit):
                    hit[e: (e // DR.RESTART + 1) * DR.RESTART] = True
            if hit.any():
                touched.append(m)
            lost_any += int(hit.sum())
            elems = got[p: p + n * w].reshape(n, w)
            same(elems[~hit], VR.raw_bytes(a).reshape(n, w)[~hit], f"block {b}: member {m} outside the failed block")
            end = p + n * w  # the band behind the member is poison still
            same(got[end: end + GUARD], arena.host[end: end + GUARD], f"block {b}: behind member {m}")
        assert touched, b
        clean = next(m for m in range(len(specs)) if m not in touched and specs[m][2])
        arena, mst, res = members_call(torch, bad, members, [touched[0], clean])
        assert res.tolist() == [0, 1] and mst[0] == bst[b] and mst[1] == 0, (b, res, mst)
        same(arena.dev.cpu().numpy()[arena.pos[clean]: arena.pos[clean] + specs[clean][1] * specs[clean][2]],
             VR.raw_bytes(members[clean][1]), "the member outside the failed block")
    assert lost_any


@gpu
def test_another_base_decodes_to_other_values_with_every_status_ok(torch_cuda, ref_vpack):
    """The documented hazard: THE CONTAINER DOES NOT IDENTIFY ITS BASES.  Against bases one unit off the decode
    succeeds with every status FSE_OK and every diff element one unit off; the other kinds are untouched."""
    from entropy_coders_amd import BlockCodec

    members, blob = ref_vpack
    other = [None if b is None else (b + np.ones(1, b.dtype)).astype(b.dtype) for _, _, b in members]
    arena, _, bst, res = decode_call(torch_cuda, blob, members, BlockCodec.pack_info(blob), other_bases=other)
    assert res.tolist() == [0, 0] and not bst.any()
    shifted = [VR.raw_bytes((a + np.ones(1, a.dtype)).astype(a.dtype)) if k == "diff" else VR.raw_bytes(a)
               for k, a, _ in members]
    same(arena.dev.cpu().numpy(), arena.expect(shifted), "every diff element one unit off, nothing else")
    assert any(s.tobytes() != r.tobytes() for s, r in zip(shifted, raws_of(members)))


# ---------------------------------------------------------------- Python and host forms
@gpu
def test_python_split_merge_and_argument_errors(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    members = mixed_members(4, [17, 4097])
    xs, kinds, bs = on_device(torch, members)
    img = codec.pack_split(xs, kinds, bases=bs)
    same(img.cpu().numpy(), VR.image(members), "pack_split with bases")
    outs = codec.pack_merge(img, [torch.empty_like(x) for x in xs], kinds, bases=bs)
    assert all(torch.equal(o, x) for o, x in zip(outs, xs))
    state = [b.clone() if b is not None else torch.empty_like(x) for x, b in zip(xs, bs)]
    codec.pack_merge(img, state, kinds, bases=[s if b is not None else None for s, b in zip(state, bs)])  # in place
    assert all(torch.equal(s, x) for s, x in zip(state, xs))
    # the default kinds: "diff" where a base is given, "planes" where not
    buf = codec.compress_pack(xs, bases=bs)
    assert codec.pack_info(buf).kinds == ["planes" if b is None else "diff" for b in bs]
    assert bytes(codec.compress_pack(xs, "delta")[:4].cpu().numpy()) == b"FSEM"  # bases=None: today's path
    with pytest.raises(ValueError, match="needs its base"):
        codec.compress_pack(xs, "diff", bases=[None] * len(xs))
    with pytest.raises(ValueError, match="planes"):
        codec.compress_pack(xs, "diff")  # without bases= the pack frame's kinds
    with pytest.raises(ValueError, match="bases for"):
        codec.compress_pack(xs, bases=bs[:-1])
    with pytest.raises(ValueError, match="versioned pack takes"):
        codec.compress_pack(xs, "auto", bases=bs)
    with pytest.raises(ValueError, match="base 0"):
        codec.compress_pack(xs[:1], bases=[xs[0][:-1]])
    with pytest.raises(ValueError, match="base 0"):
        codec.compress_pack(xs[:1], bases=[torch.zeros(xs[0].numel(), dtype=torch.int64, device="cuda")])
    with pytest.raises(ValueError, match="contiguous device"):
        codec.compress_pack(xs[:1], bases=[xs[0].cpu()])
    buf = codec.compress_pack(xs, kinds, bases=bs)
    with pytest.raises(ValueError, match="pass bases="):
        codec.decompress_pack(buf, [x.dtype for x in xs])
    with pytest.raises(ValueError, match="bases for"):
        codec.decompress_pack(buf, [x.dtype for x in xs], bases=bs[:-1])
    with pytest.raises(ValueError, match="base 0"):
        codec.decompress_pack(buf, [x.dtype for x in xs], bases=[xs[1]] + bs[1:])
    with pytest.raises(ValueError, match="decompress_pack"):
        codec.decompress_auto(buf, torch.int16)
    outs, st = codec.decompress_pack(buf, [x.dtype for x in xs], bases=bs)
    assert not bool(st.any()) and all(torch.equal(o, x) for o, x in zip(outs, xs))


@gpu
def test_host_forms(torch_cuda):
    from entropy_coders_amd import FseError, container_kind, pack_compress, pack_decompress, pack_info

    rng = np.random.default_rng(2)
    w32 = rng.normal(0, 0.02, 3000).astype(np.float32)
    arrays = [np.arange(5000, dtype=np.int64) * 7, w32 + np.float32(1e-5) * rng.normal(0, 1, 3000).astype(np.float32),
              np.zeros(0, np.int16), np.arange(100, dtype=np.uint8)]
    bases = [None, w32, np.zeros(0, np.int16), None]
    kinds = ["delta", "diff", "diff", "planes"]
    blob = pack_compress(arrays, kinds, block_size=BLOCK, bases=bases)
    assert container_kind(blob) == "vpack"
    want = list(zip(kinds, arrays, bases))
    assert blob == reference_vpack(torch_cuda, codec_for(), want)
    head = pack_info(blob)
    assert head.container == "vpack" and head.kinds == kinds and head.n_elems == [5000, 3000, 0, 100]
    back = pack_decompress(blob, [a.dtype for a in arrays], bases=bases)
    assert all(b.dtype == a.dtype and np.array_equal(b, a) for a, b in zip(arrays, back))
    assert len(blob) < len(pack_compress(arrays, ["delta", "planes", "planes", "planes"], block_size=BLOCK))
    with pytest.raises(ValueError, match="pass bases="):
        pack_decompress(blob, [a.dtype for a in arrays])
    with pytest.raises(FseError) as e:
        pack_decompress(b"FSEM" + blob[4:], [a.dtype for a in arrays], bases=bases)  # kind 4 under the pack's magic
    assert e.value.code == "BAD_FRAME"


# ---------------------------------------------------------------- stream order
class VpackChain(Chain):
    """split -> compress -> decompress (out of place) -> members (in place) on one stream with no host
    synchronisation, sources and bases poison until the gate opens."""

    SEL = [4, 0, 5]
    SHAPE = [("diff", 2, 40 * BLOCK // 2 + 333), ("delta", 4, 9001), ("diff", 1, 777), ("diff", 8, 0),
             ("planes", 4, 4097), ("diff", 2, 12289), ("diff", 8, 33)]

    def __init__(self):
        # the oracle's checkpoints: no single-symbol block here (test_host_side_of_the_vpack_chain looks)
        self.members = shaped_members(0xC4A2, self.SHAPE)
        self.specs = VR.specs_of(self.members)
        self.want = VR.build(self.members, BLOCK, CKPT, 2)
        self.image = VR.image(self.members)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        self.head = BlockCodec.pack_info(self.want)
        self.src = [torch.empty(n, dtype=torch_int(torch, w), device="cuda") for _, w, n in self.specs]
        self.bases = [torch.empty(n, dtype=torch_int(torch, w), device="cuda") if k == "diff" else None
                      for k, w, n in self.specs]
        as_int = lambda a: a.view(np.dtype(f"i{a.itemsize}") if a.itemsize > 1 else np.uint8)  # noqa: E731
        self.uploads = [(s, pinned(torch, as_int(a))) for s, (_, a, _) in zip(self.src, self.members) if a.size]
        self.uploads += [(d, pinned(torch, as_int(b))) for d, (_, _, b) in zip(self.bases, self.members)
                         if d is not None and b.size]
        kinds = [k for k, _, _ in self.specs]
        n = len(self.specs)
        _, self.barr = c.pack_bases(self.src, self.bases, kinds)
        self.arr = c.pack_members(self.src, kinds, versioned=True)
        self.scratch = torch.empty(c.pack_scratch_bytes(self.arr, n, versioned=True), dtype=torch.uint8, device="cuda")
        self.w_img, self.img = g8(torch, len(self.image))
        self.w_buf, self.buf = g8(torch, c.pack_bound(self.arr, n, versioned=True))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.outs = [g8(torch, n_ * w) for _, w, n_ in self.specs]
        self.w_bst, self.bst = g32(torch, self.head.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        # the members call decodes in place: its destinations start out as copies of the bases (made on the stream)
        self.sel_outs = [g8(torch, self.specs[m][1] * self.specs[m][2]) for m in self.SEL]
        self.w_mst, self.mst = g32(torch, len(self.SEL))
        self.w_mres, self.mres = g32(torch, 2)
        self.mscratch = torch.empty(c.pack_members_scratch_bytes(self.arr, n, self.SEL, versioned=True),
                                    dtype=torch.uint8, device="cuda")

    def poison(self):
        for s in self.src:
            s.fill_(7)
        for b in self.bases:
            if b is not None:
                b.fill_(9)
        self.buf.zero_()  # what the decoders read: all zeros is BAD_FRAME
        self.img.fill_(A5)
        self.len.fill_(F64)
        for _, v in self.outs + self.sel_outs:
            v.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.mst, self.mres):
            t.fill_(F32)

    def enqueue(self, step9):
        c, t, n = self.codec, self.torch, len(self.specs)
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        rc = c.lib.fsehip_vpack_split(self.arr, n, self.barr, ptr(self.img), ptr(self.scratch), self.scratch.numel(),
                                      stream_of(t))
        assert rc == 0, rc
        c.compress_pack_into(self.arr, n, self.scratch, self.buf, self.len, self.cres, bases=self.barr)
        c.decompress_pack_into(buf, self.head, [v.view(torch_int(t, w)) for (_, v), (_, w, _) in
                                                zip(self.outs, self.specs)], self.scratch, self.bst, self.dres,
                               bases=self.bases)
        sel_views = [v.view(torch_int(t, self.specs[m][1])) for (_, v), m in zip(self.sel_outs, self.SEL)]
        for v, m in zip(sel_views, self.SEL):
            if self.bases[m] is not None:
                v.copy_(self.bases[m])  # on the stream, behind the upload
        c.decompress_pack_members_into(buf, self.head, self.SEL, sel_views, self.mscratch, self.mst, self.mres,
                                       bases={m: v for v, m in zip(sel_views, self.SEL) if self.bases[m] is not None})
        step9()

    def check(self):
        for w, v, f, name in ((self.w_img, self.img, A5, "d_image"), (self.w_buf, self.buf, A5, "d_out"),
                              (self.w_len, self.len, F64, "d_out_len"), (self.w_cres, self.cres, F32, "compress d_result"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_mst, self.mst, F32, "d_member_status"), (self.w_mres, self.mres, F32, "members d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        same(self.img.cpu().numpy(), self.image, "the image of the bare split")
        assert self.len.tolist() == [n], (self.len.tolist(), n)
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "versioned pack bytes")
        assert bool((self.buf[n:] == 0).all()), "a store past out_len"
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        for m, ((w, v), (_, a, _)) in enumerate(zip(self.outs, self.members)):
            assert_guards(w, v, A5, f"member {m}")
            same(v.cpu().numpy(), VR.raw_bytes(a), f"member {m}")
        for d, (_, _, b) in zip(self.bases, self.members):
            if d is not None:
                same(d.view(self.torch.uint8).cpu().numpy(), VR.raw_bytes(b), "a base after the chain")
        assert self.mres.tolist() == [0, 0] and not bool(self.mst.any()), (self.mres.tolist(), self.mst.tolist())
        for (w, v), m in zip(self.sel_outs, self.SEL):
            assert_guards(w, v, A5, f"selected member {m}")
            same(v.cpu().numpy(), VR.raw_bytes(self.members[m][1]), f"selected member {m}")


def test_host_side_of_the_vpack_chain():
    chain = VpackChain()
    assert len(chain.want) < VR.sums(chain.specs)[1] and R.FSE in R.types_of(chain.want[32 + 16 * len(chain.specs):])
    img = chain.image.tobytes()
    for b in range(0, len(img), BLOCK):  # a block of one non-zero symbol is FSE with no oracle walk
        assert len(set(img[b: b + BLOCK])) > 1 or img[b] == 0, b // BLOCK
    specs, raws = VR.decode(chain.want, [b for _, _, b in chain.members])
    assert specs == chain.specs and all(r.tobytes() == a.tobytes() for r, (_, a, _) in zip(raws, chain.members))


@gpu
def test_vpack_chain_behind_the_gate(torch_cuda, warm):
    """One split -> compress -> decompress -> members chain behind the gate of tests/test_gpu_stream_order.py:
    every call returns while its inputs are still poison, so none of them waits for the stream or reads device
    data on the host."""
    chain = VpackChain()
    chain.alloc(torch_cuda)
    warm.chains["vpack"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["vpack"] = warm.run(chain, gated=False)
    behind_gate(warm, "vpack")
