"""The pack frame on the GPU (include/fsehip.h section 2j): the split and
merge kernels alone against tests/pack_ref.py, members carved from one arena at
every element-aligned offset with poison between them, a list whose descriptor
table outgrows one staging buffer, container bytes against the reference at
both formats, reference-built packs decoded on the device, selected members,
damaged buffers and stream order.  Expected bytes never come from the code
under test; outputs sit between the guard bands of
tests/test_gpu_guard_bands.py or inside a poisoned arena compared whole."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import frame_ref as R
import pack_ref as KR
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
BAD_FRAME = R.BAD_FRAME
BLOCK, CKPT = 4096, 128
SRC_POISON = 0x5A
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65541]
GUARD = 256


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def codec_for(block=BLOCK, ckpt=CKPT, nstates=2, table_log=0):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=block, table_log=table_log, ckpt_interval=ckpt, nstates=nstates)


def lib():
    from entropy_coders_amd import _lib

    return _lib.load()


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def torch_int(torch, w):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w]


# ---------------------------------------------------------------- host data
def member_data(rng, kind, w, n):
    """Compressible elements of the kind: a random walk for delta members,
    small-magnitude floats' bits (few distinct top bytes) for plane members;
    every eighth member full-range bits, for wraparound both ways."""
    if rng.integers(8) == 0:
        return rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])
    if kind == "delta":
        return np.cumsum(rng.integers(-3, 40, n)).astype(DR.UINT[w])
    x = rng.normal(0, 0.02, n)
    if w == 8:
        return x.astype(np.float64).view(np.uint64)
    if w == 4:
        return x.astype(np.float32).view(np.uint32)
    if w == 2:
        return x.astype(np.float16).view(np.uint16)
    return np.clip(x * 400, -100, 100).astype(np.int8).view(np.uint8)


def mixed_members(seed, sizes=SIZES, flip=0):
    """Both kinds and all four widths at every size."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        for w in KR.WIDTHS:
            kind = ("planes", "delta")[(i + w.bit_length() + flip) % 2]
            out.append((kind, member_data(rng, kind, w, n)))
    return out


class Arena:
    """The members of a list carved from one device arena: member m at a
    256-byte slot start + offs[m] (a multiple of its element size), exactly
    n * w bytes, at least 256 bytes of `fill` before the next."""

    def __init__(self, torch, specs, fill, offs=None, raws=None):
        self.specs, self.fill = specs, fill
        self.pos, at = [], GUARD
        for m, (_, w, n) in enumerate(specs):
            off = 0 if offs is None else offs[m]
            assert off % w == 0 and off < 16
            self.pos.append(at + off)
            at = (at + off + n * w + GUARD - 1) // GUARD * GUARD + GUARD
        self.host = np.full(at, fill, dtype=np.uint8)
        if raws is not None:
            for p, raw in zip(self.pos, raws):
                self.host[p: p + raw.size] = raw
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % GUARD == 0

    def members(self, only=None):
        from entropy_coders_amd import _lib

        arr = (_lib.PackMember * max(len(self.specs), 1))()
        for m, ((kind, w, n), p) in enumerate(zip(self.specs, self.pos)):
            keep = n and (only is None or m in only)
            arr[m] = _lib.PackMember(self.dev.data_ptr() + p if keep else None, n, w, KR.KIND[kind])
        return arr

    def expect(self, raws, only=None):
        """The arena after a decode of the members `only` (None: all): their bytes, poison everywhere else."""
        want = np.full(self.host.size, self.fill, dtype=np.uint8)
        for m, (p, raw) in enumerate(zip(self.pos, raws)):
            if only is None or m in only:
                want[p: p + raw.size] = raw
        return want


def raws_of(members):
    return [KR.raw_bytes(a) for _, a in members]


def transform_scratch(torch, arr, n):
    L = lib()
    extra = L.fsehip_pack_scratch_bytes(arr, n) - L.fsehip_pack_image_bytes(arr, n)
    return g8(torch, max(extra, 16))


def split_on_device(torch, members, offs=None):
    """fsehip_pack_split of members in a source arena (poison behind every member): the image, guards asserted."""
    specs = KR.specs_of(members)
    arena = Arena(torch, specs, SRC_POISON, offs, raws_of(members))
    arr, n = arena.members(), len(specs)
    iw, img = g8(torch, KR.sums(specs)[0])
    sw, scratch = transform_scratch(torch, arr, n)
    rc = lib().fsehip_pack_split(arr, n, ptr(img), ptr(scratch), scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(iw, img, A5, "split image")
    assert_guards(sw, scratch, A5, "split scratch")
    same(arena.dev.cpu().numpy(), arena.host, "the split's source arena")
    return img.cpu().numpy()


def merge_on_device(torch, members, image, offs=None):
    """fsehip_pack_merge of a host image into a poisoned arena, compared whole."""
    specs = KR.specs_of(members)
    arena = Arena(torch, specs, A5, offs)
    arr, n = arena.members(), len(specs)
    dimg = dev_u8(torch, image) if len(image) else torch.empty(16, dtype=torch.uint8, device="cuda")
    sw, scratch = transform_scratch(torch, arr, n)
    rc = lib().fsehip_pack_merge(arr, n, ptr(dimg), ptr(scratch), scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(sw, scratch, A5, "merge scratch")
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the merge's destination arena")


# ---------------------------------------------------------------- split and merge alone
@gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_split_and_merge_against_pack_ref(torch_cuda, flip):
    members = mixed_members(0x9AC4 + flip, flip=flip)
    want = KR.image(members)
    same(split_on_device(torch_cuda, members), want, "pack image")  # pads included: they are zero in `want`
    merge_on_device(torch_cuda, members, want)


@gpu
def test_split_and_merge_of_nothing(torch_cuda):
    L = lib()
    for members in ([], [("delta", np.zeros(0, np.int32)), ("planes", np.zeros(0, np.uint8))]):
        assert split_on_device(torch_cuda, members).size == 0
        merge_on_device(torch_cuda, members, np.zeros(0, np.uint8))
    assert L.fsehip_pack_split(None, 0, None, None, 0, stream_of(torch_cuda)) == 0


@gpu
@pytest.mark.parametrize("w", KR.WIDTHS)
def test_exact_size_members_at_every_offset(torch_cuda, w):
    """Members carved from one arena at every element-aligned offset inside
    16 bytes, ragged sizes of both kinds, poison and 256-byte bands between
    them: a read past roundup(n * w, 4) puts poison into a pad of the image, a
    16-byte store past a ragged member changes the arena."""
    rng = np.random.default_rng(0xA7E4A + w)
    members, offs = [], []
    for off in range(0, 16, w):
        for kind in ("planes", "delta"):
            for n in (1, 3, 15, 17, 33, 4097):
                members.append((kind, rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])))
                offs.append(off)
    want = KR.image(members)
    same(split_on_device(torch_cuda, members, offs), want, f"pack image w={w}")
    merge_on_device(torch_cuda, members, want, offs)


@gpu
def test_python_split_merge_and_argument_errors(torch_cuda):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    codec = codec_for()
    members = mixed_members(3, [17, 4097])
    xs = [torch.from_numpy(a.view(np.dtype(f"i{a.itemsize}") if a.itemsize > 1 else np.uint8)).cuda() for _, a in members]
    kinds = [k for k, _ in members]
    img = codec.pack_split(xs, kinds)
    same(img.cpu().numpy(), KR.image(members), "pack_split")
    outs = codec.pack_merge(img, [torch.empty_like(x) for x in xs], kinds)
    assert all(torch.equal(o, x) for o, x in zip(outs, xs))
    with pytest.raises(ValueError, match="planes"):
        codec.compress_pack(xs, "diff")
    with pytest.raises(ValueError, match="kinds"):
        codec.compress_pack(xs, ["planes"])
    with pytest.raises(ValueError, match="contiguous"):
        codec.compress_pack([torch.zeros(10, 4, dtype=torch.float32, device="cuda").t()])
    with pytest.raises(ValueError, match="device"):
        codec.compress_pack([torch.zeros(10)])
    buf = codec.compress_pack(xs, kinds)
    with pytest.raises(ValueError, match="1-byte ones"):
        codec.decompress_pack(buf, torch.float32)
    with pytest.raises(ValueError, match="dtypes"):
        codec.decompress_pack(buf, [torch.int16])
    with pytest.raises(ValueError, match="twice"):
        codec.decompress_pack_members(buf, [1, 1], torch.int16)
    with pytest.raises(ValueError, match="holds 8"):
        codec.decompress_pack_members(buf, [8], torch.uint8)
    with pytest.raises(FseError) as e:
        codec.decompress_pack(buf[16:], torch.int16)
    assert e.value.code == "BAD_FRAME"
    outs, st = codec.decompress_pack(buf, [x.dtype for x in xs])
    assert not bool(st.any()) and all(torch.equal(o, x) for o, x in zip(outs, xs))
    outs, st = codec.decompress_pack(buf, [torch.uint8, torch.bfloat16, torch.float32, torch.float64] * 2)
    assert outs[1].dtype == torch.bfloat16 and torch.equal(outs[1].view(torch.int16), xs[1])


# ---------------------------------------------------------------- container bytes
def device_sidecars(torch, codec, image):
    """The zero-filled sidecar array the block encoder fills for the image
    (host uint64), as tests/test_gpu_planes.py passes it to the reference: a
    single-symbol block has no oracle walk."""
    if codec.ckpt_interval == 0 or len(image) == 0:
        return None
    cb = codec.compress(dev_u8(torch, image))
    return cb["sidecar"].cpu().numpy().view(np.uint64)


def device_tensors(torch, members):
    return [torch.from_numpy(a.view(np.dtype(f"i{a.itemsize}") if a.itemsize > 1 else np.uint8).copy()).cuda()
            for _, a in members]


def reference_pack(torch, codec, members):
    img = KR.image(members)
    return KR.build(members, codec.block_size, codec.ckpt_interval, codec.nstates, codec.table_log,
                    sidecars=device_sidecars(torch, codec, img))


BYTES_MEMBERS = [0, 1, 17, 300, 4097, 20011]


@gpu
@pytest.mark.parametrize("nstates,ckpt,block,table_log,offset", [(2, 128, 65536, 0, 0), (2, 0, 1040, 0, 0),
                                                                 (1, 128, 1040, 0, 0), (1, 0, 65536, 0, 0),
                                                                 (2, 128, 65536, 13, 0), (2, 128, 1040, 0, 1)])
def test_bytes_against_pack_ref(torch_cuda, nstates, ckpt, block, table_log, offset):
    """Device packs equal the reference's byte for byte, at an odd buffer
    address too (guard bands round every output; only out_len bytes are
    written), and decode on both sides."""
    torch = torch_cuda
    codec = codec_for(block, ckpt, nstates, table_log)
    members = mixed_members(0xB17E5 + block + nstates, BYTES_MEMBERS)
    xs, kinds = device_tensors(torch, members), [k for k, _ in members]
    want = reference_pack(torch, codec, members)
    arr, n = codec.pack_members(xs, kinds), len(xs)
    cap = codec.pack_bound(arr, n)
    assert cap == KR.bound(KR.specs_of(members), block) and len(want) <= cap
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.pack_scratch_bytes(arr, n))
    codec.compress_pack_into(arr, n, scratch, out, out_len, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0, (out_len.tolist(), len(want), res.tolist())
    same(out[: len(want)].cpu().numpy(), np.frombuffer(want, np.uint8), "pack bytes")
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the pack"
    assert R.FSE in R.types_of(want[32 + 16 * n:])
    outs, st = codec_for().decompress_pack(out[: len(want)], [x.dtype for x in xs])
    assert not bool(st.any()) and all(torch.equal(o, x) for o, x in zip(outs, xs))
    specs, raws = KR.decode(bytes(out[: len(want)].cpu().numpy()))
    assert specs == KR.specs_of(members) and all(r.tobytes() == a.tobytes() for r, (_, a) in zip(raws, members))


@gpu
def test_empty_packs(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    buf = codec.compress_pack([])
    assert bytes(buf.cpu().numpy()) == KR.build([], BLOCK, CKPT, 2) and buf.numel() == 64
    outs, st = codec.decompress_pack(buf, torch.int16)
    assert outs == [] and st.numel() == 0
    empties = [torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda")]
    buf = codec.compress_pack(empties, ["delta", "planes"])
    assert bytes(buf.cpu().numpy()) == KR.build([("delta", np.zeros(0, np.int32)), ("planes", np.zeros(0, np.uint8))],
                                                BLOCK, CKPT, 2)
    outs, st = codec.decompress_pack(buf, [torch.int32, torch.uint8])
    assert [o.numel() for o in outs] == [0, 0]
    outs, mst = codec.decompress_pack_members(buf, [1], torch.uint8)
    assert outs[0].numel() == 0 and mst.tolist() == [0]


@gpu
def test_many_members(torch_cuda):
    """3,000 members of 1 to 40 elements: 312,000 bytes of descriptors, more
    than one 64 KiB staging buffer holds; bytes against the reference, the
    whole decode into one poisoned arena, and 500 scattered members."""
    torch = torch_cuda
    rng = np.random.default_rng(0x3000)
    members = []
    for m in range(3000):
        kind, w = ("planes", "delta")[int(rng.integers(2))], int(rng.choice(KR.WIDTHS))
        members.append((kind, member_data(rng, kind, w, int(rng.integers(1, 41)))))
    codec = codec_for(65536, 128, 2)
    xs, kinds = device_tensors(torch, members), [k for k, _ in members]
    buf = codec.compress_pack(xs, kinds)
    want = reference_pack(torch, codec, members)
    same(buf.cpu().numpy(), np.frombuffer(want, np.uint8), "pack of 3,000 members")
    specs, raws = KR.specs_of(members), raws_of(members)
    head = codec.pack_info(buf)
    assert (head.kinds, head.elem_bytes, head.n_elems) == ([k for k, _, _ in specs], [w for _, w, _ in specs],
                                                           [n for _, _, n in specs])
    offs = [int(rng.integers(16 // w)) * w for _, w, _ in specs]
    arena = Arena(torch, specs, A5, offs)
    L = lib()
    sw, scratch = g8(torch, codec.pack_scratch_bytes(head.members, 3000))
    bw, bst = g32(torch, head.inner.n_blocks)
    rw, res = g32(torch, 2)
    rc = L.fsehip_pack_decompress(C.byref(head.info), arena.members(), C.byref(head.inner), 0, ptr(buf), buf.numel(),
                                  ptr(scratch), scratch.numel(), ptr(bst), ptr(res), stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (bw, bst, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    assert res.tolist() == [0, 0] and not bool(bst.any())
    same(arena.dev.cpu().numpy(), arena.expect(raws), "3,000 members decoded")
    pick = sorted(int(i) for i in rng.choice(3000, 500, replace=False))[::-1]
    outs, mst = codec.decompress_pack_members(buf, pick, [torch_int(torch, specs[m][1]) for m in pick])
    assert not bool(mst.any())
    for o, m in zip(outs, pick):
        assert bytes(o.view(torch.uint8).cpu().numpy()) == raws[m].tobytes(), m


# ---------------------------------------------------------------- reference frames, selected members
@pytest.fixture(scope="module")
def ref_pack():
    """A reference-built pack at 4 KiB blocks: (members, bytes).  Member 5 is
    a delta member whose planes start mid-block; member 3 is empty."""
    rng = np.random.default_rng(0x5E1EC7)
    shape = [("planes", 2, 5000), ("delta", 4, 9001), ("planes", 1, 777), ("delta", 8, 0), ("planes", 4, 4097),
             ("delta", 2, 12289), ("planes", 8, 33), ("delta", 1, 5000), ("planes", 2, 1)]
    members = [(k, member_data(rng, k, w, n)) for k, w, n in shape]
    return members, KR.build(members, BLOCK, CKPT, 2)


@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, 128), (2, 0), (1, 128), (1, 0)])
def test_reference_frames_decode_on_the_device(torch_cuda, nstates, ckpt):
    torch = torch_cuda
    members = mixed_members(0x4EF + nstates + ckpt, [0, 1, 17, 4097, 9000])
    blob = KR.build(members, BLOCK, ckpt, nstates)
    assert R.FSE in R.types_of(blob[32 + 16 * len(members):])
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    outs, st = codec_for().decompress_pack(buf, [torch_int(torch, a.itemsize) for _, a in members])
    assert not bool(st.any())
    for o, (_, a) in zip(outs, members):
        assert bytes(o.view(torch.uint8).cpu().numpy()) == a.tobytes()


def members_call(torch, blob, members, sel, head=None):
    """fsehip_pack_decompress_members of host bytes into a poisoned arena that
    holds EVERY member's destination: (arena, member statuses, result)."""
    from entropy_coders_amd import BlockCodec

    specs = KR.specs_of(members)
    head = BlockCodec.pack_info(blob) if head is None else head
    arena = Arena(torch, specs, A5)
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    arr = arena.members()
    csel = (C.c_uint32 * max(len(sel), 1))(*sel)
    need = lib().fsehip_pack_members_scratch_bytes(arr, len(specs), csel, len(sel))
    sw, scratch = g8(torch, need)
    mw, mst = g32(torch, len(sel))
    rw, res = g32(torch, 2)
    rc = lib().fsehip_pack_decompress_members(C.byref(head.info), arr, C.byref(head.inner), 0, ptr(buf), buf.numel(),
                                              csel, len(sel), ptr(scratch), scratch.numel(), ptr(mst), ptr(res),
                                              stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (mw, mst, F32, "d_member_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return arena, mst.cpu().numpy(), res.cpu().numpy()


@gpu
@pytest.mark.parametrize("sel", [[0], [8], [3], list(range(9)), [5], [7, 1, 5], []],
                         ids=["first", "last", "empty-member", "every", "delta-mid-block", "out-of-order", "none"])
def test_selected_members(torch_cuda, ref_pack, sel):
    members, blob = ref_pack
    off5 = KR.plane_offsets(KR.specs_of(members))[5]
    assert all(o % BLOCK for o in off5), "member 5's planes start mid-block"
    arena, mst, res = members_call(torch_cuda, blob, members, sel)
    assert res.tolist() == [0, 0] and not mst.any(), (res, mst)
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members), only=set(sel)),
         "the selected members' bytes, poison in every other destination")


@gpu
def test_selected_members_python(torch_cuda, ref_pack):
    torch = torch_cuda
    members, blob = ref_pack
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    outs, mst = codec_for().decompress_pack_members(buf, [5, 0], [torch.int16, torch.bfloat16])
    assert mst.tolist() == [0, 0] and outs[1].dtype == torch.bfloat16
    assert bytes(outs[0].view(torch.uint8).cpu().numpy()) == members[5][1].tobytes()
    assert bytes(outs[1].view(torch.uint8).cpu().numpy()) == members[0][1].tobytes()


@gpu
def test_host_forms(torch_cuda):
    from entropy_coders_amd import FseError, container_kind, pack_compress, pack_decompress, pack_info

    arrays = [np.arange(5000, dtype=np.int64) * 7, np.random.default_rng(1).normal(0, 1, 3000).astype(np.float32),
              np.zeros(0, np.int16), np.arange(100, dtype=np.uint8)]
    kinds = ["delta", "planes", "planes", "delta"]
    blob = pack_compress(arrays, kinds, block_size=BLOCK)
    assert container_kind(blob) == "pack"
    want = [(k, a) for k, a in zip(kinds, arrays)]
    codec = codec_for()
    assert blob == reference_pack(torch_cuda, codec, want)
    head = pack_info(blob)
    assert head.kinds == kinds and head.n_elems == [5000, 3000, 0, 100]
    back = pack_decompress(blob, [a.dtype for a in arrays])
    assert all(b.dtype == a.dtype and np.array_equal(b, a) for a, b in zip(arrays, back))
    with pytest.raises(ValueError, match="4-byte"):
        pack_decompress(blob, np.int64)
    with pytest.raises(FseError) as e:
        pack_decompress(b"FSEP" + blob[4:], [a.dtype for a in arrays])
    assert e.value.code == "BAD_FRAME"


# ---------------------------------------------------------------- damage
def decode_call(torch, blob, members, head):
    """fsehip_pack_decompress of host bytes with the given head into a poisoned arena: (arena, block statuses, result)."""
    specs = KR.specs_of(members)
    arena = Arena(torch, specs, A5)
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    arr = arena.members()
    sw, scratch = g8(torch, lib().fsehip_pack_scratch_bytes(arr, len(specs)))
    bw, bst = g32(torch, head.inner.n_blocks)
    rw, res = g32(torch, 2)
    rc = lib().fsehip_pack_decompress(C.byref(head.info), arr, C.byref(head.inner), 0, ptr(buf), buf.numel(),
                                      ptr(scratch), scratch.numel(), ptr(bst), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (bw, bst, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return arena, bst.cpu().numpy(), res.cpu().numpy()


def flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x01]) + b[at + 1:]


HEAD_DAMAGE = {
    "magic": lambda b: b"FSEP" + b[4:],
    "version": lambda b: flip(b, 4),
    "reserved": lambda b: flip(b, 13),
    "n_members": lambda b: flip(b, 8),
    "image_bytes": lambda b: flip(b, 17),
    "content_bytes": lambda b: flip(b, 24),
    "first-member-kind": lambda b: b[:32] + b"\x02" + b[33:],
    "last-member-count": lambda b: flip(b, 32 + 16 * 8 + 8),
    "member-reserved": lambda b: flip(b, 32 + 16 * 4 + 5),
    "inner-n_total": lambda b: flip(b, 32 + 16 * 9 + 17),
    "truncated": lambda b: b[:-1],
}


@gpu
@pytest.mark.parametrize("name", list(HEAD_DAMAGE))
def test_a_head_changed_on_the_device_only_is_bad_frame(torch_cuda, ref_pack, name):
    """The device's own check, given the good buffer's head: BAD_FRAME, every
    status BAD_FRAME, nothing stored to any member -- for the whole decode and
    for selected members."""
    from entropy_coders_amd import BlockCodec

    members, good = ref_pack
    head = BlockCodec.pack_info(good)
    bad = HEAD_DAMAGE[name](good)
    arena, bst, res = decode_call(torch_cuda, bad, members, head)
    assert res.tolist() == [BAD_FRAME, head.inner.n_blocks] and (bst == BAD_FRAME).all(), (res, bst[:4])
    same(arena.dev.cpu().numpy(), arena.host, "a rejected pack must leave every destination untouched")
    arena, mst, res = members_call(torch_cuda, bad, members, [0, 5, 3], head=head)
    assert res.tolist() == [BAD_FRAME, 3] and (mst == BAD_FRAME).all(), (res, mst)
    same(arena.dev.cpu().numpy(), arena.host, "a rejected pack must leave the selected destinations untouched")


@gpu
def test_a_damaged_payload_byte_costs_the_elements_of_one_block(torch_cuda, ref_pack):
    """The last payload byte of one FSE record of the inner frame, which holds
    the stream's end marker, flipped to zero (a damage no decoder can miss; a
    flip in mid-stream may decode to wrong bytes of the right length): that
    block fails; a plane member loses the elements with a byte in it, a delta member
    the rest of those restart groups as well; every other element of every
    member equals the source."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    members, good = ref_pack
    specs = KR.specs_of(members)
    head_bytes = 32 + 16 * len(specs)
    finfo, directory, records = R.split_frame(good[head_bytes:])
    offsets = KR.plane_offsets(specs)
    lost_any = 0
    for b in [i for i, (t, _) in enumerate(directory) if t == R.FSE][1::5]:
        pos = finfo["records_off"] + sum(8 * len(c) + len(d) for c, d in records[:b])
        at = head_bytes + pos + 8 * len(records[b][0]) + len(records[b][1]) - 1
        assert good[at] != 0
        bad = good[:at] + bytes([good[at] ^ good[at]]) + good[at + 1:]
        arena, bst, res = decode_call(torch, bad, members, BlockCodec.pack_info(good))
        assert int(res[0]) == 0 and int(res[1]) >= 1 and bst[b] != 0 and not np.delete(bst, b).any(), (b, res, bst)
        got = arena.dev.cpu().numpy()
        same(got[: arena.pos[0]], arena.host[: arena.pos[0]], "the arena below the first member")
        touched = []
        for m, ((kind, w, n), p, (_, a)) in enumerate(zip(specs, arena.pos, members)):
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
            same(elems[~hit], KR.raw_bytes(a).reshape(n, w)[~hit], f"block {b}: member {m} outside the failed block")
            end = p + n * w  # the band behind the member is poison still
            same(got[end: end + GUARD], arena.host[end: end + GUARD], f"block {b}: behind member {m}")
        assert touched, b
        # the same buffer through the members call: a member with a byte in the block fails, one without does not
        clean = next(m for m in range(len(specs)) if m not in touched and specs[m][2])
        arena, mst, res = members_call(torch, bad, members, [touched[0], clean])
        assert res.tolist() == [0, 1] and mst[0] == bst[b] and mst[1] == 0, (b, res, mst)
        same(arena.dev.cpu().numpy()[arena.pos[clean]: arena.pos[clean] + specs[clean][1] * specs[clean][2]],
             KR.raw_bytes(members[clean][1]), "the member outside the failed block")
    assert lost_any


# ---------------------------------------------------------------- stream order
class PackChain(Chain):
    """compress -> decompress -> members on one stream with no host
    synchronisation, inputs poison until the gate opens."""

    SEL = [4, 0, 5]

    def __init__(self):
        rng = np.random.default_rng(0xC4A1)
        shape = [("planes", 2, 40 * BLOCK // 2 + 333), ("delta", 4, 9001), ("planes", 1, 777), ("delta", 8, 0),
                 ("planes", 4, 4097), ("delta", 2, 12289), ("planes", 8, 33)]
        # the oracle's checkpoints: no single-symbol block here (test_host_side_of_the_pack_chain looks)
        self.members = [(k, member_data(rng, k, w, n)) for k, w, n in shape]
        self.specs = KR.specs_of(self.members)
        self.want = KR.build(self.members, BLOCK, CKPT, 2)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        self.head = BlockCodec.pack_info(self.want)
        self.src = [torch.empty(n, dtype=torch_int(torch, w), device="cuda") for _, w, n in self.specs]
        self.uploads = [(s, pinned(torch, a.view(np.dtype(f"i{a.itemsize}") if a.itemsize > 1 else np.uint8)))
                        for s, (_, a) in zip(self.src, self.members) if a.size]
        self.arr, n = c.pack_members(self.src, [k for k, _, _ in self.specs]), len(self.specs)
        self.scratch = torch.empty(c.pack_scratch_bytes(self.arr, n), dtype=torch.uint8, device="cuda")
        self.w_buf, self.buf = g8(torch, c.pack_bound(self.arr, n))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.outs = [g8(torch, n_ * w) for _, w, n_ in self.specs]
        self.w_bst, self.bst = g32(torch, self.head.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.sel_outs = [g8(torch, self.specs[m][1] * self.specs[m][2]) for m in self.SEL]
        self.w_mst, self.mst = g32(torch, len(self.SEL))
        self.w_mres, self.mres = g32(torch, 2)
        self.mscratch = torch.empty(c.pack_members_scratch_bytes(self.arr, n, self.SEL), dtype=torch.uint8,
                                    device="cuda")

    def poison(self):
        for s in self.src:
            s.fill_(7)
        self.buf.zero_()  # what the decoders read: all zeros is BAD_FRAME
        self.len.fill_(F64)
        for _, v in self.outs + self.sel_outs:
            v.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.mst, self.mres):
            t.fill_(F32)

    def enqueue(self, step9):
        c, t = self.codec, self.torch
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        c.compress_pack_into(self.arr, len(self.specs), self.scratch, self.buf, self.len, self.cres)
        c.decompress_pack_into(buf, self.head, [v.view(torch_int(t, w)) for (_, v), (_, w, _) in
                                                zip(self.outs, self.specs)], self.scratch, self.bst, self.dres)
        c.decompress_pack_members_into(buf, self.head, self.SEL,
                                       [v.view(torch_int(t, self.specs[m][1])) for (_, v), m in
                                        zip(self.sel_outs, self.SEL)], self.mscratch, self.mst, self.mres)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_buf, self.buf, A5, "d_out"), (self.w_len, self.len, F64, "d_out_len"),
                              (self.w_cres, self.cres, F32, "compress d_result"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_mst, self.mst, F32, "d_member_status"), (self.w_mres, self.mres, F32, "members d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        assert self.len.tolist() == [n], (self.len.tolist(), n)
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "pack bytes")
        assert bool((self.buf[n:] == 0).all()), "a store past out_len"
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        for m, ((w, v), (_, a)) in enumerate(zip(self.outs, self.members)):
            assert_guards(w, v, A5, f"member {m}")
            same(v.cpu().numpy(), KR.raw_bytes(a), f"member {m}")
        assert self.mres.tolist() == [0, 0] and not bool(self.mst.any()), (self.mres.tolist(), self.mst.tolist())
        for (w, v), m in zip(self.sel_outs, self.SEL):
            assert_guards(w, v, A5, f"selected member {m}")
            same(v.cpu().numpy(), KR.raw_bytes(self.members[m][1]), f"selected member {m}")


def test_host_side_of_the_pack_chain():
    chain = PackChain()
    assert len(chain.want) < KR.sums(chain.specs)[1] and R.FSE in R.types_of(chain.want[32 + 16 * len(chain.specs):])
    img = KR.image(chain.members).tobytes()
    for b in range(0, len(img), BLOCK):  # a block of one non-zero symbol is FSE with no oracle walk
        assert len(set(img[b: b + BLOCK])) > 1 or img[b] == 0, b // BLOCK
    specs, raws = KR.decode(chain.want)
    assert specs == chain.specs and all(r.tobytes() == a.tobytes() for r, (_, a) in zip(raws, chain.members))


@gpu
def test_pack_chain_behind_the_gate(torch_cuda, warm):
    """One compress -> decompress -> members chain behind the gate of
    tests/test_gpu_stream_order.py: every call returns while its inputs are
    still poison, so none of them waits for the stream or reads device data
    on the host."""
    chain = PackChain()
    chain.alloc(torch_cuda)
    warm.chains["pack"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["pack"] = warm.run(chain, gated=False)
    behind_gate(warm, "pack")
