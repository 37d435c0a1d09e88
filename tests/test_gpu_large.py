"""Every container past 4 GiB on the GPU, against tests/large_ref.py: a source
of one 15-block tile repeated about 5,000 times and a ragged tail (4.6 GiB),
whose reference frame -- frame_ref.build_frame of the tile and the tail on
the CPU oracle, laid out k times on the device -- is itself longer than 2^32
bytes.  Source, image and frame all have byte offsets, element indices, scan
carries, CRC exponents and directory offsets that do not fit 32 bits, and a
tile of 15 blocks sends an offset wrapped by 2^32 or 2^31 to a different
block (large_ref.TILE_BLOCKS).

  frame       exact bytes at two chunkings; decode of the REFERENCE frame;
              byte ranges across 2^31, 2^32 and a record across frame offset 2^32
  check       the record, verify, one flipped byte above 2^32, sealed ranges
  transforms  plane / delta / diff images against their torch restatements
  containers  plane, delta and diff frames as header + frame of the image
  packs       pack, versioned pack and sealed pack with a 2.3 G element member
  estimate    the frame estimate and compress_auto

Device memory: torch.cuda.max_memory_allocated reported a peak of 27.7 GiB
for this module on an MI355X (test_peak_memory_is_under_the_cap prints it);
the library's own workspace (one chunk's scratch) comes on top.  The module
skips when less than CAP, 40 GiB, is free, and never otherwise.  Every test
frees what it allocated: the seconds such a test sometimes takes are the
driver's, handing a freed multi-GiB block out again, not a kernel's."""
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import delta_ref as DR
import diff_ref as FR
import large_ref as L
import planes_ref as PR

pytestmark = pytest.mark.gpu

BLOCK = L.BLOCK
CKPT = 128
SEED = 0x1A26E
CAP = 40 << 30          # bytes this module may hold at once
CHECKSUM = -21
# (ckpt, nstates) of every reference frame below: k makes each of them pass 2^32
CONFIGS = [(CKPT, 2), (CKPT, 1), (0, 2)]
AT32, AT31 = 1 << 32, 1 << 31


def codec_for(ckpt=CKPT, nstates=2):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=BLOCK, ckpt_interval=ckpt, nstates=nstates)


@pytest.fixture(scope="module")
def big():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    free, _ = torch.cuda.mem_get_info()
    if free < CAP:
        pytest.skip(f"the module holds up to {CAP} bytes of device memory, {free} are free")
    tile, tail = L.tile_and_tail(SEED)
    k = L.tiles_for(tile, tail, BLOCK, CONFIGS)
    layouts = {c: L.tiled_layout(tile, k, tail, BLOCK, *c) for c in CONFIGS}
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ns = SimpleNamespace(torch=torch, tile=tile, tail=tail, k=k, layouts=layouts,
                         n_total=k * len(tile) + len(tail), src=L.tiled_source(tile, k, tail, "cuda"))
    yield ns
    ns.src = None
    codec_for().release_workspace()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def free(torch):
    torch.cuda.empty_cache()


def same_bytes(torch, got, want, what):
    """torch.equal of two tensors' bytes; on a difference, where it starts."""
    got, want = got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8)
    assert got.numel() == want.numel(), f"{what}: {got.numel()} bytes, the reference has {want.numel()}"
    if torch.equal(got, want):
        return
    step = 1 << 28
    for lo in range(0, got.numel(), step):
        a, b = got[lo: lo + step], want[lo: lo + step]
        if not torch.equal(a, b):
            i = lo + int((a != b).nonzero()[0])
            pytest.fail(f"{what}: first difference at byte {i} = {i:#x} of {got.numel()} (64 KiB block {i >> 16}): "
                        f"{got[i: i + 8].tolist()} against {want[i: i + 8].tolist()}")
    raise AssertionError(f"{what}: torch.equal of the whole differs from torch.equal of its parts")


def elems(big, w, t=None):
    """The source (or another tiled tensor) trimmed to whole w-byte elements, as integers."""
    t = big.src if t is None else t
    return t[: big.n_total // w * w].view(L.INT[w])


def rotated_base(big):
    """A second tiled tensor, from the tile rotated by one block: differences against it are non-trivial everywhere."""
    return L.tiled_source(L.rotated(big.tile), big.k, big.tail, "cuda")


def test_the_case_is_past_the_edge(big):
    assert big.n_total > AT32 + 2 * len(big.tile)
    assert big.src.numel() == big.n_total and big.n_total % 2 == 1
    for c, lay in big.layouts.items():
        assert lay["frame_len"] > AT32 + 2 * len(lay["tile_rec"]), c
        assert lay["n_blocks"] == big.k * L.TILE_BLOCKS + 1
    # k is the smallest such count
    assert any(L.tiled_layout(big.tile, big.k - 1, big.tail, BLOCK, *c)["frame_len"]
               < AT32 + 2 * len(big.layouts[c]["tile_rec"]) for c in CONFIGS)
    # w = 2 puts element index 2^31 inside the tensor, w = 8 byte offset 2^32 at element 2^29
    assert big.n_total // 2 > AT31 and big.n_total // 8 > 1 << 29 and (1 << 29) * 8 == AT32


def test_the_comparison_sees_one_byte_past_2_32(big):
    """Every test below rests on torch.equal over more than 2^32 elements:
    one changed byte anywhere, the very last included, must make it fail."""
    torch = big.torch
    other = big.src.clone()
    same_bytes(torch, other, big.src, "the clone")
    for at in (big.n_total - 1, AT32 + 1, AT32 - 1, AT31, 0):
        other[at] ^= 1
        assert not torch.equal(other, big.src), at
        if at > AT32:  # where it is: same_bytes' own report
            with pytest.raises(pytest.fail.Exception, match=f"first difference at byte {at} "):
                same_bytes(torch, other, big.src, "one byte changed")
        other[at] ^= 1
    assert torch.equal(other, big.src)
    del other
    free(torch)


# ---------------------------------------------------------------- a. the frame, exact bytes
@pytest.mark.parametrize("nstates", [2, 1])
def test_frame_bytes(big, nstates):
    torch = big.torch
    lay = big.layouts[(CKPT, nstates)]
    assert big.n_total > AT32 + 2 * len(big.tile)
    want = L.tiled_frame(big.tile, big.k, big.tail, BLOCK, CKPT, nstates, "cuda", layout=lay)
    assert want.numel() == lay["frame_len"] > AT32 + 2 * len(lay["tile_rec"])
    codec = codec_for(CKPT, nstates)
    for chunk in (0, 1000):  # 1,000 does not divide the block count: other chunk seams, the same frame
        assert lay["n_blocks"] % 1000
        got = codec.compress_frame(big.src, chunk_blocks=chunk)
        same_bytes(torch, got, want, f"frame nstates={nstates} chunk_blocks={chunk}")
        del got
    del want
    free(torch)


def test_a_record_from_2_32_further_on_is_reported(big):
    """The mutation the tile of 15 blocks exists for: block b + 65,536's
    record in block b's place (what a record offset wrapped by 2^32 bytes of
    source would fetch) is another record, and the comparison says where."""
    torch = big.torch
    lay = big.layouts[(CKPT, 2)]
    want = L.tiled_frame(big.tile, big.k, big.tail, BLOCK, CKPT, 2, "cuda", layout=lay)
    b = 5 * L.TILE_BLOCKS
    far = b + AT32 // BLOCK
    assert far < lay["n_blocks"] and far % L.TILE_BLOCKS != b % L.TILE_BLOCKS
    (lo, hi), (lo2, hi2) = L.record_span(lay, b), L.record_span(lay, far)
    assert hi - lo == hi2 - lo2 == BLOCK  # both RAW: the frame stays well formed
    bad = want.clone()
    bad[lo:hi] = want[lo2:hi2]
    with pytest.raises(pytest.fail.Exception, match="first difference at byte") as e:
        same_bytes(torch, bad, want, "a record from 2^32 further on")
    assert lo <= int(str(e.value).split("first difference at byte ")[1].split()[0]) < lo + 8
    del want, bad
    free(torch)


# ---------------------------------------------------------------- b. the frame, decode of the reference
@pytest.mark.parametrize("nstates,ckpt", [(2, CKPT), (1, CKPT), (2, 0)])
def test_frame_decode_of_the_reference(big, nstates, ckpt):
    torch = big.torch
    lay = big.layouts[(ckpt, nstates)]
    ref = L.tiled_frame(big.tile, big.k, big.tail, BLOCK, ckpt, nstates, "cuda", layout=lay)
    assert ref.numel() > AT32
    out, status = codec_for(ckpt, nstates).decompress_frame(ref)
    assert status.numel() == lay["n_blocks"] and not bool(status.any())
    same_bytes(torch, out, big.src, f"decode nstates={nstates} ckpt={ckpt}")
    del ref, out, status
    free(torch)


# ---------------------------------------------------------------- c. the frame, ranges
def frame_ranges(big, lay):
    n = big.n_total
    block, lo, hi = L.block_of_frame_offset(lay, AT32)
    assert lo < AT32 < hi  # its record straddles frame offset 2^32
    b_lo = block * BLOCK
    assert AT31 < b_lo - 7 and b_lo + BLOCK + 11 < n
    ranges = [(AT32 - 70001, 70001 + 65539),          # across raw offset 2^32, odd on both sides
              (AT31 - 12345, 12345 + 54321),          # across 2^31
              (AT32 + 3 * BLOCK + 777, 200001),       # wholly above 2^32, from mid-block
              (AT32 + 40 * BLOCK + 4099, 6 * BLOCK + 999),  # the same with whole blocks inside: the direct route
              (n - 50000, 50000),                     # the tail and part of the block before it
              (n - 1, 1),
              (b_lo - 7, BLOCK + 18)]                 # the block whose record straddles frame offset 2^32
    assert 50000 > len(big.tail)
    return ranges


def test_frame_ranges(big):
    torch = big.torch
    lay = big.layouts[(CKPT, 2)]
    ref = L.tiled_frame(big.tile, big.k, big.tail, BLOCK, CKPT, 2, "cuda", layout=lay)
    ranges = frame_ranges(big, lay)
    codec = codec_for()
    views, status = codec.decompress_frame_ranges(ref, ranges)
    assert status.tolist() == [0] * len(ranges)
    for (s, ln), v in zip(ranges, views):
        same_bytes(torch, v, big.src[s: s + ln], f"range ({s}, {ln})")
    # the output 5 bytes off: the unaligned bounce path, and nothing stored outside
    packed, at = [], 0
    for s, ln in ranges:
        packed.append((s, ln, at))
        at += ln
    buf = torch.full((at + 5 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[5: 5 + at]
    assert out.data_ptr() % 16 == 5
    status = torch.full((len(ranges),), 77, dtype=torch.int32, device="cuda")
    result = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    codec.decompress_frame_ranges_into(ref, codec.frame_info(ref), packed, out, status, result)
    assert result.tolist() == [0, 0] and status.tolist() == [0] * len(ranges)
    for s, ln, d in packed:
        same_bytes(torch, out[d: d + ln], big.src[s: s + ln], f"range ({s}, {ln}) at {d} + 5")
    assert buf[:5].tolist() == [0xA5] * 5 and buf[5 + at:].tolist() == [0xA5] * 32
    del ref, views, buf, out
    free(torch)


# ---------------------------------------------------------------- d. the check record
def test_check_record(big):
    torch = big.torch
    codec = codec_for()
    want = L.tiled_crc(big.tile, big.k, big.tail)
    got = codec.check_build(big.src)
    assert got.cpu().numpy().tobytes() == want
    rec = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
    status, result = codec.check_verify(rec, big.src)
    assert status.numel() == (big.n_total + 65535) >> 16 and not bool(status.any()) and result.tolist() == [0, 0]
    at = AT32 + 70000
    bad = big.src.clone()
    bad[at] ^= 0x40
    status, result = codec.check_verify(rec, bad)
    assert status.nonzero().flatten().tolist() == [at >> 16] and int(status[at >> 16]) == CHECKSUM
    assert result.tolist() == [CHECKSUM, 1]
    del bad
    free(torch)
    sealed = codec.compress_sealed(big.src, "frame")
    assert sealed[: len(want)].cpu().numpy().tobytes() == want
    assert sealed.numel() == len(want) + big.layouts[(CKPT, 2)]["frame_len"]
    s, ln = AT32 - 70001, 140003 + 2 * BLOCK  # whole check blocks on both sides of 2^32 among them
    views, st, cst = codec.decompress_sealed_ranges(sealed, None, [(s, ln)])
    assert st.tolist() == [0] and cst.tolist() == [0]
    same_bytes(torch, views[0], big.src[s: s + ln], "sealed range across 2^32")
    del sealed, views
    free(torch)


# ---------------------------------------------------------------- e. the transforms
@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("kind", ["planes", "delta"])
def test_transforms(big, kind, w):
    torch = big.torch
    codec = codec_for()
    x = elems(big, w)
    n, dt = x.numel(), L.INT[w]
    assert n * w > AT32 and (w != 2 or n > AT31) and (w != 8 or n > 1 << 29)
    image, encode, decode = {"planes": (L.planes_image, codec.planes_split, codec.planes_merge),
                             "delta": (L.delta_image, codec.delta_encode, codec.delta_decode)}[kind]
    ref = image(x)
    got = encode(x)
    same_bytes(torch, got, ref, f"{kind} image w={w}")
    del ref
    back = decode(got, n, dt)
    same_bytes(torch, back, x, f"{kind} inverse w={w}")
    del got, back
    free(torch)


@pytest.mark.parametrize("w", [2, 4, 8])
def test_diff_transform(big, w):
    torch = big.torch
    codec = codec_for()
    x = elems(big, w)
    assert x.numel() * w > AT32 and (w != 2 or x.numel() > AT31) and (w != 8 or x.numel() > 1 << 29)
    base = elems(big, w, rotated_base(big))
    ref = L.diff_image(x, base)
    got = codec.diff_encode(x, base)
    same_bytes(torch, got, ref, f"diff image w={w}")
    del ref
    back = codec.diff_decode(got, base)
    same_bytes(torch, back, x, f"diff inverse w={w}")
    del back
    assert codec.diff_decode(got, base, out=base) is base  # in place: the base becomes x
    same_bytes(torch, base, x, f"diff inverse in place w={w}")
    del got, base
    free(torch)


# ---------------------------------------------------------------- f. the element containers, layered
# One width per container: w = 2 for planes and diff (element indices past 2^31), w = 8 for delta.
CONTAINERS = [("planes", 2), ("diff", 2), ("delta", 8)]


def container_of(big, kind, w):
    """(x, base | None, the container's expected header, the torch image, the compressed buffer)."""
    codec = codec_for()
    x = elems(big, w)
    if kind == "planes":
        return x, None, PR.header(w, x.numel()), L.planes_image, codec.compress_planes(x)
    if kind == "delta":
        return x, None, DR.header(w, x.numel()), L.delta_image, codec.compress_delta(x)
    base = elems(big, w, rotated_base(big))
    return x, base, FR.header(w, x.numel()), lambda t: L.diff_image(t, base), codec.compress_diff(x, base)


@pytest.mark.parametrize("kind,w", CONTAINERS)
def test_element_container_bytes(big, kind, w):
    """The composition planes_ref.py / delta_ref.py / diff_ref.py define: the
    header, then the frame of the image.  The frame is pinned by
    test_frame_bytes, the image by test_transforms / test_diff_transform."""
    torch = big.torch
    x, base, header, image_of, buf = container_of(big, kind, w)
    assert buf[:16].cpu().numpy().tobytes() == header
    image = image_of(x)
    assert image.numel() == w * PR.stride_of(x.numel()) > AT32
    inner = codec_for().compress_frame(image)
    assert inner.numel() > AT31
    same_bytes(torch, buf[16:], inner, f"{kind} w={w}: the inner frame")
    del inner, image, buf, base
    free(torch)


@pytest.mark.parametrize("kind,w", CONTAINERS)
def test_element_container_decode(big, kind, w):
    torch = big.torch
    codec = codec_for()
    x, base, _, _, buf = container_of(big, kind, w)
    n, dt = x.numel(), L.INT[w]
    if kind == "planes":
        out, status = codec.decompress_planes(buf, dt)
    elif kind == "delta":
        out, status = codec.decompress_delta(buf, dt)
    else:
        out, status = codec.decompress_diff(buf, base)
    assert not bool(status.any())
    same_bytes(torch, out, x, f"{kind} w={w} round trip")
    del out, status
    # element ranges: across byte 2^32 of the source, across byte 2^32 of the image, the ragged end
    plane, i = divmod(AT32, PR.stride_of(n))
    assert 0 < plane < w and 5000 < i < n - 5000
    ranges = [(AT32 // w - 1001, 2003), (i - 1001, 2003), (n - 777, 777)]
    if kind == "planes":
        views, status = codec.decompress_planes_ranges(buf, dt, ranges)
    elif kind == "delta":
        views, status = codec.decompress_delta_ranges(buf, dt, ranges)
    else:
        views, status = codec.decompress_diff_ranges(buf, base, ranges)
    assert status.tolist() == [0] * len(ranges)
    for (s, cnt), v in zip(ranges, views):
        same_bytes(torch, v, x[s: s + cnt], f"{kind} w={w} elements ({s}, {cnt})")
    del views, buf, base
    free(torch)


# ---------------------------------------------------------------- g. packs
def pack_members(big):
    """Six members: the source as int16 (more than 2^32 bytes and 2^31
    elements), 2^20 + 3 int64 ids, and four small float members behind them."""
    torch = big.torch
    g = torch.Generator().manual_seed(SEED)
    ids = torch.cumsum(torch.randint(1, 2000, (2 ** 20 + 3,), generator=g), 0)
    smalls = [(torch.randn(cnt, generator=g) * 0.02).to(dt) for cnt, dt in
              ((256, torch.bfloat16), (4097, torch.float32), (70001, torch.bfloat16), (1000, torch.float32))]
    newer = [(s.float() + 1e-4 * torch.randn(s.numel(), generator=g)).to(s.dtype) for s in smalls]
    xs = [elems(big, 2), ids.cuda()] + [s.cuda() for s in newer]
    bases = [None, None, smalls[0].cuda(), None, None, smalls[3].cuda()]  # the big member's base: the caller's
    return xs, bases


def crc_of(t):
    """zlib.crc32 of a tensor's bytes."""
    return zlib.crc32(t.cpu().reshape(-1).view(L.INT[t.element_size()]).numpy().tobytes())


def test_pack(big):
    torch = big.torch
    codec = codec_for()
    xs, _ = pack_members(big)
    kinds = ["planes", "delta", "planes", "planes", "planes", "planes"]
    dts = [x.dtype for x in xs]
    assert xs[0].numel() > AT31 and xs[0].numel() * 2 > AT32
    members = codec.pack_members(xs, kinds)
    for m in range(2, 6):  # the small members' planes lie behind the big member's
        offs = [int(codec.lib.fsehip_pack_plane_offset(members, 6, m, p)) for p in range(xs[m].element_size())]
        assert min(offs) > AT31 and max(offs) > AT32, (m, offs)
    buf = codec.compress_pack(xs, kinds)
    assert buf.numel() > AT31
    head = codec.pack_info(buf)
    assert head.container == "pack" and head.kinds == kinds
    assert head.elem_bytes == [x.element_size() for x in xs] and head.n_elems == [x.numel() for x in xs]
    assert head.info.content_bytes == sum(x.numel() * x.element_size() for x in xs) > AT32
    outs, status = codec.decompress_pack(buf, dts)
    assert not bool(status.any())
    for m, (o, x) in enumerate(zip(outs, xs)):
        assert o.dtype == x.dtype
        same_bytes(torch, o, x, f"pack member {m}")
    del outs
    free(torch)
    pick = [5, 2, 3, 4]
    outs, mst = codec.decompress_pack_members(buf, pick, [dts[m] for m in pick])
    assert mst.tolist() == [0] * len(pick)
    for o, m in zip(outs, pick):
        same_bytes(torch, o, xs[m], f"selected pack member {m}")
    del buf, outs
    free(torch)


def test_versioned_pack(big):
    torch = big.torch
    codec = codec_for()
    xs, bases = pack_members(big)
    bases[0] = elems(big, 2, rotated_base(big))
    dts = [x.dtype for x in xs]
    buf = codec.compress_pack(xs, bases=bases)
    head = codec.pack_info(buf)
    assert head.container == "vpack"
    assert head.kinds == ["diff", "planes", "diff", "planes", "planes", "diff"]
    assert head.n_elems == [x.numel() for x in xs]
    outs, status = codec.decompress_pack(buf, dts, bases=bases)  # out of place
    assert not bool(status.any())
    for m, (o, x) in enumerate(zip(outs, xs)):
        same_bytes(torch, o, x, f"versioned pack member {m}")
    del outs
    free(torch)
    olds = [b.clone() if b is not None else torch.empty_like(x) for b, x in zip(bases, xs)]  # in place
    outs, status = codec.decompress_pack(buf, dts, bases=[o if b is not None else None for o, b in zip(olds, bases)],
                                         outs=olds)
    assert not bool(status.any()) and all(o is q for o, q in zip(outs, olds))
    for m, (o, x) in enumerate(zip(olds, xs)):
        same_bytes(torch, o, x, f"versioned pack member {m} in place")
    del outs, olds
    free(torch)
    pick = [5, 2, 3, 4]
    outs, mst = codec.decompress_pack_members(buf, pick, [dts[m] for m in pick], bases={m: bases[m] for m in pick})
    assert mst.tolist() == [0] * len(pick)
    for o, m in zip(outs, pick):
        same_bytes(torch, o, xs[m], f"selected versioned pack member {m}")
    del buf, outs, bases
    free(torch)


def test_sealed_pack(big):
    torch = big.torch
    codec = codec_for()
    xs, bases = pack_members(big)
    bases[0] = elems(big, 2, rotated_base(big))
    dts = [x.dtype for x in xs]
    buf = codec.compress_pack_sealed(xs, bases=bases)
    rec, head = codec.pack_sealed_info(buf)
    assert rec.n_members == 6 and rec.flags & 1 and head.container == "vpack"
    assert rec.content_bytes == sum(x.numel() * x.element_size() for x in xs)
    table = struct.unpack("<12I", buf[32: 32 + 8 * 6].cpu().numpy().tobytes())
    content, based = table[0::2], table[1::2]
    # the big member: the tiled content without its odd last byte, by CRC combines as tiled_crc; its base likewise
    assert content[0] == L.tiled_crc32(big.tile, big.k, big.tail[:-1])
    assert based[0] == L.tiled_crc32(L.rotated(big.tile), big.k, big.tail[:-1])
    for m in range(1, 6):
        assert content[m] == crc_of(xs[m]), m
        assert based[m] == (crc_of(bases[m]) if bases[m] is not None else 0), m
    outs, status, mc, bc = codec.decompress_pack_sealed(buf, dts, bases=bases)
    assert not bool(status.any()) and mc.tolist() == [0] * 6 and bc.tolist() == [0] * 6
    for m, (o, x) in enumerate(zip(outs, xs)):
        same_bytes(torch, o, x, f"sealed pack member {m}")
    del outs, buf, bases
    free(torch)


def test_sealed_pack_refuses_a_wrong_base(big):
    """A base that differs in one byte above offset 2^32: the member is named
    in base_check and no destination byte is stored."""
    torch = big.torch
    codec = codec_for()
    xs, bases = pack_members(big)
    bases[0] = elems(big, 2, rotated_base(big))
    dts = [x.dtype for x in xs]
    buf = codec.compress_pack_sealed(xs, bases=bases)
    # a wrong base for the big member, one byte above offset 2^32: named, and nothing is stored
    wrong = bases[0].clone()
    wrong.view(torch.uint8)[AT32 + 12345] ^= 1
    dest = [torch.full_like(x, 7) for x in xs]
    before = [d.clone() for d in dest[1:]]
    outs, status, mc, bc = codec.decompress_pack_sealed(buf, dts, bases=[wrong] + bases[1:], outs=dest)
    assert bc.tolist() == [CHECKSUM, 0, 0, 0, 0, 0]
    assert bool((dest[0] == 7).all())
    for m, (d, q) in enumerate(zip(dest[1:], before), 1):
        same_bytes(torch, d, q, f"destination {m} after a refused decode")
    del buf, outs, dest, wrong, bases
    free(torch)


# ---------------------------------------------------------------- h. the estimate
def test_estimate_and_auto(big):
    torch = big.torch
    codec = codec_for()
    # exact, as tests/test_gpu_estimate.py compares at small sizes
    assert codec.estimate(big.src)["frame"] == L.tiled_estimate(big.tile, big.k, big.tail, BLOCK, CKPT, 2)
    x = elems(big, 2)
    buf, kind = codec.compress_auto(x)
    direct = {"frame": lambda t: codec.compress_frame(t.view(torch.uint8)), "planes": codec.compress_planes,
              "delta": codec.compress_delta}[kind](x)
    est = codec.estimate(x)
    assert kind == min(("frame", "planes", "delta"), key=lambda name: est[name])
    same_bytes(torch, buf, direct, f"compress_auto against compress_{kind}")
    del buf, direct
    free(torch)


def test_peak_memory_is_under_the_cap(big):
    peak = big.torch.cuda.max_memory_allocated()
    print(f"\ntest_gpu_large: torch.cuda.max_memory_allocated = {peak} bytes = {peak / 2 ** 30:.1f} GiB")
    assert peak < CAP
