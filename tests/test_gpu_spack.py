"""The member check record and the sealed pack on the GPU (include/fsehip.h
section 2l): records of members carved from poisoned arenas at element
alignment only against tests/spack_ref.py (zlib.crc32), the unit, combine and
grid boundaries, 3,000 members, sealed pack bytes against the reference at
both frame formats with and without bases, reference-built sealed packs
decoded on the device, the wrong base that must leave a checkpoint untouched,
damage to payload, header and table, the host forms, stream order and the
call-level statuses.  Expected bytes never come from the code under test;
outputs sit between the guard bands of tests/test_gpu_guard_bands.py or
inside a poisoned arena compared whole."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import delta_ref as DR
import frame_ref as R
import spack_ref as SR
import vpack_ref as VR
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_pack import (SRC_POISON, codec_for, dev_u8, device_sidecars, lib, member_data, stream_of,
                           torch_cuda, torch_int)  # noqa: F401  (torch_cuda: the fixture)
from test_gpu_stream_order import behind_gate, same, warm  # noqa: F401  (warm: the fixture)
from test_gpu_vpack import (VArena, VpackChain, base_arena, base_for, base_raws_of, device_tensors, mixed_members, offs_of, on_device,
                            raws_of, shaped_members)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
OK, CHECKSUM, BAD_FRAME = SR.OK, SR.CHECKSUM, SR.BAD_FRAME
BAD_ARG, DST_TOO_SMALL, UNSUPPORTED = -11, -7, -14
BLOCK, CKPT = 4096, 128
UNIT = 65536
COUNTS = [0, 1, 15, 16, 17, 31, 33, 65535, 65536, 65537, 131077]  # member byte counts
SERIAL_UNITS = 64   # the combine's thread-versus-workgroup threshold (kMcheckSerialUnits)
GRID_UNITS = 8192   # the units the capped grid's waves take in one pass: 2,048 workgroups of 4 waves


# ---------------------------------------------------------------- records
def build_record(torch, members, offs=None, with_bases=True):
    """fsehip_mcheck_build of members and bases in two poisoned source arenas: (record bytes, arena, base arena)."""
    specs = VR.specs_of(members)
    arena, bases = VArena(torch, specs, SRC_POISON, offs, raws_of(members)), base_arena(torch, members, offs)
    arr, n = arena.members(), len(specs)
    need = lib().fsehip_mcheck_scratch_bytes(arr, n, None, 0, int(with_bases))
    assert need
    sw, scratch = g8(torch, need)
    rw, whole = g8(torch, 1 + SR.record_bytes(n))
    rec = whole[1:]  # an odd address
    rc = lib().fsehip_mcheck_build(arr, bases.pointers() if with_bases else None, n, ptr(rec), ptr(scratch),
                                   scratch.numel(), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(sw, scratch, A5, "d_scratch")
    assert_guards(rw, whole, A5, "d_record")
    assert int(whole[0]) == A5, "a store below the record"
    same(arena.dev.cpu().numpy(), arena.host, "the source arena")
    same(bases.dev.cpu().numpy(), bases.host, "the base arena")
    return bytes(rec.cpu().numpy()), arena, bases


def verify_record(torch, record, arena, which, ptrs=None, sel=None):
    """fsehip_mcheck_verify of a record given as bytes against the arena's members: (statuses, result)."""
    from entropy_coders_amd import _lib

    info = _lib.McheckInfo()
    assert lib().fsehip_mcheck_read_header(record, len(record), C.byref(info)) == 0
    arr, n = arena.members(), len(arena.specs)
    selarr = None if sel is None else (C.c_uint32 * max(len(sel), 1))(*sel)
    count = n if sel is None else len(sel)
    need = lib().fsehip_mcheck_scratch_bytes(arr, n, selarr, 0 if sel is None else len(sel), 0)
    sw, scratch = g8(torch, need)
    tw, st = g32(torch, count)
    rw, res = g32(torch, 2)
    drec = dev_u8(torch, np.frombuffer(record, np.uint8))
    rc = lib().fsehip_mcheck_verify(C.byref(info), ptr(drec), arr, selarr, 0 if sel is None else len(sel), which, ptrs,
                                    ptr(scratch), scratch.numel(), ptr(st), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (tw, st, F32, "d_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return st.cpu().numpy(), res.tolist()


def counted_members(seed, w):
    """Members of width w whose byte counts are COUNTS rounded down and up to whole elements, diff and planes
    alternating, every diff member with its own base."""
    rng = np.random.default_rng(seed)
    out = []
    for c in COUNTS:
        for n in sorted({c // w, -(-c // w)}):
            kind = ("diff", "planes")[len(out) % 2]
            a = rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])
            out.append((kind, a, base_for(rng, a) if kind == "diff" else None))
    return out


@gpu
@pytest.mark.parametrize("w", VR.WIDTHS)
def test_record_against_the_reference(torch_cuda, w):
    """Byte counts round the 16-byte word and the 64 KiB unit at every width, element alignment only."""
    members = counted_members(0x5EA1 + w, w)
    specs = VR.specs_of(members)
    offs = [w * (m % (16 // w)) for m in range(len(specs))]
    got, arena, bases = build_record(torch_cuda, members, offs)
    assert got == SR.record(members, True)
    got0, _, _ = build_record(torch_cuda, members, offs, with_bases=False)
    assert got0 == SR.record(members, False)
    st, res = verify_record(torch_cuda, got, arena, 0)
    assert res == [OK, 0] and not st.any()
    st, res = verify_record(torch_cuda, got, arena, 1, bases.pointers())
    assert res == [OK, 0] and not st.any()
    # the contents held against the bases' entries and the reverse: exactly the spans that differ fail
    mst, bst = SR.verify(SR.table(members, True), SR.BASES, specs, base_raws_of(members), raws_of(members))
    st, res = verify_record(torch_cuda, got, arena, 1, (C.c_void_p * len(specs))(*[
        (arena.dev.data_ptr() + p) if k == "diff" and n else None for (k, _, n), p in zip(specs, arena.pos)]))
    assert st.tolist() == bst and res == [CHECKSUM if any(bst) else OK, sum(s != 0 for s in bst)]
    sel = [m for m in range(len(specs)) if m % 3 == 1][::-1]
    st, res = verify_record(torch_cuda, got, arena, 0, None, sel)
    assert res == [OK, 0] and st.size == len(sel) and not st.any()


@gpu
def test_every_pointer_alignment_at_one_byte_elements(torch_cuda):
    """w = 1: the pointer mod 16 takes all 16 values, at sizes below, at and above a unit."""
    rng = np.random.default_rng(0xA11)
    sizes = [1, 15, 16, 17, 33, UNIT - 1, UNIT, UNIT + 1] * 2
    members = []
    for i, n in enumerate(sizes):
        a = rng.integers(0, 256, n + i, dtype=np.uint8)
        members.append(("diff", a, base_for(rng, a)))
    got, _, _ = build_record(torch_cuda, members, list(range(16)))
    assert got == SR.record(members, True)


@gpu
def test_the_combine_threshold(torch_cuda):
    """Members of one unit fewer than, exactly and one more than the units a single thread combines, ragged and
    whole last units, between small members."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(0x7E5)
    sizes = [5, (SERIAL_UNITS - 1) * UNIT - 5, 70000, SERIAL_UNITS * UNIT, 0, SERIAL_UNITS * UNIT + 1,
             (SERIAL_UNITS + 1) * UNIT, 33]
    xs = [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g) for n in sizes]
    codec = codec_for()
    rec = bytes(codec.mcheck_build(xs).cpu().numpy())
    want = SR.header(len(xs), sum(sizes)) + b"".join(
        struct.pack("<II", zlib.crc32(x.cpu().numpy().tobytes()) if x.numel() else 0, 0) for x in xs)
    assert rec == want


@gpu
def test_more_units_than_the_capped_grid(torch_cuda):
    """One member of 8,200 units and 77 bytes: the waves' second pass, the combine's third chunk; a small member
    behind it starts at unit 8,201."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(0x8200)
    n = (GRID_UNITS + 8) * UNIT + 77
    big = torch.randint(0, 256, (n + 1,), dtype=torch.uint8, device="cuda", generator=g)[1:]  # an odd address
    small = torch.randint(0, 256, (3000,), dtype=torch.int16, device="cuda", generator=g)
    codec = codec_for()
    rec = bytes(codec.mcheck_build([big, small]).cpu().numpy())
    want = SR.header(2, n + 6000) + struct.pack("<IIII", zlib.crc32(big.cpu().numpy().tobytes()), 0,
                                                zlib.crc32(small.cpu().numpy().tobytes()), 0)
    assert rec == want


def many_members(seed=0x3001, count=3000):
    rng = np.random.default_rng(seed)
    members = []
    for m in range(count):
        kind, w = ("diff", "delta", "planes")[int(rng.integers(3))], int(rng.choice(VR.WIDTHS))
        a = member_data(rng, "delta" if kind == "delta" else "planes", w, int(rng.integers(0, 41))).view(DR.UINT[w])
        members.append((kind, a, base_for(rng, a) if kind == "diff" else None))
    return members


@gpu
def test_many_members(torch_cuda):
    """3,000 members of 0 to 40 elements: the record, and the sealed pack's bytes and decode."""
    torch = torch_cuda
    members = many_members()
    specs = VR.specs_of(members)
    rng = np.random.default_rng(5)
    offs = [int(rng.integers(16 // w)) * w for _, w, _ in specs]
    got, _, _ = build_record(torch, members, offs)
    assert got == SR.record(members, True)
    codec = codec_for(65536, 128, 2)
    xs, kinds, bs = on_device(torch, members)
    buf = codec.compress_pack_sealed(xs, kinds, bases=bs)
    img = VR.image(members)
    want = SR.build(members, 65536, 128, 2, sidecars=device_sidecars(torch, codec, img))
    same(buf.cpu().numpy(), np.frombuffer(want, np.uint8), "sealed pack of 3,000 members")
    outs, st, mc, bc, cres = codec.decompress_pack_sealed(buf, [x.dtype for x in xs], bases=bs, with_result=True)
    assert cres.tolist() == [0, 0, 0, 0] and not bool(st.any()) and not bool(mc.any()) and not bool(bc.any())
    assert all(torch.equal(o, x) for o, x in zip(outs, xs))


# ---------------------------------------------------------------- sealed pack bytes
BYTES_MEMBERS = [0, 1, 17, 300, 4097, 20011]


@gpu
@pytest.mark.parametrize("nstates,ckpt,block,offset", [(2, 128, 65536, 0), (1, 0, 1040, 1)])
@pytest.mark.parametrize("form", ["bases", "no-base-crcs", "pack"])
def test_bytes_against_the_reference(torch_cuda, nstates, ckpt, block, offset, form):
    """Device sealed packs equal the reference's byte for byte, at an odd buffer address too, guard bands round
    every output, and decode on both sides."""
    torch = torch_cuda
    codec = codec_for(block, ckpt, nstates)
    members = mixed_members(0xB17E6 + block + nstates, BYTES_MEMBERS)
    if form == "pack":
        members = [("planes" if k == "diff" else k, a, None) for k, a, _ in members]
    versioned = form != "pack"
    xs, kinds, bs = on_device(torch, members)
    img = VR.image(members)
    want = SR.build(members, block, ckpt, nstates, sidecars=device_sidecars(torch, codec, img), versioned=versioned,
                    check_bases=form == "bases")
    barr = None
    if versioned:
        kinds, barr = codec.pack_bases(xs, bs, kinds)
    arr, n = codec.pack_members(xs, kinds, versioned=versioned), len(xs)
    cap = codec.pack_sealed_bound(arr, n, versioned)
    assert cap == SR.record_bytes(n) + VR.bound(VR.specs_of(members), block) and len(want) <= cap
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.pack_sealed_scratch_bytes(arr, n, versioned))
    codec.compress_pack_sealed_into(arr, n, scratch, out, out_len, res, bases=barr, check_bases=form == "bases")
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0, (out_len.tolist(), len(want), res.tolist())
    same(out[: len(want)].cpu().numpy(), np.frombuffer(want, np.uint8), "sealed pack bytes")
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the sealed pack"
    from entropy_coders_amd import container_kind

    assert container_kind(out) == "spack"
    rec, head = codec.pack_sealed_info(out[: len(want)])
    f, tab, v, _ = SR.parse(want)
    assert (rec.flags, rec.n_members, rec.content_bytes, rec.header_crc) == (
        f["flags"], f["n_members"], f["content_bytes"], f["header_crc"])
    assert head.container == ("vpack" if versioned else "pack") and v == versioned
    outs, st, mc, bc = codec_for().decompress_pack_sealed(out[: len(want)], [x.dtype for x in xs],
                                                          bases=bs if versioned else None)
    assert not bool(st.any()) and not bool(mc.any()) and not bool(bc.any())
    assert all(torch.equal(o, x) for o, x in zip(outs, xs))


@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, 128), (1, 0)])
def test_reference_sealed_packs_decode_on_the_device(torch_cuda, nstates, ckpt):
    torch = torch_cuda
    members = mixed_members(0x4F0 + nstates + ckpt, [0, 1, 17, 4097, 9000])
    blob = SR.build(members, BLOCK, ckpt, nstates)
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    bs = device_tensors(torch, [b for _, _, b in members])
    outs, st, mc, bc = codec_for().decompress_pack_sealed(buf, [torch_int(torch, a.itemsize) for _, a, _ in members],
                                                          bases=bs)
    assert not bool(st.any()) and not bool(mc.any()) and not bool(bc.any())
    for o, (_, a, _) in zip(outs, members):
        assert bytes(o.view(torch.uint8).cpu().numpy()) == a.tobytes()


# ---------------------------------------------------------------- the raw decode call, into arenas
@pytest.fixture(scope="module")
def ref_spack():
    """A reference-built sealed versioned pack at 4 KiB blocks: (members, bytes)."""
    members = shaped_members(0x5E1EC8)
    return members, SR.build(members, BLOCK, CKPT, 2)


def sealed_decode_call(torch, blob, members, good=None, in_place=False, other_bases=None, sel=None):
    """fsehip_spack_decompress (sel: _members) of host bytes, the head read from `good` (default: the bytes
    themselves), into a poisoned arena; bases in an arena of their own or (in_place) at the diff members'
    destinations: (arena, base arena | None, statuses, result, member_check, base_check, check_result)."""
    from entropy_coders_amd import BlockCodec

    rec, head = BlockCodec.pack_sealed_info(blob if good is None else good)
    versioned = head.container == "vpack"
    specs = VR.specs_of(members)
    n = len(specs)
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
    if not versioned:
        barr = None
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    arr = arena.members(None if sel is None else set(sel))
    L = lib()
    count = n if sel is None else len(sel)
    rw, res = g32(torch, 2)
    mw, mc = g32(torch, count)
    bw, bc = g32(torch, count)
    cw, cres = g32(torch, 4)
    if sel is None:
        sw, scratch = g8(torch, L.fsehip_spack_scratch_bytes(arr, n, int(versioned)))
        tw, st = g32(torch, head.inner.n_blocks)
        rc = L.fsehip_spack_decompress(C.byref(rec), C.byref(head.info), int(versioned), arr, barr, C.byref(head.inner),
                                       0, ptr(buf), buf.numel(), ptr(scratch), scratch.numel(), ptr(st), ptr(res),
                                       ptr(mc), ptr(bc), ptr(cres), stream_of(torch))
    else:
        selarr = (C.c_uint32 * max(len(sel), 1))(*sel)
        sw, scratch = g8(torch, max(L.fsehip_spack_members_scratch_bytes(arr, n, int(versioned), selarr, len(sel)), 16))
        tw, st = g32(torch, count)
        rc = L.fsehip_spack_decompress_members(C.byref(rec), C.byref(head.info), int(versioned), arr, barr,
                                               C.byref(head.inner), 0, ptr(buf), buf.numel(), selarr, len(sel),
                                               ptr(scratch), scratch.numel(), ptr(st), ptr(res), ptr(mc), ptr(bc),
                                               ptr(cres), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((sw, scratch, A5, "d_scratch"), (tw, st, F32, "statuses"), (rw, res, F32, "d_result"),
                           (mw, mc, F32, "d_member_check"), (bw, bc, F32, "d_base_check"),
                           (cw, cres, F32, "d_check_result")):
        assert_guards(w_, v, f, what)
    if bases is not None:
        same(bases.dev.cpu().numpy(), bases.host, "the base arena after an out-of-place decode")
    return arena, bases, st.cpu().numpy(), res.tolist(), mc.cpu().numpy(), bc.cpu().numpy(), cres.tolist()


@gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_decode_into_arenas(torch_cuda, ref_spack, in_place):
    members, blob = ref_spack
    arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, blob, members, in_place=in_place)
    assert res == [0, 0] and not st.any() and not mc.any() and not bc.any() and cres == [0, 0, 0, 0]
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the arena after the sealed decode")
    sel = [5, 0, 3, 8]
    arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, blob, members, in_place=in_place, sel=sel)
    assert res == [0, 0] and not st.any() and not mc.any() and not bc.any() and cres == [0, 0, 0, 0]
    want = arena.host.copy()  # in place the arena held every diff member's base: the unselected ones' stay
    for m in sel:
        raw = raws_of(members)[m]
        want[arena.pos[m]: arena.pos[m] + raw.size] = raw
    same(arena.dev.cpu().numpy(), want, "the arena after the selected decode")


def one_byte_off(members, m):
    """The bases with member m's differing in a single byte."""
    out = []
    for i, (_, _, b) in enumerate(members):
        if i == m:
            raw = VR.raw_bytes(b).copy()
            raw[raw.size // 2] ^= 0x10
            b = raw.view(b.dtype)
        out.append(b)
    return out


@gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_a_wrong_base_stores_nothing(torch_cuda, ref_spack, in_place):
    """One diff member's base differs in a single byte (CRC-32 detects any single-byte change): that member's base
    check alone is CHECKSUM, and the whole arena -- with outs = bases the old checkpoint -- is byte for byte what
    it was; the same through the members call with only that member selected."""
    members, blob = ref_spack
    wrong = 5
    other = one_byte_off(members, wrong)
    for sel in (None, [wrong]):
        arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, blob, members, in_place=in_place,
                                                            other_bases=other, sel=sel)
        idx = list(range(len(members))) if sel is None else sel
        assert res == [0, 0] and not st.any(), (res, st)  # the pack itself is sound
        assert bc.tolist() == [CHECKSUM if m == wrong else OK for m in idx], bc
        same(arena.dev.cpu().numpy(), arena.host, "a failed base must leave every destination untouched")
        # what lies at the destinations is not the recorded content, except where there is none
        assert mc.tolist() == [OK if VR.specs_of(members)[m][2] == 0 else CHECKSUM for m in idx], mc
        assert cres == [CHECKSUM, sum(s != 0 for s in mc.tolist()), 1, 0], cres


@gpu
def test_a_wrong_base_without_base_crcs(torch_cuda):
    """check_bases=False: the base check has nothing to compare and says OK, the merge runs, and the member's
    content check after it is CHECKSUM -- that member alone."""
    members = shaped_members(0x5E1EC8)
    blob = SR.build(members, BLOCK, CKPT, 2, check_bases=False)
    wrong = 5
    arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, blob, members,
                                                        other_bases=one_byte_off(members, wrong))
    assert res == [0, 0] and not st.any() and not bc.any()
    assert mc.tolist() == [CHECKSUM if m == wrong else OK for m in range(len(members))]
    assert cres == [CHECKSUM, 1, 0, 0]
    raws = raws_of(members)
    got = arena.dev.cpu().numpy()
    for m, (p, raw) in enumerate(zip(arena.pos, raws)):
        if m != wrong:
            same(got[p: p + raw.size], raw, f"member {m}")


# ---------------------------------------------------------------- damage
def flip(b, at, mask=0x01):
    return b[:at] + bytes([b[at] ^ mask]) + b[at + 1:]


@pytest.fixture(scope="module")
def raw_spack():
    """Uniform random members, so every block of the inner frame is RAW: (members, bytes)."""
    rng = np.random.default_rng(0xDA3A6E)
    members = []
    for k, w, n in [("planes", 1, 5000), ("diff", 2, 3000), ("planes", 4, 1025), ("diff", 8, 700), ("planes", 2, 0),
                    ("diff", 1, 4096)]:
        a = rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w])
        b = rng.integers(0, 256, n * w, dtype=np.uint8).view(DR.UINT[w]) if k == "diff" else None
        members.append((k, a, b))
    blob = SR.build(members, BLOCK, CKPT, 2)
    inner = blob[SR.record_bytes(len(members)) + 32 + 16 * len(members):]
    assert set(R.types_of(inner)) == {R.RAW}
    return members, blob


@gpu
def test_a_flipped_payload_byte_is_checksum_of_its_member(torch_cuda, raw_spack):
    """RAW blocks decode whatever they hold: every block status is OK, and exactly the member with a byte there
    fails its content check."""
    members, good = raw_spack
    specs = VR.specs_of(members)
    n = len(specs)
    head = SR.record_bytes(n) + 32 + 16 * n
    finfo, directory, records = R.split_frame(good[head:])
    offsets = VR.plane_offsets(specs)
    for target, k in ((0, 0), (2, 3), (3, 0), (5, 0)):
        img_at = offsets[target][k] + specs[target][2] // 2  # a byte of plane k of the member
        at = head + finfo["records_off"] + img_at  # RAW records hold the image's bytes back to back
        bad = flip(good, at, 0x40)
        arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, bad, members, good=good)
        assert res == [0, 0] and not st.any() and not bc.any(), (res, st, bc)
        assert mc.tolist() == [CHECKSUM if m == target else OK for m in range(n)], (target, mc)
        assert cres == [CHECKSUM, 1, 0, 0]
        arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, bad, members, good=good, sel=[target, 1])
        assert res == [0, 0] and mc.tolist() == [CHECKSUM, OK] and cres == [CHECKSUM, 1, 0, 0]


@gpu
@pytest.mark.parametrize("at", [0, 4, 6, 9, 17, 29])
def test_a_flipped_record_header_byte_is_bad_frame_everywhere(torch_cuda, raw_spack, at):
    members, good = raw_spack
    n = len(members)
    for sel in (None, [3, 0]):
        count = n if sel is None else len(sel)
        arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, flip(good, at), members, good=good, sel=sel)
        assert (mc == BAD_FRAME).all() and (bc == BAD_FRAME).all() and cres == [BAD_FRAME, count, count, 0], cres
        same(arena.dev.cpu().numpy(), arena.host, "a record that is not the caller's must leave every destination alone")


@gpu
def test_a_flipped_table_entry_is_checksum_of_that_member_alone(torch_cuda, raw_spack):
    members, good = raw_spack
    n = len(members)
    arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, flip(good, 32 + 8 * 2 + 1), members, good=good)
    assert res == [0, 0] and not st.any() and not bc.any()
    assert mc.tolist() == [CHECKSUM if m == 2 else OK for m in range(n)] and cres == [CHECKSUM, 1, 0, 0]
    same(arena.dev.cpu().numpy(), arena.expect(raws_of(members)), "the members are sound: only the entry is not")
    # a base entry: the failed base closes the gate
    arena, _, st, res, mc, bc, cres = sealed_decode_call(torch_cuda, flip(good, 32 + 8 * 3 + 6), members, good=good)
    assert bc.tolist() == [CHECKSUM if m == 3 else OK for m in range(n)] and cres[0] == CHECKSUM and cres[2] == 1
    same(arena.dev.cpu().numpy(), arena.host, "a failed base must leave every destination untouched")


# ---------------------------------------------------------------- Python forms
@gpu
def test_python_forms(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    members = shaped_members(0x9A7)
    xs, kinds, bs = on_device(torch, members)
    buf = codec.compress_pack_sealed(xs, kinds, bases=bs)
    assert bytes(buf.cpu().numpy()) == SR.build(
        members, BLOCK, CKPT, 2, sidecars=device_sidecars(torch, codec, VR.image(members)))
    # in place: outs = bases updates the old checkpoint
    olds = [b.clone() if b is not None else torch.empty_like(x) for b, x in zip(bs, xs)]
    outs, st, mc, bc = codec.decompress_pack_sealed(buf, [x.dtype for x in xs], bases=[
        o if b is not None else None for o, b in zip(olds, bs)], outs=olds)
    assert all(o is q for o, q in zip(outs, olds)) and all(torch.equal(o, x) for o, x in zip(outs, xs))
    assert not bool(mc.any()) and not bool(bc.any())
    # a wrong old checkpoint: untouched
    olds = [b.clone() if b is not None else torch.full_like(x, 7) for b, x in zip(bs, xs)]
    olds[0][3] ^= 1
    before = [o.clone() for o in olds]
    outs, st, mc, bc, cres = codec.decompress_pack_sealed(buf, [x.dtype for x in xs], bases=[
        o if b is not None else None for o, b in zip(olds, bs)], outs=olds, with_result=True)
    assert bc.tolist()[0] == CHECKSUM and sum(s != 0 for s in bc.tolist()) == 1 and cres.tolist()[2] == 1
    assert all(torch.equal(o, q) for o, q in zip(olds, before))
    pick = [6, 0]
    outs, mst, mc, bc = codec.decompress_pack_members_sealed(buf, pick, [xs[m].dtype for m in pick],
                                                             bases={m: bs[m] for m in pick})
    assert not bool(mst.any()) and not bool(mc.any()) and not bool(bc.any())
    assert all(torch.equal(o, xs[m]) for o, m in zip(outs, pick))
    rec = codec.mcheck_build(xs, bases=bs, kinds=kinds)
    assert torch.equal(rec, buf[: rec.numel()])


@gpu
def test_host_forms(torch_cuda):
    from entropy_coders_amd import (FseError, container_kind, pack_decompress, pack_sealed_compress,
                                    pack_sealed_decompress, pack_sealed_info)

    rng = np.random.default_rng(11)
    arrays = [np.arange(5000, dtype=np.int64) * 7, rng.normal(0, 1, 3000).astype(np.float32), np.zeros(0, np.int16),
              np.arange(100, dtype=np.uint8)]
    bases = [arrays[0] - 3, None, None, (arrays[3] + 1).astype(np.uint8)]
    blob = pack_sealed_compress(arrays, bases=bases, block_size=BLOCK)
    assert container_kind(blob) == "spack"
    members = [("diff", arrays[0].view(np.uint64), bases[0].view(np.uint64)), ("planes", arrays[1].view(np.uint32), None),
               ("planes", arrays[2].view(np.uint16), None), ("diff", arrays[3], bases[3])]
    assert blob[: SR.record_bytes(4)] == SR.record(members, True)
    rec, head = pack_sealed_info(blob)
    assert rec.flags == 1 and head.container == "vpack" and head.n_elems == [5000, 3000, 0, 100]
    back = pack_sealed_decompress(blob, [a.dtype for a in arrays], bases=bases)
    assert all(b.dtype == a.dtype and np.array_equal(b, a) for a, b in zip(arrays, back))
    wrong = list(bases)
    wrong[3] = bases[3].copy()
    wrong[3][50] ^= 4
    with pytest.raises(FseError, match=r"base of member\(s\) \[3\]") as e:
        pack_sealed_decompress(blob, [a.dtype for a in arrays], bases=wrong)
    assert e.value.code == "CHECKSUM"
    table_hit = flip(blob, 32 + 8 * 1, 0x80)
    with pytest.raises(FseError, match=r"content of member\(s\) \[1\]") as e:
        pack_sealed_decompress(table_hit, [a.dtype for a in arrays], bases=bases)
    assert e.value.code == "CHECKSUM"
    with pytest.raises(FseError) as e:  # every existing reader refuses the new magic
        pack_decompress(blob, [a.dtype for a in arrays], bases=bases)
    assert e.value.code == "BAD_FRAME"
    plain = pack_sealed_compress(arrays[1:3], block_size=BLOCK)
    rec, head = pack_sealed_info(plain)
    assert rec.flags == 0 and head.container == "pack"
    back = pack_sealed_decompress(plain, [a.dtype for a in arrays[1:3]])
    assert all(np.array_equal(b, a) for a, b in zip(arrays[1:3], back))


# ---------------------------------------------------------------- call-level statuses
@gpu
def test_call_level_statuses(torch_cuda, ref_spack):
    from entropy_coders_amd import BlockCodec, _lib

    torch = torch_cuda
    L = lib()
    members, blob = ref_spack
    specs = VR.specs_of(members)
    n = len(specs)
    arena, bases = VArena(torch, specs, SRC_POISON, offs_of(specs), raws_of(members)), base_arena(torch, members)
    arr, barr = arena.members(), bases.pointers()
    s = stream_of(torch)
    scratch = torch.empty(L.fsehip_spack_scratch_bytes(arr, n, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty(L.fsehip_spack_bound(arr, n, 1, BLOCK), dtype=torch.uint8, device="cuda")
    ln, res = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    p = _lib.FrameParams(BLOCK, 0, CKPT, 0, 2, 0)
    before = arena.dev.clone()

    def compress(p_=p, arr_=arr, barr_=barr, sc=scratch, cap=None, o=out, ocap=None):
        return L.fsehip_spack_compress(C.byref(p_) if p_ else None, arr_, n, barr_, 1, ptr(sc) if sc is not None else None,
                                       sc.numel() if cap is None else cap, ptr(o), o.numel() if ocap is None else ocap,
                                       ptr(ln), ptr(res), s)

    assert compress(p_=None) == BAD_ARG
    assert compress(sc=scratch[1:]) == BAD_ARG
    assert compress(cap=scratch.numel() - 1) == DST_TOO_SMALL
    assert compress(ocap=out.numel() - 1) == DST_TOO_SMALL
    assert compress(barr_=None) == UNSUPPORTED  # diff members in front of a pack frame
    nobase = bases.pointers()
    nobase[0] = None
    assert compress(barr_=nobase) == BAD_ARG
    odd = arena.members()
    odd[0].d_ptr += 1
    assert compress(arr_=odd) == BAD_ARG
    badkind = arena.members()
    badkind[1].kind = 3
    assert compress(arr_=badkind) == UNSUPPORTED
    assert compress(p_=_lib.FrameParams(1 << 29, 0, CKPT, 0, 2, 0)) == UNSUPPORTED

    rec_scratch = torch.empty(L.fsehip_mcheck_scratch_bytes(arr, n, None, 0, 1), dtype=torch.uint8, device="cuda")
    record = torch.empty(SR.record_bytes(n), dtype=torch.uint8, device="cuda")
    assert L.fsehip_mcheck_build(arr, barr, n, None, ptr(rec_scratch), rec_scratch.numel(), s) == BAD_ARG
    assert L.fsehip_mcheck_build(arr, barr, n, ptr(record), ptr(rec_scratch), rec_scratch.numel() - 1, s) == DST_TOO_SMALL
    assert L.fsehip_mcheck_build(arr, nobase, n, ptr(record), ptr(rec_scratch), rec_scratch.numel(), s) == BAD_ARG
    assert L.fsehip_mcheck_build(badkind, barr, n, ptr(record), ptr(rec_scratch), rec_scratch.numel(), s) == UNSUPPORTED

    rec, head = BlockCodec.pack_sealed_info(blob)
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    st = torch.zeros(head.inner.n_blocks, dtype=torch.int32, device="cuda")
    mc, bc = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    cres = torch.zeros(4, dtype=torch.int32, device="cuda")
    dst = VArena(torch, specs, A5, offs_of(specs))
    darr = dst.members()

    def decompress(rec_=rec, arr_=darr, barr_=barr, cap=None, cres_=cres, versioned=1, info=head.info):
        return L.fsehip_spack_decompress(C.byref(rec_), C.byref(info), versioned, arr_, barr_, C.byref(head.inner), 0,
                                         ptr(buf), buf.numel(), ptr(scratch), scratch.numel() if cap is None else cap,
                                         ptr(st), ptr(res), ptr(mc), ptr(bc), ptr(cres_) if cres_ is not None else None, s)

    assert decompress(cres_=None) == BAD_ARG
    other = _lib.McheckInfo.from_buffer_copy(rec)
    other.n_members += 1
    assert decompress(rec_=other) == BAD_ARG
    other = _lib.McheckInfo.from_buffer_copy(rec)
    other.content_bytes += 1
    assert decompress(rec_=other) == BAD_ARG
    other = _lib.McheckInfo.from_buffer_copy(rec)
    other.flags = 2
    assert decompress(rec_=other) == BAD_ARG
    assert decompress(versioned=0) == BAD_ARG  # base CRCs in front of a pack frame
    assert decompress(cap=scratch.numel() - 1) == DST_TOO_SMALL
    assert decompress(barr_=nobase) == BAD_ARG
    overlap = dst.members()
    overlap[1].d_ptr = overlap[0].d_ptr
    assert decompress(arr_=overlap) == BAD_ARG
    sel = (C.c_uint32 * 2)(1, 1)
    msc = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = L.fsehip_spack_decompress_members(C.byref(rec), C.byref(head.info), 1, darr, barr, C.byref(head.inner), 0,
                                           ptr(buf), buf.numel(), sel, 2, ptr(msc), msc.numel(), ptr(st), ptr(res),
                                           ptr(mc), ptr(bc), ptr(cres), s)
    assert rc == BAD_ARG
    info = _lib.McheckInfo()
    vsel = (C.c_uint32 * 1)(n)
    assert L.fsehip_mcheck_read_header(blob, 32, C.byref(info)) == 0
    assert L.fsehip_mcheck_verify(C.byref(info), ptr(buf), darr, vsel, 1, 0, None, ptr(rec_scratch), rec_scratch.numel(),
                                  ptr(mc), ptr(res), s) == BAD_ARG
    assert L.fsehip_mcheck_verify(C.byref(info), ptr(buf), darr, None, 0, 2, None, ptr(rec_scratch), rec_scratch.numel(),
                                  ptr(mc), ptr(res), s) == BAD_ARG
    assert L.fsehip_mcheck_verify(C.byref(info), ptr(buf), darr, None, 0, 1, None, ptr(rec_scratch), rec_scratch.numel(),
                                  ptr(mc), ptr(res), s) == BAD_ARG  # diff members' bases are needed
    assert L.fsehip_mcheck_verify(C.byref(info), ptr(buf), darr, None, 0, 0, None, ptr(rec_scratch), 16,
                                  ptr(mc), ptr(res), s) == DST_TOO_SMALL
    torch.cuda.synchronize()
    assert torch.equal(arena.dev, before) and bool((dst.dev == A5).all()), "a refused call touched device memory"


# ---------------------------------------------------------------- stream order
class SpackChain(VpackChain):
    """compress_pack_sealed -> decompress_pack_sealed (out of place) -> members (in place) on one stream with no host
    synchronisation, sources and bases poison until the gate opens: tests/test_gpu_vpack.py's chain with the record
    in front, so the base pass's three launches and the gate word run ahead of each merge in stream order."""

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        super().alloc(torch)  # with the versioned pack's bytes still in self.want: its head is read there
        self.want = SR.build(self.members, BLOCK, CKPT, 2)
        c, n = self.codec, len(self.specs)
        self.rec, self.head = BlockCodec.pack_sealed_info(self.want)
        assert self.rec.flags == SR.BASES and self.head.container == "vpack"
        self.scratch = torch.empty(c.pack_sealed_scratch_bytes(self.arr, n, True), dtype=torch.uint8, device="cuda")
        self.w_buf, self.buf = g8(torch, c.pack_sealed_bound(self.arr, n, True))
        self.mscratch = torch.empty(c.pack_sealed_members_scratch_bytes(self.arr, n, self.SEL, True), dtype=torch.uint8,
                                    device="cuda")
        self.checks = [g32(torch, k) for k in (n, n, 4, len(self.SEL), len(self.SEL), 4)]

    def poison(self):
        super().poison()
        for _, v in self.checks:
            v.fill_(F32)

    def enqueue(self, step9):
        c, t, n = self.codec, self.torch, len(self.specs)
        buf = self.buf[: len(self.want)]
        (_, mc), (_, bc), (_, cr), (_, smc), (_, sbc), (_, scr) = self.checks
        rc = c.lib.fsehip_vpack_split(self.arr, n, self.barr, ptr(self.img), ptr(self.scratch), self.scratch.numel(),
                                      stream_of(t))
        assert rc == 0, rc
        c.compress_pack_sealed_into(self.arr, n, self.scratch, self.buf, self.len, self.cres, bases=self.barr)
        c.decompress_pack_sealed_into(buf, self.rec, self.head, [v.view(torch_int(t, w)) for (_, v), (_, w, _) in
                                                                 zip(self.outs, self.specs)], self.scratch, self.bst,
                                      self.dres, mc, bc, cr, bases=self.bases)
        sel_views = [v.view(torch_int(t, self.specs[m][1])) for (_, v), m in zip(self.sel_outs, self.SEL)]
        for v, m in zip(sel_views, self.SEL):
            if self.bases[m] is not None:
                v.copy_(self.bases[m])  # on the stream, behind the upload: the members call decodes in place
        c.decompress_pack_members_sealed_into(
            buf, self.rec, self.head, self.SEL, sel_views, self.mscratch, self.mst, self.mres, smc, sbc, scr,
            bases={m: v for v, m in zip(sel_views, self.SEL) if self.bases[m] is not None})
        step9()

    def check(self):
        super().check()
        for (w, v), name in zip(self.checks, ("member_check", "base_check", "check_result", "selected member_check",
                                              "selected base_check", "selected check_result")):
            assert_guards(w, v, F32, name)
            assert not bool(v.any()), (name, v.tolist())


@gpu
def test_sealed_pack_chain_behind_the_gate(torch_cuda, warm):
    """One sealed compress -> decompress -> members chain over a versioned pack with base CRCs behind the gate of
    tests/test_gpu_stream_order.py: every call returns while its inputs are still poison, so none of them waits
    for the stream or reads device data on the host."""
    chain = SpackChain()
    chain.alloc(torch_cuda)
    warm.chains["spack"] = chain
    warm.run(chain, gated=False)
    warm.enqueue_ms["spack"] = warm.run(chain, gated=False)
    behind_gate(warm, "spack")
