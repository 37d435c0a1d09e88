"""The check record and sealed buffers on the device (include/fsehip.h section
2f).  Expected records, sealed layouts and covered blocks come from
tests/check_ref.py (zlib.crc32 per block, the combine written out, the
containers of frame_ref / planes_ref / delta_ref), never from the library.
Every output sits between 256-byte guard bands.  Every case is at most a few
hundred KiB."""
import ctypes as C
import zlib

import numpy as np
import pytest

import check_ref as K
import frame_ref as R
import planes_ref as PR
from oracle import oracle as O
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
CHECKSUM, BAD_FRAME = K.CHECKSUM, K.BAD_FRAME
BLOCK, CKPT = 4096, 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def codec_for(block=BLOCK, ckpt=CKPT, nstates=2):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=block, ckpt_interval=ckpt, nstates=nstates)


def lib():
    from entropy_coders_amd import _lib

    return _lib.load()


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def info_of(rec):
    from entropy_coders_amd import BlockCodec

    return BlockCodec.check_info(bytes(rec[:32]))


def lengths(check_log):
    B = 1 << check_log
    return sorted({0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 5})


def content_of(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "ff":
        return np.full(n, 0xFF, dtype=np.uint8)
    return np.asarray(O.generate(0, 0.155, 0x5EED0C00 + seed, 0, n), dtype=np.uint8) if n else np.zeros(0, np.uint8)


# ---------------------------------------------------------------- build and verify against the reference
SLOT = 1024          # bytes of the record arena per case: 256 guard, the record at 256 + shift, guard to the end
SLOT32 = 256         # int32 of the status arena per case: 64 guard, 8 statuses, 64 guard, the result, guard


@gpu
@pytest.mark.parametrize("data", ["random", "zeros", "ff", "c2"])
@pytest.mark.parametrize("check_log", [8, 12, 16])
def test_build_and_verify_against_the_reference(torch_cuda, check_log, data):
    """Every length at every content offset 0..15, the record at every offset
    0..3: fsehip_check_build byte for byte, fsehip_check_verify clean, guard
    bands and content untouched.  All cases of one parameter are queued
    first (no synchronisation in between) and read back once."""
    torch = torch_cuda
    L, hs = lib(), stream_of(torch)
    ns = lengths(check_log)
    top = max(ns)
    host = content_of(data, top + 16, check_log)
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    cases = [(n, off, (i + off) % 4) for i, n in enumerate(ns) for off in range(16)]
    assert {c[2] for c in cases} == {0, 1, 2, 3}
    want = {(n, off): K.record(host[off: off + n].tobytes(), check_log) for n, off, _ in cases}
    assert max(len(w) for w in want.values()) + 3 + 512 <= SLOT
    arena = torch.full((len(cases) * SLOT,), A5, dtype=torch.uint8, device="cuda")
    st_arena = torch.full((len(cases) * SLOT32,), F32, dtype=torch.int32, device="cuda")
    assert arena.data_ptr() % 256 == 0
    for i, (n, off, shift) in enumerate(cases):
        rec = arena.data_ptr() + i * SLOT + 256 + shift
        rc = L.fsehip_check_build(check_log, C.c_void_p(src.data_ptr() + off), n, C.c_void_p(rec), hs)
        assert rc == 0, (n, off, shift, rc)
        info = info_of(want[n, off])
        # statuses at int32 64.., the result at 64 + 8 + 64 ..: 256-byte bands round each
        stp = st_arena.data_ptr() + 4 * (i * SLOT32 + 64)
        rc = L.fsehip_check_verify(C.byref(info), C.c_void_p(rec), C.c_void_p(src.data_ptr() + off), n,
                                   C.c_void_p(stp), C.c_void_p(stp + 4 * (8 + 64)), hs)
        assert rc == 0, (n, off, shift, rc)
    torch.cuda.synchronize()
    got, got32 = arena.cpu().numpy(), st_arena.cpu().numpy()
    same(src.cpu().numpy(), host, "the content")
    for i, (n, off, shift) in enumerate(cases):
        what = f"check_log {check_log} {data} n {n} content offset {off} record offset {shift}"
        w = np.frombuffer(want[n, off], dtype=np.uint8)
        slot = got[i * SLOT: (i + 1) * SLOT]
        lo = 256 + shift
        same(slot[lo: lo + len(w)], w, what)
        assert (slot[:lo] == A5).all() and (slot[lo + len(w):] == A5).all(), f"{what}: a store outside the record"
        s32 = got32[i * SLOT32: (i + 1) * SLOT32]
        n_cb = K.n_cb_of(n, check_log)
        assert n_cb <= 8
        assert s32[64: 64 + n_cb].tolist() == [0] * n_cb, (what, s32[64: 64 + n_cb])
        assert s32[136: 138].tolist() == [0, 0], (what, s32[136: 138])
        rest = np.concatenate([s32[:64], s32[64 + n_cb: 136], s32[138:]])
        assert (rest == F32).all(), f"{what}: a store outside the statuses"
    if data == "zeros":  # the init-handling trap: every length of zeros has a CRC of its own
        crcs = [K.parse(want[n, 0])["content_crc"] for n in ns if n]
        assert len(set(crcs)) == len(crcs)


def build_guarded(torch, content_dev, n, check_log):
    L = lib()
    w_rec, rec = g8(torch, K.record_bytes(n, check_log))
    assert L.fsehip_check_build(check_log, ptr(content_dev), n, ptr(rec), stream_of(torch)) == 0
    torch.cuda.synchronize()
    assert_guards(w_rec, rec, A5, "d_record")
    return rec


def verify_guarded(torch, info, rec, content_dev, n):
    L = lib()
    w_st, st = g32(torch, info.n_cb)
    w_res, res = g32(torch, 2)
    rc = L.fsehip_check_verify(C.byref(info), ptr(rec), ptr(content_dev), n, ptr(st), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(w_st, st, F32, "d_check_status")
    assert_guards(w_res, res, F32, "d_result")
    return st.cpu().numpy().tolist(), res.cpu().numpy().tolist()


@gpu
def test_combine_beyond_one_run_and_one_workgroup(torch_cuda):
    """2,049 check blocks of 256 bytes plus 7 bytes: the combine gives its
    threads runs of more than one entry, and there are more entries than the
    finish kernel has threads."""
    torch = torch_cuda
    n = 2049 * 256 + 7
    host = content_of("random", n + 3, 2049)[3:]
    whole = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), host])).cuda()
    content = whole[3:]
    want = K.record(host.tobytes(), 8)
    assert K.parse(want)["n_cb"] == 2050
    rec = build_guarded(torch, content, n, 8)
    same(rec.cpu().numpy(), np.frombuffer(want, dtype=np.uint8), "the record of 2,050 check blocks")
    st, res = verify_guarded(torch, info_of(want), rec, content, n)
    assert res == [0, 0] and not any(st)


@gpu
@pytest.mark.parametrize("check_log", [8, 12])
def test_verify_names_the_damaged_block(torch_cuda, check_log):
    torch = torch_cuda
    B = 1 << check_log
    n = 3 * B + 5
    host = content_of("c2", n, 77)
    want = K.record(host.tobytes(), check_log)
    info = info_of(want)
    rec = dev_u8(torch, np.frombuffer(want, dtype=np.uint8))
    base = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    content = base[3: 3 + n]  # an odd address
    for at in (0, n - 1, B - 1, B, 2 * B - 1, 2 * B, 3 * B - 1, 3 * B):
        damaged = host.copy()
        damaged[at] ^= 1 << (at % 8)
        content.copy_(torch.from_numpy(damaged))
        st, res = verify_guarded(torch, info, rec, content, n)
        assert st == [CHECKSUM if b == at // B else 0 for b in range(4)], (at, st)
        assert res == [CHECKSUM, 1], (at, res)
        same(content.cpu().numpy(), damaged, "the content after verify")
    content.copy_(torch.from_numpy(host))
    # one flipped bit in one table entry fails that block alone; the computed CRCs still combine to content_crc
    for b in range(4):
        bad = bytearray(want)
        bad[32 + 4 * b + (b % 4)] ^= 0x10
        st, res = verify_guarded(torch, info, dev_u8(torch, np.frombuffer(bytes(bad), dtype=np.uint8)), content, n)
        assert st == [CHECKSUM if i == b else 0 for i in range(4)] and res == [0, 1], (b, st, res)
    # a flipped content_crc under a header_crc that matches it: every block OK, the content as a whole not
    bad = bytearray(want)
    bad[21] ^= 0x40
    bad = K.refresh_header_crc(bytes(bad))
    st, res = verify_guarded(torch, info_of(bad), dev_u8(torch, np.frombuffer(bad, dtype=np.uint8)), content, n)
    assert st == [0, 0, 0, 0] and res == [CHECKSUM, 0], (st, res)
    # a header on the device that differs from `info`: BAD_FRAME everywhere
    for at in (0, 6, 9, 20, 31):
        bad = bytearray(want)
        bad[at] ^= 1
        st, res = verify_guarded(torch, info, dev_u8(torch, np.frombuffer(bytes(bad), dtype=np.uint8)), content, n)
        assert st == [BAD_FRAME] * 4 and res == [BAD_FRAME, 4], (at, st, res)
    st, res = verify_guarded(torch, info, rec, content, n)
    assert st == [0, 0, 0, 0] and res == [0, 0]


@gpu
def test_python_check_build_and_verify(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    x = torch.from_numpy(np.random.default_rng(5).integers(-1000, 1000, 30011).astype(np.int32)).cuda()
    raw = PR.raw_bytes(x.cpu().numpy()).tobytes()
    for cb in (256, 65536):
        rec = codec.check_build(x, check_block=cb)
        assert rec.cpu().numpy().tobytes() == K.record(raw, cb.bit_length() - 1)
        st, res = codec.check_verify(rec, x)
        assert res.tolist() == [0, 0] and not bool(st.any())
    assert codec.check_build(x[:0]).cpu().numpy().tobytes() == K.record(b"", 16)
    with pytest.raises(ValueError):
        codec.check_build(x, check_block=1000)


# ---------------------------------------------------------------- sealed buffers
def sealed_elems(torch, kind, w):
    """Three blocks of the container and a ragged tail."""
    from test_gpu_delta import walk
    from test_gpu_planes import randn_ints

    if kind == "frame":
        return content_of("c2", 3 * BLOCK + 333, 3)
    n = 3 * BLOCK // w + 333 // w + 1
    if kind == "planes":
        return randn_ints(torch, n, {2: torch.bfloat16, 4: torch.float32}[w], 3)
    return walk(n, w, 3)


SEALED = [("frame", 1, CKPT), ("planes", 2, 0), ("planes", 4, 0), ("delta", 4, 0), ("delta", 8, 0)]


@gpu
@pytest.mark.parametrize("kind,w,ckpt", SEALED)
@pytest.mark.parametrize("check_block", [256, 65536])
def test_sealed_buffer_equals_the_reference_and_round_trips(torch_cuda, kind, w, ckpt, check_block):
    torch = torch_cuda
    codec = codec_for(ckpt=ckpt)
    a = sealed_elems(torch, kind, w)
    assert a.dtype.itemsize == w
    check_log = check_block.bit_length() - 1
    want = K.seal(a, kind, BLOCK, ckpt, 2, check_log)
    x = torch.from_numpy(a).cuda()
    # the _into call between guard bands
    scratch = None
    if kind != "frame":
        need = (codec.planes_scratch_bytes if kind == "planes" else codec.delta_scratch_bytes)(x.numel(), w)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    w_buf, buf = g8(torch, codec.sealed_bound(x, kind, check_block))
    w_len, out_len = g64(torch, 1)
    w_res, res = g32(torch, 2)
    buf.zero_()
    rec = codec.compress_sealed_into(x, kind, buf, out_len, res, scratch, check_block)
    torch.cuda.synchronize()
    for wh, v, f, name in ((w_buf, buf, A5, "buf"), (w_len, out_len, F64, "out_len"), (w_res, res, F32, "result")):
        assert_guards(wh, v, f, name)
    assert rec == K.record_bytes(a.nbytes, check_log) and rec + int(out_len.item()) == len(want)
    same(buf[: len(want)].cpu().numpy(), np.frombuffer(want, dtype=np.uint8), f"sealed {kind} w {w}")
    assert bool((buf[len(want):] == 0).all()), "a store past the buffer's end"
    sealed = codec.compress_sealed(x, kind, check_block)
    assert sealed.cpu().numpy().tobytes() == want
    # round trip, at the buffer's own address and at an odd one
    odd = torch.empty(len(want) + 1, dtype=torch.uint8, device="cuda")[1:]
    odd.copy_(sealed)
    assert odd.data_ptr() % 2 == 1
    for b in (sealed, odd):
        out, bst, cst, cres = codec.decompress_sealed(b, x.dtype, with_result=True)
        assert torch.equal(out, x) and not bool(bst.any()) and not bool(cst.any()) and cres.tolist() == [0, 0]
        assert cst.numel() == K.n_cb_of(a.nbytes, check_log)
    from entropy_coders_amd import sealed_compress, sealed_decompress

    if check_block == 256:
        blob = sealed_compress(a, kind, check_block, block_size=BLOCK, ckpt_interval=ckpt)
        assert blob == want
        back = sealed_decompress(blob, None if kind == "frame" else a.dtype)
        assert (back == a.tobytes()) if kind == "frame" else np.array_equal(back, a)


@gpu
def test_empty_sealed_buffer(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    x = torch.empty(0, dtype=torch.uint8, device="cuda")
    sealed = codec.compress_sealed(x)
    assert sealed.cpu().numpy().tobytes() == K.seal(np.zeros(0, np.uint8), "frame", BLOCK, CKPT, 2)
    out, bst, cst = codec.decompress_sealed(sealed)
    assert out.numel() == 0 and bst.numel() == 0 and cst.numel() == 0


@gpu
def test_a_flipped_raw_byte_is_caught_by_the_check_alone(torch_cuda):
    """The case the containers cannot see: uniform random content (every
    block RAW), one byte of a RAW record flipped.  The frame decodes with
    every block status OK and a wrong byte; the check names the block."""
    from entropy_coders_amd import FseError, sealed_decompress

    torch = torch_cuda
    codec = codec_for()
    host = content_of("random", 3 * BLOCK + 333, 11)
    x = torch.from_numpy(host).cuda()
    want = K.seal(host, "frame", BLOCK, CKPT, 2, 8)
    sealed = codec.compress_sealed(x, "frame", 256)
    assert sealed.cpu().numpy().tobytes() == want
    off = K.record_bytes(len(host), 8)
    assert set(R.types_of(want[off:])) == {R.RAW}
    records = off + 32 + 4 * 4  # RAW records back to back: content byte i lies at records + i
    for at in (0, 255, 256, 5000, len(host) - 1):
        bad = sealed.clone()
        bad[records + at] ^= 0x20
        out, bst, cst, cres = codec.decompress_sealed(bad, with_result=True)
        assert not bool(bst.any()), "the frame itself sees nothing"
        got = out.cpu().numpy()
        assert got[at] == host[at] ^ 0x20 and np.array_equal(np.delete(got, at), np.delete(host, at))
        want_st = [CHECKSUM if b == at // 256 else 0 for b in range(K.n_cb_of(len(host), 8))]
        assert cst.tolist() == want_st and cres.tolist() == [CHECKSUM, 1], (at, cres.tolist())
        with pytest.raises(FseError) as e:
            sealed_decompress(bad.cpu().numpy().tobytes())
        assert e.value.code == "CHECKSUM"
    assert sealed_decompress(want) == host.tobytes()


@gpu
def test_flips_inside_fse_payloads(torch_cuda):
    """A flipped bit inside an FSE record's payload, 64 seeded positions:
    whatever the decoder makes of it, a check block whose status is OK holds
    the input's bytes."""
    torch = torch_cuda
    codec = codec_for()
    host = content_of("c2", 3 * BLOCK + 333, 12)
    x = torch.from_numpy(host).cuda()
    sealed = codec.compress_sealed(x, "frame", 256)
    want = K.seal(host, "frame", BLOCK, CKPT, 2, 8)
    assert sealed.cpu().numpy().tobytes() == want
    off = K.record_bytes(len(host), 8)
    types = R.types_of(want[off:])
    assert set(types) == {R.FSE}
    frame = want[off:]
    n_blocks = len(types)
    directory = np.frombuffer(frame[32: 32 + 4 * n_blocks], dtype="<u4")
    spb = [R.spb_of(R.raw_len(len(host), BLOCK, b), CKPT, 2) for b in range(n_blocks)]
    starts, at = [], 32 + 4 * n_blocks
    for b in range(n_blocks):
        stored = int(directory[b] & 0x3FFFFFFF)
        starts.append((at + 8 * spb[b], stored))  # the header || payload behind the checkpoints
        at += 8 * spb[b] + stored
    assert at == len(frame)
    rng = np.random.default_rng(0xF11B)
    n_cb = K.n_cb_of(len(host), 8)
    seen_damage = 0
    for _ in range(64):
        b = int(rng.integers(0, n_blocks))
        s, stored = starts[b]
        pos = off + s + int(rng.integers(stored // 4, stored))  # inside the payload, behind the table header
        bad = sealed.clone()
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        out, bst, cst, cres = codec.decompress_sealed(bad, with_result=True)
        got, st = out.cpu().numpy(), cst.tolist()
        for cb in range(n_cb):
            if st[cb] == 0:
                assert np.array_equal(got[cb * 256: (cb + 1) * 256], host[cb * 256: (cb + 1) * 256]), (pos, cb)
            else:
                assert st[cb] == CHECKSUM
        wrong = not np.array_equal(got, host)
        assert wrong == any(st) and (cres.tolist()[0] == CHECKSUM) == wrong and cres.tolist()[1] == sum(map(bool, st))
        seen_damage += wrong
    assert seen_damage > 0


# ---------------------------------------------------------------- ranges
def place(host, triples, size):
    dst = np.full(size, A5, dtype=np.uint8)
    for s, ln, d in triples:
        dst[d: d + ln] = host[s: s + ln]
    return dst


def verify_ranges_guarded(torch, info, rec, triples, dst_dev):
    L = lib()
    from entropy_coders_amd import BlockCodec

    arr = BlockCodec.frame_ranges(triples)
    w_st, st = g32(torch, len(triples))
    w_res, res = g32(torch, 2)
    before = dst_dev.clone()
    rc = L.fsehip_check_verify_ranges(C.byref(info), ptr(rec), arr, len(triples), ptr(dst_dev), dst_dev.numel(),
                                      ptr(st), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(w_st, st, F32, "d_range_status")
    assert_guards(w_res, res, F32, "d_result")
    assert torch.equal(before, dst_dev), "verify stored into the ranges"
    return st.cpu().numpy().tolist(), res.cpu().numpy().tolist()


@gpu
@pytest.mark.parametrize("check_log", [8, 10, 12])
def test_verify_ranges_against_the_model(torch_cuda, check_log):
    torch = torch_cuda
    B = 1 << check_log
    n = 5 * B + 77
    host = content_of("random", n, 21 + check_log)
    want = K.record(host.tobytes(), check_log)
    info = info_of(want)
    rec = dev_u8(torch, np.frombuffer(want, dtype=np.uint8))
    edges = sorted({0, n, *(k * B + d for k in range(1, 6) for d in (-1, 0, 1))})
    pairs = [(s, e) for s in edges for e in edges if e >= s]
    assert (n, n) in pairs and (0, n) in pairs and any(s == e for s, e in pairs)
    rng = np.random.default_rng(check_log)
    codec = codec_for()
    # 33 ranges in a call (two launches), every pair once (every destination shift: test_every_destination_shift)
    for i0 in range(0, len(pairs), 33):
        chunk = pairs[i0: i0 + 33]
        shift = (i0 // 33) % 16
        triples, at = [], shift
        for s, e in chunk:
            triples.append((s, e - s, at))
            at += e - s + int(rng.integers(0, 3))
        base = torch.zeros(at + 16, dtype=torch.uint8, device="cuda")
        assert base.data_ptr() % 16 == 0
        dst_host = place(host, triples, at)
        dst = base[:at]
        dst.copy_(torch.from_numpy(dst_host))
        st, res = verify_ranges_guarded(torch, info, rec, triples, dst)
        assert st == [0] * len(triples) and res == [0, 0], (check_log, i0, st, res)
        assert codec.check_ranges_verified_bytes(info, triples) == K.verified_bytes(n, check_log, triples)
        # one flipped byte in one range: it fails iff the byte lies in a block the range wholly covers
        for pick in rng.integers(0, len(triples), 6):
            s, ln, d = triples[int(pick)]
            if not ln:
                continue
            x = int(rng.integers(0, ln))
            dst[d + x] ^= 0x04
            st, res = verify_ranges_guarded(torch, info, rec, triples, dst)
            hit = (s + x) // B in K.covered(n, check_log, s, ln)
            assert st == [CHECKSUM if (j == int(pick) and hit) else 0 for j in range(len(triples))], (s, ln, x, st)
            assert res == [0, 1 if hit else 0]
            dst[d + x] ^= 0x04
    # a header on the device that differs from `info`
    bad = bytearray(want)
    bad[17] ^= 1
    triples = [(0, B, 0), (5, 0, 0)]
    dst = dev_u8(torch, host[:B])
    st, res = verify_ranges_guarded(torch, info, dev_u8(torch, np.frombuffer(bytes(bad), dtype=np.uint8)), triples, dst)
    assert st == [BAD_FRAME, BAD_FRAME] and res == [BAD_FRAME, 2]
    assert verify_ranges_guarded(torch, info, rec, [], dst) == ([], [0, 0])


@gpu
def test_every_destination_shift(torch_cuda):
    torch = torch_cuda
    n = 4 * 256 + 9
    host = content_of("c2", n, 31)
    want = K.record(host.tobytes(), 8)
    info, rec = info_of(want), dev_u8(torch, np.frombuffer(want, dtype=np.uint8))
    for shift in range(16):
        triples = [(255, 600, shift), (512, n - 512, shift + 700)]
        base = torch.zeros(shift + 700 + n + 16, dtype=torch.uint8, device="cuda")
        dst = base[: shift + 700 + n - 512]
        dst.copy_(torch.from_numpy(place(host, triples, dst.numel())))
        st, res = verify_ranges_guarded(torch, info, rec, triples, dst)
        assert st == [0, 0] and res == [0, 0], shift
        dst[shift + 1] ^= 1    # content byte 256: the first range covers blocks 1 and 2 wholly
        dst[shift + 700 + n - 513] ^= 1  # the content's last byte: the ragged last block counts
        st, res = verify_ranges_guarded(torch, info, rec, triples, dst)
        assert st == [CHECKSUM, CHECKSUM] and res == [0, 2], (shift, st, res)


@gpu
@pytest.mark.parametrize("kind,w", [("frame", 1), ("planes", 2), ("delta", 4)])
def test_sealed_ranges_end_to_end(torch_cuda, kind, w):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    codec = codec_for(ckpt=CKPT if kind == "frame" else 0)
    a = sealed_elems(torch, kind, w) if kind != "frame" else content_of("random", 3 * BLOCK + 333, 41)
    x = torch.from_numpy(a).cuda()
    sealed = codec.compress_sealed(x, kind, 256)
    n = len(a)
    per = 256 // w  # elements per check block
    ranges = [(0, n), (per - 1, 3 * per + 2), (per, per), (5, 0), (n - per - 3, per + 3)]
    views, st, cst = codec.decompress_sealed_ranges(sealed, x.dtype, ranges)
    assert not bool(st.any()) and not bool(cst.any())
    for (s, c), v in zip(ranges, views):
        assert np.array_equal(v.cpu().numpy(), a[s: s + c])
    assert torch.equal(codec.decompress_sealed_range(sealed, x.dtype, per, 2 * per), x[per: 3 * per])
    if kind == "frame":  # RAW records: a flipped byte reaches the output unseen by the frame
        off = K.record_bytes(n, 8)
        bad = sealed.clone()
        bad[off + 32 + 16 + 300] ^= 2  # content byte 300, check block 1
        views, st, cst = codec.decompress_sealed_ranges(bad, None, [(0, 256), (256, 256), (257, 400), (200, 400)])
        assert not bool(st.any()) and cst.tolist() == [0, CHECKSUM, 0, CHECKSUM]
        with pytest.raises(FseError) as e:
            codec.decompress_sealed_range(bad, None, 256, 512)
        assert e.value.code == "CHECKSUM"


# ---------------------------------------------------------------- stream order
class CheckChain(Chain):
    """check_build -> compress_sealed -> decompress_sealed -> verify_ranges on
    one stream with no host synchronisation, inputs poison until the gate
    opens."""

    N = 40 * BLOCK + 333

    def __init__(self):
        self.host = np.asarray(O.generate(0, 0.155, 0x5EED0C99, 0, self.N), dtype=np.uint8)
        self.want = K.seal(self.host, "frame", BLOCK, CKPT, 2, 12)
        self.want_rec = K.record(self.host.tobytes(), 8)
        self.triples = [(0, 4096, 3), (4095, 8194, 5000), (self.N - 5000, 5000, 14000), (77, 0, 1)]
        self.dst_size = 19000

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        n = self.N
        self.sealed = BlockCodec.sealed_info(self.want)
        self.inner = c.sealed_inner_info("frame", self.want[self.sealed[2]:])
        self.rec_info = info_of(self.want_rec)
        self.src = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.host))]
        self.w_rec, self.rec = g8(torch, len(self.want_rec))
        self.w_buf, self.buf = g8(torch, c.sealed_bound(self.src, "frame", 4096))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.w_out, self.out = g8(torch, n)
        self.w_bst, self.bst = g32(torch, self.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.w_cst, self.cst = g32(torch, self.sealed[0].n_cb)
        self.w_vres, self.vres = g32(torch, 2)
        self.w_rst, self.rst = g32(torch, len(self.triples))
        self.w_rres, self.rres = g32(torch, 2)
        self.arr = c.frame_ranges(self.triples)
        self.dst = torch.empty(self.dst_size, dtype=torch.uint8, device="cuda")
        self.dst_upload = pinned(torch, place(self.host, self.triples, self.dst_size))
        self.uploads.append((self.dst, self.dst_upload))

    def poison(self):
        self.src.fill_(7)
        self.dst.fill_(7)
        self.buf.zero_()  # what the decoder reads: all zeros is BAD_FRAME
        self.rec.fill_(A5)
        self.len.fill_(F64)
        self.out.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.cst, self.vres, self.rst, self.rres):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        c.check_build_into(self.src, self.rec, 256)
        c.compress_sealed_into(self.src, "frame", self.buf, self.len, self.cres, None, 4096)
        c.decompress_sealed_into(buf, self.sealed, self.inner, self.out, self.bst, self.dres, self.cst, self.vres)
        c.check_verify_ranges_into(self.rec, self.rec_info, self.arr, self.dst, self.rst, self.rres)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_rec, self.rec, A5, "d_record"), (self.w_buf, self.buf, A5, "sealed buffer"),
                              (self.w_len, self.len, F64, "d_out_len"), (self.w_cres, self.cres, F32, "compress result"),
                              (self.w_out, self.out, A5, "content"), (self.w_bst, self.bst, F32, "d_block_status"),
                              (self.w_dres, self.dres, F32, "d_result"), (self.w_cst, self.cst, F32, "d_check_status"),
                              (self.w_vres, self.vres, F32, "verify d_result"),
                              (self.w_rst, self.rst, F32, "d_range_status"), (self.w_rres, self.rres, F32, "ranges d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        same(self.rec.cpu().numpy(), np.frombuffer(self.want_rec, dtype=np.uint8), "the record")
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "the sealed buffer")
        assert self.len.tolist() == [n - self.sealed[2]]
        assert self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        same(self.out.cpu().numpy(), self.host, "the decoded content")
        assert self.vres.tolist() == [0, 0] and not bool(self.cst.any()), (self.vres.tolist(), self.cst.tolist())
        assert self.rres.tolist() == [0, 0] and not bool(self.rst.any()), (self.rres.tolist(), self.rst.tolist())


def test_host_side_of_the_check_chain():
    chain = CheckChain()
    assert len(chain.want) < chain.N and zlib.crc32(chain.host.tobytes()) == K.parse(chain.want)["content_crc"]
    assert K.verified_bytes(chain.N, 8, chain.triples) > 0


@gpu
def test_check_chain_behind_the_gate(torch_cuda, warm):
    """check_build, compress_sealed, decompress_sealed and the ranges call
    behind the gate of tests/test_gpu_stream_order.py: every call returns
    while its inputs are still poison, so none of them waits for the stream
    or reads device data on the host."""
    chain = CheckChain()
    chain.alloc(torch_cuda)
    warm.chains["check"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["check"] = warm.run(chain, gated=False)
    behind_gate(warm, "check")
