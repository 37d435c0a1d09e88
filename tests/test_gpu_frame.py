"""The frame on the GPU (fsehip_frame_compress / fsehip_frame_decompress,
BlockCodec.compress_frame / decompress_frame, frame_compress /
frame_decompress) against tests/frame_ref.py, the format restated over the
CPU oracle: exact bytes, round trips, chunk invariance, the empty input, odd
frame addresses, guard bands round every output, and damaged frames."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as R
from oracle import oracle as O

gpu = pytest.mark.gpu

BLOCK, CKPT = R.BLOCK, R.CKPT
GUARD_BYTES = 256
FILL = {"uint8": 0xA5, "int32": -99, "int64": -99}  # values no tested output can hold
BAD_FRAME = R.BAD_FRAME


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def corpora():
    """tail length -> the shared corpus (host array); computed once, never changed."""
    out = {t: R.corpus(t) for t in (1000, 1)}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the guard-band helper (tests/test_gpu_guard_bands.py)
def guarded(torch, n_elems, dtype, fill):
    """(whole, view): `view` is n_elems elements of `whole`, starts at a
    multiple of 256 bytes and has at least 256 bytes of `fill` on both sides
    (the view itself is filled too)."""
    item = torch.empty(0, dtype=dtype).element_size()
    pad = GUARD_BYTES // item
    body = (n_elems + pad - 1) // pad * pad
    whole = torch.full((pad + body + pad,), fill, dtype=dtype, device="cuda")
    assert whole.data_ptr() % GUARD_BYTES == 0
    view = whole[pad: pad + n_elems]
    assert view.numel() == n_elems and view.storage_offset() * item % GUARD_BYTES == 0
    return whole, view


def assert_guards(whole, view, fill, what=""):
    """Both bands of `whole` around `view` still hold `fill`."""
    lo, n = view.storage_offset(), view.numel()
    below, above = whole[:lo], whole[lo + n:]
    assert below.numel() * whole.element_size() >= GUARD_BYTES and above.numel() * whole.element_size() >= GUARD_BYTES
    assert bool((below == fill).all()), f"{what}: a store below the array"
    assert bool((above == fill).all()), f"{what}: a store past the array's last element"


def g8(torch, n):
    return guarded(torch, n, torch.uint8, FILL["uint8"])


def g32(torch, n):
    return guarded(torch, n, torch.int32, FILL["int32"])


def g64(torch, n):
    return guarded(torch, n, torch.int64, FILL["int64"])


def codec_for(nstates=2, ckpt=CKPT, table_log=0, block=BLOCK):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=block, table_log=table_log, ckpt_interval=ckpt, nstates=nstates)


def dev(torch, host):
    return torch.from_numpy(np.array(host, dtype=np.uint8)).cuda()


def host_bytes(t):
    return t.cpu().numpy().tobytes()


def device_sidecars(codec, src):
    """The zero-filled sidecar array fsehip_compress_blocks fills (host uint64), and the compressed batch."""
    cb = codec.compress(src)  # alloc() zero-fills the sidecar
    return cb["sidecar"].cpu().numpy().view(np.uint64), cb


def decode_guarded(torch, codec, frame, chunk_blocks=0):
    """decompress_frame_into with guard bands round the output and the
    statuses.  Returns (info, out bytes, statuses, result); the guards are
    asserted."""
    info = codec.frame_info(frame)
    ow, out = g8(torch, info.n_total)
    sw, st = g32(torch, info.n_blocks)
    rw, res = g32(torch, 2)
    codec.decompress_frame_into(frame, info, out, st, res, chunk_blocks)
    torch.cuda.synchronize()
    assert_guards(ow, out, FILL["uint8"], "d_out")
    assert_guards(sw, st, FILL["int32"], "d_block_status")
    assert_guards(rw, res, FILL["int32"], "d_result")
    return info, out, st.cpu().numpy(), res.cpu().numpy()


# ---------------------------------------------------------------- exact bytes, round trip
def test_corpus_has_all_three_types(corpora):
    """On the oracle alone: the corpus exercises RAW, RLE and FSE (a changed
    generator cannot quietly turn the tests below into FSE-only)."""
    for tail, raw in corpora.items():
        for nstates in (2, 1):
            types = R.types_of(R.build_frame(raw, BLOCK, CKPT, nstates))
            assert {R.RAW, R.RLE, R.FSE} <= set(types), (tail, nstates, types)
    assert R.types_of(R.build_frame(corpora[1], BLOCK, CKPT, 2))[-1] == R.RAW  # the 1-byte tail: TOO_SHORT


# (1-state at table logs 12 and 13: tests/test_gpu_onestate_logs.py)
FORMATS = [(2, CKPT, 0), (2, 0, 0), (2, CKPT, 13), (2, 0, 13), (1, CKPT, 0), (1, 0, 0)]


@gpu
@pytest.mark.parametrize("nstates,ckpt,table_log", FORMATS)
@pytest.mark.parametrize("tail", [1000, 1])
def test_frame_exact_bytes_and_round_trip(torch_cuda, corpora, nstates, ckpt, table_log, tail):
    torch = torch_cuda
    raw = corpora[tail]
    codec = codec_for(nstates, ckpt, table_log)
    src = dev(torch, raw)
    side, cb = device_sidecars(codec, src)
    frame = codec.compress_frame(src)
    want = R.build_frame(raw, BLOCK, ckpt, nstates, table_log, sidecars=side if ckpt else None)
    got = host_bytes(frame)
    assert len(got) == len(want) and got == want
    assert len(got) <= codec.frame_bound(len(raw))
    # the sidecars' defined prefix is the oracle's decode checkpoints (tests/test_gpu_parity.py)
    if ckpt:
        status = cb["status"].cpu().numpy()
        for b in np.flatnonzero(status == 0):
            comp = codec.block_bytes(cb, int(b))
            ref = R.oracle_checkpoints(comp, ckpt, nstates, codec.side_per_block)
            if ref is None:  # single-symbol block: no oracle walk
                continue
            k = len(O.checkpoints1(comp, ckpt)[0] if nstates == 1 else O.checkpoints2(comp, ckpt)[0])
            mine = side[b * codec.side_per_block: b * codec.side_per_block + k]
            assert np.array_equal(mine, ref[:k]), f"checkpoints of block {b}"
    # round trip on the device, with guards, and on the oracle
    info, out, st, res = decode_guarded(torch, codec_for(), frame)  # a codec with other parameters: the frame alone decides
    assert (info.n_total, info.n_blocks, info.nstates) == (len(raw), R.n_blocks_of(len(raw), BLOCK), nstates)
    assert list(res) == [0, 0] and not st.any(), (res, st)
    assert host_bytes(out) == raw.tobytes()
    assert R.decode_frame(got) == raw.tobytes()
    out2, st2 = codec.decompress_frame(frame)
    assert torch.equal(out2, out) and not bool(st2.any())


@gpu
def test_frame_result_counts_non_fse_blocks(torch_cuda, corpora):
    torch = torch_cuda
    raw = corpora[1000]
    codec = codec_for()
    src = dev(torch, raw)
    fw, frame = g8(torch, codec.frame_bound(len(raw)))
    lw, flen = g64(torch, 1)
    rw, res = g32(torch, 2)
    codec.compress_frame_into(src, frame, flen, res)
    torch.cuda.synchronize()
    want = R.build_frame(raw, BLOCK, CKPT, 2, sidecars=device_sidecars(codec, src)[0])
    n = int(flen.item())
    assert n == len(want) and host_bytes(frame[:n]) == want
    assert list(res.cpu().numpy()) == [0, sum(t != R.FSE for t in R.types_of(want))]
    # nothing past frame_len inside the frame_cap-sized buffer, nor outside it
    assert bool((frame[n:] == FILL["uint8"]).all()), "a store past frame_len"
    assert_guards(fw, frame, FILL["uint8"], "d_frame")
    assert_guards(lw, flen, FILL["int64"], "d_frame_len")
    assert_guards(rw, res, FILL["int32"], "d_result")


# ---------------------------------------------------------------- chunks, empty input, alignment
@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, CKPT), (2, 0), (1, CKPT)])
def test_chunk_split_does_not_show(torch_cuda, corpora, nstates, ckpt):
    torch = torch_cuda
    raw = corpora[1000]
    codec = codec_for(nstates, ckpt)
    src = dev(torch, raw)
    frames = [host_bytes(codec.compress_frame(src, chunk_blocks=c)) for c in (1, 3, 4096)]
    assert frames[0] == frames[1] == frames[2]
    frame = dev(torch, np.frombuffer(frames[0], dtype=np.uint8))
    for c in (1, 3, 4096):
        _, out, st, res = decode_guarded(torch, codec, frame, chunk_blocks=c)
        assert list(res) == [0, 0] and not st.any(), (c, res, st)
        assert host_bytes(out) == raw.tobytes(), c


@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, CKPT), (1, 0)])
def test_empty_input(torch_cuda, nstates, ckpt):
    torch = torch_cuda
    codec = codec_for(nstates, ckpt)
    frame = codec.compress_frame(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert host_bytes(frame) == R.build_frame(np.zeros(0, np.uint8), BLOCK, ckpt, nstates) and frame.numel() == 32
    info, out, st, res = decode_guarded(torch, codec, frame)
    assert info.n_total == 0 and info.n_blocks == 0 and out.numel() == 0 and list(res) == [0, 0]


@gpu
@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("tail", [1000, 1])
def test_frame_at_any_byte_address(torch_cuda, corpora, offset, tail):
    """The frame tensor at byte 0 and byte 5 of its allocation, on both sides."""
    torch = torch_cuda
    raw = corpora[tail]
    codec = codec_for()
    src = dev(torch, raw)
    cap = codec.frame_bound(len(raw))
    fw, fv = g8(torch, cap + 16)
    frame = fv[offset: offset + cap]
    assert frame.data_ptr() % 16 == offset
    flen = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = torch.full((2,), -99, dtype=torch.int32, device="cuda")
    codec.compress_frame_into(src, frame, flen, res)
    torch.cuda.synchronize()
    n = int(flen.item())
    want = R.build_frame(raw, BLOCK, CKPT, 2, sidecars=device_sidecars(codec, src)[0])
    assert host_bytes(frame[:n]) == want and int(res[0]) == 0
    assert bool((fv[:offset] == FILL["uint8"]).all()) and bool((fv[offset + n:] == FILL["uint8"]).all())
    assert_guards(fw, fv, FILL["uint8"], "d_frame")
    _, out, st, res = decode_guarded(torch, codec, frame[:n])
    assert list(res) == [0, 0] and not st.any()
    assert host_bytes(out) == raw.tobytes()


# ---------------------------------------------------------------- damaged frames
# The decoder's validation (frame_check_kernel / frame_scan_kernel in
# csrc/fse_frame.hip): nothing is copied unless the header equals the parsed
# one and the directory's record lengths end exactly at frame_len, which puts
# every record inside the frame; an FSE length is bounded by the slot; the
# block decoders bound their own reads by comp_len.  These cases check
# statuses; none is meant to reach a bad access.
def _decode_damaged(torch, frame_bytes):
    frame = dev(torch, np.frombuffer(frame_bytes, dtype=np.uint8))
    return decode_guarded(torch, codec_for(), frame)


def _entry(frame, b):
    return int.from_bytes(frame[32 + 4 * b: 36 + 4 * b], "little")


def _with_entry(frame, b, e):
    return frame[:32 + 4 * b] + int(e).to_bytes(4, "little") + frame[36 + 4 * b:]


def _record_pos(frame, b):
    """Byte offset of block b's record and its length (checkpoints included)."""
    info, directory, records = R.split_frame(frame)
    pos = info["records_off"]
    for i in range(b):
        pos += 8 * len(records[i][0]) + len(records[i][1])
    return pos, 8 * len(records[b][0]) + len(records[b][1])


@pytest.fixture(scope="module")
def good_frame(torch_cuda, corpora):
    """The corpus frame as the device writes it (test_frame_exact_bytes_and_round_trip
    holds it to the reference), as host bytes to damage."""
    return host_bytes(codec_for().compress_frame(dev(torch_cuda, corpora[1000])))


def _assert_frame_level(torch, frame_bytes, n_total):
    info, out, st, res = _decode_damaged(torch, frame_bytes)
    assert int(res[0]) == BAD_FRAME
    assert (st == BAD_FRAME).all() and int(res[1]) == info.n_blocks
    assert bool((out == FILL["uint8"]).all()), "a rejected frame must leave d_out untouched"


def _assert_one_block(torch, frame_bytes, raw, bad, status=None):
    """Only block `bad` fails (with `status`, or any failure when None); the others decode correctly."""
    info, out, st, res = _decode_damaged(torch, frame_bytes)
    assert int(res[0]) == 0 and int(res[1]) == 1, res
    assert st[bad] != 0 and (status is None or st[bad] == status), st
    assert not np.delete(st, bad).any(), st
    got, want = out.cpu().numpy(), raw
    for b in range(info.n_blocks):
        if b != bad:
            assert np.array_equal(got[b * BLOCK: (b + 1) * BLOCK], want[b * BLOCK: (b + 1) * BLOCK]), b
    return got[bad * BLOCK: (bad + 1) * BLOCK]


@gpu
def test_damaged_truncated_or_lengthened(torch_cuda, corpora, good_frame):
    _assert_frame_level(torch_cuda, good_frame[:-1], len(corpora[1000]))
    _assert_frame_level(torch_cuda, good_frame + b"\x00", len(corpora[1000]))
    _assert_frame_level(torch_cuda, good_frame[:32 + 8], len(corpora[1000]))  # ends inside the directory


@gpu
def test_damaged_header_differs_on_the_device(torch_cuda, corpora, good_frame):
    """fsehip_frame_decompress is handed an info that is not the frame's own header."""
    torch = torch_cuda
    codec = codec_for()
    frame = dev(torch, np.frombuffer(good_frame, dtype=np.uint8))
    info = codec.frame_info(good_frame)
    info.nstates = 1
    info.ckpt_interval = 256
    ow, out = g8(torch, info.n_total)
    st = torch.zeros(info.n_blocks, dtype=torch.int32, device="cuda")
    res = torch.zeros(2, dtype=torch.int32, device="cuda")
    codec.decompress_frame_into(frame, info, out, st, res)
    torch.cuda.synchronize()
    assert int(res[0]) == BAD_FRAME and bool((out == FILL["uint8"]).all())
    assert_guards(ow, out, FILL["uint8"], "d_out")


@gpu
def test_damaged_type_3_entry(torch_cuda, corpora, good_frame):
    raw = corpora[1000]
    types = R.types_of(good_frame)
    b = types.index(R.RAW)  # a type-3 entry's record is stored_len bytes: the frame stays consistent
    bad = _with_entry(good_frame, b, 3 << 30 | _entry(good_frame, b) & 0x3FFFFFFF)
    block = _assert_one_block(torch_cuda, bad, raw, b, BAD_FRAME)
    assert (block == FILL["uint8"]).all(), "a skipped block's output stays untouched"
    # on an FSE entry the checkpoints no longer count: the directory does not end at frame_len
    f = types.index(R.FSE)
    _assert_frame_level(torch_cuda, _with_entry(good_frame, f, 3 << 30 | _entry(good_frame, f) & 0x3FFFFFFF), len(raw))


@gpu
def test_damaged_raw_length(torch_cuda, corpora, good_frame):
    raw = corpora[1000]
    b = R.types_of(good_frame).index(R.RAW)
    short = _with_entry(good_frame, b, R.RAW << 30 | (BLOCK - 1))
    _assert_frame_level(torch_cuda, short, len(raw))  # the frame is now one byte longer than its directory says
    pos, ln = _record_pos(good_frame, b)
    consistent = short[:pos + ln - 1] + short[pos + ln:]  # drop the record's last byte: lengths agree again
    block = _assert_one_block(torch_cuda, consistent, raw, b, BAD_FRAME)
    assert (block == FILL["uint8"]).all()


@gpu
def test_damaged_fse_length_above_the_slot(torch_cuda, corpora, good_frame):
    raw = corpora[1000]
    b = R.types_of(good_frame).index(R.FSE)
    slot = R.slot_bytes(BLOCK, 11)
    big = _with_entry(good_frame, b, R.FSE << 30 | (slot + 1))
    _assert_frame_level(torch_cuda, big, len(raw))
    pos, ln = _record_pos(good_frame, b)
    pad = slot + 1 - (_entry(good_frame, b) & 0x3FFFFFFF)
    consistent = big[:pos + ln] + bytes(pad) + big[pos + ln:]  # the record really is slot + 1 bytes long
    block = _assert_one_block(torch_cuda, consistent, raw, b, BAD_FRAME)
    assert (block == FILL["uint8"]).all()
    # rle length 2, consistent as well
    r = R.types_of(good_frame).index(R.RLE)
    pos, ln = _record_pos(good_frame, r)
    two = _with_entry(good_frame, r, R.RLE << 30 | 2)
    _assert_one_block(torch_cuda, two[:pos] + b"\x00" + two[pos:], raw, r, BAD_FRAME)


@gpu
def test_damaged_fse_payload_byte(torch_cuda, corpora, good_frame):
    """A flipped byte inside one FSE payload: that block fails in its decoder
    (a checkpoint no longer matches) or decodes to other bytes; the frame and
    the other blocks are unaffected."""
    raw = corpora[1000]
    b = 0  # the LUT block: 2,069 bytes after 144 bytes of checkpoints
    pos, ln = _record_pos(good_frame, b)
    at = pos + ln - 700
    bad = good_frame[:at] + bytes([good_frame[at] ^ 0xFF]) + good_frame[at + 1:]
    info, out, st, res = _decode_damaged(torch_cuda, bad)
    assert int(res[0]) == 0 and not st[1:].any()
    got = out.cpu().numpy()
    assert np.array_equal(got[BLOCK:], raw[BLOCK:])
    assert st[0] != 0 and int(res[1]) == 1, (st, res)


@gpu
def test_rle_of_any_byte_decodes(torch_cuda, corpora, good_frame):
    """The encoder stores only zero runs; a decoder accepts any byte."""
    raw = np.array(corpora[1000])
    r = R.types_of(good_frame).index(R.RLE)
    pos, _ = _record_pos(good_frame, r)
    frame = good_frame[:pos] + b"\x5C" + good_frame[pos + 1:]
    raw[r * BLOCK: (r + 1) * BLOCK] = 0x5C
    info, out, st, res = _decode_damaged(torch_cuda, frame)
    assert list(res) == [0, 0] and host_bytes(out) == raw.tobytes()


# ---------------------------------------------------------------- host API
@gpu
def test_host_api(torch_cuda, corpora):
    from entropy_coders_amd import FseError, frame_compress, frame_decompress

    for data in (corpora[1000].tobytes(), corpora[1].tobytes(), b"", b"\x07"):
        frame = frame_compress(data, block_size=BLOCK)
        assert len(frame) <= 32 + 4 * R.n_blocks_of(len(data), BLOCK) + len(data)
        assert frame_decompress(frame) == data
    assert frame_decompress(frame_compress(b"\x07")) == b"\x07"  # the default 64 KiB block
    for garbage in (b"", b"FSEF", bytes(range(64)), b"FSEF" + bytes(60)):
        with pytest.raises(FseError) as e:
            frame_decompress(garbage)
        assert e.value.code == "BAD_FRAME"
