"""Byte ranges of a frame on the GPU (fsehip_frame_decompress_ranges /
_range, BlockCodec.decompress_frame_ranges_into / _ranges / _range,
frame_decompress_range).  The expected bytes are raw[src_off: src_off + len]
of the input itself, never the library's.  Every destination sits between
256-byte guard bands and is compared whole, gaps between ranges included."""
import numpy as np
import pytest

import frame_ref as R

gpu = pytest.mark.gpu

BLOCK, CKPT = R.BLOCK, R.CKPT
GUARD_BYTES = 256
FILL8, FILL32 = 0xA5, -99
BAD_FRAME = R.BAD_FRAME
# as tests/test_gpu_frame.py: both formats, with and without checkpoints, table log 13
FORMATS = [(2, CKPT, 0), (2, 0, 0), (2, CKPT, 13), (2, 0, 13), (1, CKPT, 0), (1, 0, 0)]
# the corpus' blocks: FSE, FSE, RAW, RAW, RLE, FSE (single symbol), FSE, RAW, then the tail
FSE_B, RAW_B, RLE_B = 1, 2, 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def corpora():
    out = {t: R.corpus(t) for t in (1000, 1)}
    for a in out.values():
        a.setflags(write=False)
    return out


def codec_for(nstates=2, ckpt=CKPT, table_log=0, block=BLOCK):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=block, table_log=table_log, ckpt_interval=ckpt, nstates=nstates)


def dev(torch, host):
    return torch.from_numpy(np.array(host, dtype=np.uint8)).cuda()


@pytest.fixture(scope="module")
def frames(torch_cuda, corpora):
    """(nstates, ckpt, table_log, tail) -> the frame on the device, built once each."""
    cache = {}

    def get(nstates=2, ckpt=CKPT, table_log=0, tail=1000):
        key = (nstates, ckpt, table_log, tail)
        if key not in cache:
            cache[key] = codec_for(nstates, ckpt, table_log).compress_frame(dev(torch_cuda, corpora[tail]))
        return cache[key]

    return get


def guarded(torch, n_elems, dtype, fill):
    """(whole, view): `view` starts at a multiple of 256 bytes with at least 256 bytes of `fill` on both sides."""
    item = torch.empty(0, dtype=dtype).element_size()
    pad = GUARD_BYTES // item
    body = (n_elems + pad - 1) // pad * pad
    whole = torch.full((pad + body + pad,), fill, dtype=dtype, device="cuda")
    assert whole.data_ptr() % GUARD_BYTES == 0
    return whole, whole[pad: pad + n_elems]


def assert_guards(whole, view, fill, what):
    lo, n = view.storage_offset(), view.numel()
    assert bool((whole[:lo] == fill).all()), f"{what}: a store below the array"
    assert bool((whole[lo + n:] == fill).all()), f"{what}: a store past the array's last element"


def run(torch, frame, ranges, chunk_blocks=0, size=None, shift=0, codec=None, triples=None):
    """One call on guarded buffers.  ranges: (src_off, len, dst_off); the
    destination is `size` bytes (default: the ranges' extent + 33) starting
    `shift` bytes after a 256-byte boundary.  Returns (destination, range
    statuses, result) as host arrays, guards asserted."""
    codec = codec or codec_for()
    info = codec.frame_info(frame)
    triples = ranges if triples is None else triples  # `ranges` may be a prebuilt fsehip_frame_range array
    if size is None:
        size = max([d + ln for _, ln, d in triples], default=0) + 33
    ow, ov = guarded(torch, size + shift, torch.uint8, FILL8)
    out = ov[shift:]
    assert out.data_ptr() % GUARD_BYTES == shift
    sw, st = guarded(torch, len(triples), torch.int32, FILL32)
    rw, res = guarded(torch, 2, torch.int32, FILL32)
    codec.decompress_frame_ranges_into(frame, info, ranges, out, st, res, chunk_blocks)
    torch.cuda.synchronize()
    assert_guards(ow, ov, FILL8, "d_out")
    assert bool((ov[:shift] == FILL8).all()), "a store below d_out"
    assert_guards(sw, st, FILL32, "d_range_status")
    assert_guards(rw, res, FILL32, "d_result")
    return out.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy()


def expected(raw, ranges, size, skip=()):
    """The whole destination: FILL8 but for the ranges' bytes; source bytes in
    the blocks `skip` (failed blocks) stay at the fill value."""
    want = np.full(size, FILL8, dtype=np.uint8)
    for s, ln, d in ranges:
        want[d: d + ln] = raw[s: s + ln]
        for b in skip:
            lo, hi = max(s, b * BLOCK), min(s + ln, (b + 1) * BLOCK)
            if lo < hi:
                want[d + lo - s: d + hi - s] = FILL8
    return want


def check_ok(torch, frame, raw, ranges, **kw):
    out, st, res = run(torch, frame, ranges, **kw)
    ranges = kw.get("triples") or ranges
    assert list(res) == [0, 0], res
    assert not st.any(), st
    want = expected(raw, ranges, len(out))
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"first wrong byte at destination {bad[0]} of {len(out)}, ranges {ranges[:4]}"
    return out


def single_ranges(n):
    """(name, src_off, len, destination shift): the single-range cases."""
    B = BLOCK
    return [
        ("first byte", 0, 1, 0),
        ("a block's last byte", 2 * B - 1, 1, 0),
        ("a block's first byte", 2 * B, 1, 0),
        ("the frame's last byte", n - 1, 1, 0),
        ("inside one block", B + 100, 1000, 0),
        ("across one boundary, both partial", B - 300, 700, 0),
        ("exactly one block", 6 * B, B, 0),
        ("blocks 1..7 whole, aligned: direct", B, 7 * B, 0),
        ("blocks 1..7 whole, destination off by one: bounce", B, 7 * B, 1),
        ("the whole frame", 0, n, 0),
        ("the whole frame, destination off by 3", 0, n, 3),
        ("ends in the ragged tail", 7 * B + 10, n - 1 - (7 * B + 10), 0),
        ("whole blocks up to the frame's end", 4 * B, n - 4 * B, 0),
        ("edges in RAW and RLE", RAW_B * B + 7, (RLE_B - RAW_B) * B + 90, 5),
        ("edges in RLE and FSE", RLE_B * B + 33, 2 * B, 0),
        ("edges in FSE and RAW", FSE_B * B + 4000, 200, 15),
        ("partial head, direct middle, partial tail", 5, 7 * B, 16 - 5),
    ]


# ---------------------------------------------------------------- 1. single ranges
@gpu
@pytest.mark.parametrize("nstates,ckpt,table_log", FORMATS)
@pytest.mark.parametrize("tail", [1000, 1])
def test_single_ranges(torch_cuda, corpora, frames, nstates, ckpt, table_log, tail):
    raw = corpora[tail]
    frame = frames(nstates, ckpt, table_log, tail)
    for name, s, ln, shift in single_ranges(len(raw)):
        assert ln > 0, name
        check_ok(torch_cuda, frame, raw, [(s, ln, 0)], shift=shift)


@gpu
def test_small_blocks(torch_cuda):
    """64-byte blocks, 5 of them and a 2-byte tail: the 16-byte paths degenerate."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    raw = np.concatenate([np.zeros(64, np.uint8), np.full(64, 9, np.uint8), rng.integers(0, 4, 64, dtype=np.uint8),
                          rng.integers(0, 256, 64, dtype=np.uint8), np.full(64, 1, np.uint8),
                          np.array([3, 4], np.uint8)])
    codec = codec_for(ckpt=0, block=64)
    frame = codec.compress_frame(dev(torch, raw))
    n = len(raw)
    for s, ln, shift in [(0, n, 0), (0, n, 1), (0, 1, 0), (n - 1, 1, 0), (63, 2, 0), (64, 64, 0), (64, 4 * 64 + 2, 0),
                         (0, 5 * 64, 0), (1, n - 1, 15), (130, 100, 7)]:
        check_ok(torch, frame, raw, [(s, ln, 0)], shift=shift, codec=codec)
    ranges, at = [], 0
    for s in range(0, n, 23):
        ranges.append((s, min(23, n - s), at))
        at += min(23, n - s) + 3
    check_ok(torch, frame, raw, ranges, codec=codec)


@gpu
def test_long_pieces(torch_cuda):
    """64 KiB blocks: pieces longer than one workgroup's share of the piece
    copy, at odd alignments on both sides, and a prebuilt range array."""
    torch = torch_cuda
    codec = codec_for(ckpt=64, block=65536)
    n = 6 * 65536 + 12345
    src = codec.generate(0, 0.155, 0x5EED0002, n)
    src[2 * 65536: 3 * 65536] = torch.randint(0, 256, (65536,), dtype=torch.uint8, device="cuda")  # a RAW block
    src[3 * 65536: 4 * 65536] = 0                                                                   # an RLE block
    raw = src.cpu().numpy()
    frame = codec.compress_frame(src)
    assert {R.RAW, R.RLE, R.FSE} <= set(R.types_of(frame.cpu().numpy().tobytes()))
    for s, ln, shift in [(0, n, 0), (0, n, 1), (1, n - 1, 0), (65536 + 8191, 3 * 65536 + 3, 5), (7, 65536 - 7, 9),
                         (5 * 65536 + 1, 65536 + 12344, 0), (2 * 65536 + 8193, 8192, 3)]:
        check_ok(torch, frame, raw, [(s, ln, 0)], shift=shift, codec=codec)
    ranges = [(3, 3 * 65536, 1), (4 * 65536 - 5, 2 * 65536 + 12350, 3 * 65536 + 16), (0, 6 * 65536, 6 * 65536 + 12400)]
    check_ok(torch, frame, raw, ranges, codec=codec)
    check_ok(torch, frame, raw, codec.frame_ranges(ranges), codec=codec, triples=ranges)


# ---------------------------------------------------------------- 2. alignment grid
MODS = (0, 1, 3, 4, 8, 15)
LENGTHS = tuple(range(0, 10)) + (15, 16, 17, 4095, 4096, 4097)


@gpu
@pytest.mark.parametrize("start_block", [FSE_B, RAW_B])
@pytest.mark.parametrize("src_mod", MODS)
def test_alignment_grid(torch_cuda, corpora, frames, start_block, src_mod):
    """src_off mod 16 x destination mod 16 x lengths, one call per source alignment."""
    raw = corpora[1000]
    ranges, at = [], 0
    for k, dst_mod in enumerate(MODS):
        for ln in LENGTHS:
            s = start_block * BLOCK + 16 * (k + 1) + src_mod
            at = (at + 15) // 16 * 16 + 16 + dst_mod
            ranges.append((s, ln, at))
            at += ln
    check_ok(torch_cuda, frames(), raw, ranges)
    # and alone, where a range is its own call: the short ones and one that crosses a block
    for dst_mod in (0, 3, 15):
        for ln in (0, 1, 16, 4097):
            check_ok(torch_cuda, frames(), raw, [(start_block * BLOCK + src_mod, ln, 0)], shift=dst_mod)


# ---------------------------------------------------------------- 3. many ranges in one call
@gpu
def test_many_ranges(torch_cuda, corpora, frames):
    torch = torch_cuda
    raw = corpora[1000]
    frame = frames()
    # 64 slices of one block
    check_ok(torch, frame, raw, [(BLOCK + 64 * i, 64, 70 * i) for i in range(64)])
    # the same source range to two destinations, one of them a direct run
    check_ok(torch, frame, raw, [(0, 6 * BLOCK, 0), (0, 6 * BLOCK, 6 * BLOCK + 16), (BLOCK + 5, 50, 12 * BLOCK + 40)])
    check_ok(torch, frame, raw, [(100, 300, 0), (100, 300, 301)])
    # unsorted, overlapping sources, empty ranges mixed in
    n = len(raw)
    ranges = [(7 * BLOCK + 1, n - 7 * BLOCK - 1, 20000), (0, 0, 5), (3 * BLOCK - 9, 18, 0), (n, 0, 77),
              (BLOCK, 5 * BLOCK, 4096 * 8), (2 * BLOCK + 1, 2 * BLOCK, 40), (5, 0, 41), (n - 1, 1, 18)]
    check_ok(torch, frame, raw, ranges)
    # no ranges at all
    out, st, res = run(torch, frame, [], size=64)
    assert list(res) == [0, 0] and (out == FILL8).all()


# ---------------------------------------------------------------- 4. chunk invariance
@gpu
@pytest.mark.parametrize("nstates,ckpt", [(2, CKPT), (2, 0), (1, CKPT)])
@pytest.mark.parametrize("tail", [1000, 1])
def test_chunk_invariance(torch_cuda, corpora, frames, nstates, ckpt, tail):
    raw = corpora[tail]
    n = len(raw)
    ranges = [(0, n, 0), (3, n - 3, n + 16), (BLOCK + 1, 10, 2 * n + 40), (8 * BLOCK, n - 8 * BLOCK, 2 * n + 60),
              (2 * BLOCK, 6 * BLOCK, 2 * n + 1100 + (-(2 * n + 1100)) % 16)]
    outs = [check_ok(torch_cuda, frames(nstates, ckpt, 0, tail), raw, ranges, chunk_blocks=c) for c in (1, 2, 3, 0)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


# ---------------------------------------------------------------- 5. frame placement
@gpu
def test_frame_at_an_odd_address(torch_cuda, corpora, frames):
    torch = torch_cuda
    raw = corpora[1000]
    good = frames()
    whole = torch.zeros(good.numel() + 16, dtype=torch.uint8, device="cuda")
    frame = whole[5: 5 + good.numel()]
    frame.copy_(good)
    assert frame.data_ptr() % 16 == 5
    n = len(raw)
    check_ok(torch, frame, raw, [(0, n, 0), (BLOCK - 1, 2, n + 3), (2 * BLOCK + 1, BLOCK, n + 9), (4 * BLOCK, 10, n + 5000)])


@gpu
def test_empty_frame(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    frame = codec.compress_frame(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert frame.numel() == 32
    for ranges in ([], [(0, 0, 0)], [(0, 0, 3), (0, 0, 3)]):
        out, st, res = run(torch, frame, ranges, size=16)
        assert list(res) == [0, 0] and not st.any() and (out == FILL8).all()


# ---------------------------------------------------------------- 6. uncovered blocks are not decoded
def _record_pos(frame, b):
    """Byte offset of block b's record and its length (checkpoints included)."""
    info, directory, records = R.split_frame(frame)
    pos = info["records_off"]
    for i in range(b):
        pos += 8 * len(records[i][0]) + len(records[i][1])
    return pos, 8 * len(records[b][0]) + len(records[b][1])


def _entry(frame, b):
    return int.from_bytes(frame[32 + 4 * b: 36 + 4 * b], "little")


def _with_entry(frame, b, e):
    return frame[:32 + 4 * b] + int(e).to_bytes(4, "little") + frame[36 + 4 * b:]


def _full_decode(torch, frame):
    codec = codec_for()
    info = codec.frame_info(frame)
    out = torch.full((info.n_total,), FILL8, dtype=torch.uint8, device="cuda")
    st = torch.zeros(info.n_blocks, dtype=torch.int32, device="cuda")
    res = torch.zeros(2, dtype=torch.int32, device="cuda")
    codec.decompress_frame_into(frame, info, out, st, res)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


@gpu
def test_uncovered_blocks_are_not_decoded(torch_cuda, corpora, frames):
    torch = torch_cuda
    raw = corpora[1000]
    good = frames().cpu().numpy().tobytes()
    pos, ln = _record_pos(good, 6)
    cut = min(24, ln // 2)  # the payload's last bytes; the lengths in the directory still add up
    bad = good[:pos + ln - cut] + bytes(x ^ 0xFF for x in good[pos + ln - cut: pos + ln]) + good[pos + ln:]
    frame = dev(torch, np.frombuffer(bad, dtype=np.uint8))
    check_ok(torch, frame, raw, [(0, 2 * BLOCK, 0)])
    check_ok(torch, frame, raw, [(7, 2 * BLOCK - 9, 1), (7 * BLOCK, BLOCK + 1000, 2 * BLOCK)])
    # a range over block 6 reports what the whole-frame call reports for it
    full_out, full_st = _full_decode(torch, frame)
    ranges = [(6 * BLOCK - 10, BLOCK + 20, 0)]
    out, st, res = run(torch, frame, ranges)
    assert int(res[0]) == 0 and int(st[0]) == int(full_st[6]) and int(res[1]) == int(full_st[6] != 0)
    if full_st[6] != 0:
        assert np.array_equal(out, expected(raw, ranges, len(out), skip=(6,)))
    else:  # decoded, to other bytes: the same ones
        assert np.array_equal(out[10: 10 + BLOCK], full_out[6 * BLOCK: 7 * BLOCK])
        assert np.array_equal(out[:10], raw[6 * BLOCK - 10: 6 * BLOCK])


# ---------------------------------------------------------------- 7. damaged frames
@gpu
def test_truncated_or_lengthened(torch_cuda, corpora, frames):
    torch = torch_cuda
    good = frames().cpu().numpy().tobytes()
    ranges = [(0, 100, 0), (5000, 0, 100), (BLOCK, 7 * BLOCK, 112)]
    for damaged in (good[:-1], good + b"\x00", good[:32 + 8]):
        out, st, res = run(torch, dev(torch, np.frombuffer(damaged, dtype=np.uint8)), ranges)
        assert int(res[0]) == BAD_FRAME and int(res[1]) == len(ranges)
        assert (st == BAD_FRAME).all(), st
        assert (out == FILL8).all(), "a rejected frame must leave d_out untouched"


@gpu
@pytest.mark.parametrize("k", [2, 7])
def test_type_3_entry(torch_cuda, corpora, frames, k):
    """A type-3 entry on a RAW block keeps the directory consistent: block k alone is lost."""
    torch = torch_cuda
    raw = corpora[1000]
    good = frames().cpu().numpy().tobytes()
    assert R.types_of(good)[k] == R.RAW
    frame = dev(torch, np.frombuffer(_with_entry(good, k, 3 << 30 | _entry(good, k) & 0x3FFFFFFF), dtype=np.uint8))
    n = len(raw)
    ranges = [(0, n, 0),                                  # direct, touches k
              (k * BLOCK - 5, 10, n + 7),                 # bounce, touches k
              (0, BLOCK + 3, n + 32),                     # does not touch k
              (k * BLOCK + 100, 50, n + 32 + BLOCK + 9),  # inside k
              ((k + 1) * BLOCK, 20, n + 3 * BLOCK),       # right after k
              (0, 0, 1)]
    for chunk in (0, 2):
        out, st, res = run(torch, frame, ranges, chunk_blocks=chunk)
        assert list(st) == [BAD_FRAME, BAD_FRAME, 0, BAD_FRAME, 0, 0], st
        assert list(res) == [0, 3], res
        assert np.array_equal(out, expected(raw, ranges, len(out), skip=(k,)))


@gpu
def test_two_failed_blocks_report_the_lower(torch_cuda, corpora, frames):
    torch = torch_cuda
    raw = corpora[1000]
    good = frames().cpu().numpy().tobytes()
    pos, ln = _record_pos(good, 0)
    at = pos + ln - 700  # as tests/test_gpu_frame.py: block 0 then fails in its decoder
    bad = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
    bad = _with_entry(bad, 2, 3 << 30 | _entry(bad, 2) & 0x3FFFFFFF)
    frame = dev(torch, np.frombuffer(bad, dtype=np.uint8))
    _, full_st = _full_decode(torch, frame)
    assert full_st[0] != 0 and full_st[2] == BAD_FRAME and not np.delete(full_st, [0, 2]).any()
    ranges = [(BLOCK - 100, 2 * BLOCK, 0), (2 * BLOCK - 1, 2, 3 * BLOCK), (BLOCK, BLOCK, 3 * BLOCK + 8)]
    out, st, res = run(torch, frame, ranges)
    assert list(st) == [int(full_st[0]), BAD_FRAME, 0] and list(res) == [0, 2]
    assert np.array_equal(out, expected(raw, ranges, len(out), skip=(0, 2)))


# ---------------------------------------------------------------- 8. call-level errors
@gpu
def test_call_level_errors(torch_cuda, corpora, frames):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    n = len(corpora[1000])
    frame = frames()
    codec = codec_for()
    info = codec.frame_info(frame)
    top = 2 ** 64 - 1
    cases = [([(top, 2, 0)], "BAD_ARG"), ([(2, top, 0)], "BAD_ARG"), ([(n, 1, 0)], "BAD_ARG"),
             ([(n - 1, 2, 0)], "BAD_ARG"), ([(0, 2, top)], "BAD_ARG"),
             ([(0, 10, 0), (100, 10, 9)], "BAD_ARG"), ([(0, 10, 5), (0, 10, 0)], "BAD_ARG"),
             ([(0, 10, 1024 - 9)], "DST_TOO_SMALL"), ([(0, 4, 0), (0, 2000, 8)], "DST_TOO_SMALL")]
    ow, out = guarded(torch, 1024, torch.uint8, FILL8)
    st = torch.full((2,), FILL32, dtype=torch.int32, device="cuda")
    res = torch.full((2,), FILL32, dtype=torch.int32, device="cuda")
    for ranges, code in cases:
        with pytest.raises(FseError) as e:
            codec.decompress_frame_ranges_into(frame, info, ranges, out, st, res)
        assert e.value.code == code, (ranges, e.value.code)
    bad_info = codec.frame_info(frame)
    bad_info.n_blocks += 1
    with pytest.raises(FseError) as e:
        codec.decompress_frame_ranges_into(frame, bad_info, [(0, 1, 0)], out, st, res)
    assert e.value.code == "BAD_ARG"
    torch.cuda.synchronize()
    assert bool((ow == FILL8).all()) and bool((st == FILL32).all()) and bool((res == FILL32).all())
    # what stays valid at the edges
    codec.decompress_frame_ranges_into(frame, info, [(n, 0, 1024), (0, 10, 1014)], out, st, res)
    torch.cuda.synchronize()
    assert res.tolist() == [0, 0] and st.tolist() == [0, 0]


# ---------------------------------------------------------------- 9. the Python layer
@gpu
def test_python_layer(torch_cuda, corpora, frames):
    from entropy_coders_amd import FseError, frame_decompress_range

    torch = torch_cuda
    raw = corpora[1000]
    n = len(raw)
    frame = frames()
    codec = codec_for()
    for s, ln in [(0, n), (BLOCK - 1, 2), (n - 1, 1), (17, 0), (BLOCK, 7 * BLOCK)]:
        got = codec.decompress_frame_range(frame, s, ln)
        assert got.dtype == torch.uint8 and got.numel() == ln
        assert got.cpu().numpy().tobytes() == raw[s: s + ln].tobytes()
    pairs = [(5, 100), (0, 0), (4 * BLOCK - 3, 2 * BLOCK), (5, 100)]
    views, st = codec.decompress_frame_ranges(frame, pairs)
    assert not bool(st.any()) and len(views) == len(pairs)
    for v, (s, ln) in zip(views, pairs):
        assert v.cpu().numpy().tobytes() == raw[s: s + ln].tobytes()
    host = frame.cpu().numpy().tobytes()
    assert frame_decompress_range(host, 3 * BLOCK - 1, BLOCK + 2) == raw[3 * BLOCK - 1: 4 * BLOCK + 1].tobytes()
    assert frame_decompress_range(host, n, 0) == b""
    with pytest.raises(FseError) as e:
        frame_decompress_range(b"FSEF" + bytes(60), 0, 1)
    assert e.value.code == "BAD_FRAME"
    with pytest.raises(FseError) as e:
        frame_decompress_range(host, n, 1)
    assert e.value.code == "BAD_ARG"
    # a failed block raises, a range beside it does not
    k = 2
    bad = dev(torch, np.frombuffer(_with_entry(host, k, 3 << 30 | _entry(host, k) & 0x3FFFFFFF), dtype=np.uint8))
    with pytest.raises(FseError) as e:
        codec.decompress_frame_range(bad, k * BLOCK - 1, 2)
    assert e.value.code == "BAD_FRAME"
    assert codec.decompress_frame_range(bad, 0, k * BLOCK).cpu().numpy().tobytes() == raw[: k * BLOCK].tobytes()
    with pytest.raises(FseError) as e:
        codec.decompress_frame_range(frame[:-1], 0, 1)
    assert e.value.code == "BAD_FRAME"
