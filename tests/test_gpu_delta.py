"""The delta frame on the GPU (include/fsehip.h section 2e): the encode and
decode kernels alone against numpy, container bytes against tests/delta_ref.py
(the format restated over the CPU oracle), round trips over the dtypes,
element ranges round the restart boundaries, damaged buffers and stream order.
Expected bytes never come from the code under test; outputs sit between the
guard bands of tests/test_gpu_guard_bands.py."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as DR
import frame_ref as R
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
BAD_FRAME = R.BAD_FRAME
BLOCK, CKPT = 4096, 128
N_ODD = 100003
G = DR.RESTART
# 1023 / 1024 / 1025: the edge of a wave's 64 lanes x 16 elements
SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025, G - 1, G, G + 1, 2 * G + 5]
# the encode grid is capped at 2048 workgroups of 256 lanes x 16 elements, the decode grid at 2048 restart groups
ONE_PASS = 2048 * G
INT_OF = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
WIDTHS = [1, 2, 4, 8]


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


def host_u8(t):
    """A device tensor's bytes as a host uint8 array."""
    import torch

    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def dev_u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def torch_int(torch, w):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w]


def walk(n, w, seed=0, lo=-20, hi=60):
    """A seeded random walk as w-byte integers (it wraps for the narrow ones): what the format is for."""
    rng = np.random.default_rng(0xDE17A + seed)
    return np.cumsum(rng.integers(lo, hi, n)).astype(INT_OF[w])


# ---------------------------------------------------------------- encode and decode alone
def patterns(w, n, rng):
    """name -> n unsigned w-byte integers."""
    u = DR.UINT[w]
    top = (1 << (8 * w)) - 1
    i = np.arange(n, dtype=np.uint64)
    out = {
        "random": np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=u),  # wraps both ways
        "constant": np.full(n, 0xC3A55A3CC3A55A3C & top, dtype=u),
        "rising": (i * np.uint64(3) + np.uint64(top - 100)).astype(u),  # strictly rising, through the wrap
        "min-max": np.where(i % 2 == 0, np.uint64(1) << np.uint64(8 * w - 1), np.uint64(top >> 1)).astype(u),
    }
    if w == 8:  # steps across multiples of 2^32, up and down: the carry between the halves
        out["carry"] = (np.uint64(0xFFFFFFF0) + i * np.uint64(0x7FFFFFFF)).astype(u)
        out["borrow"] = (np.uint64(0x500000010) - i * np.uint64(0x30000001)).astype(u)
    return out


def _encode(torch, w, x, off):
    """fsehip_delta_encode of x at a byte offset below 16, with nothing but poison behind roundup(n * w, 4)."""
    n = len(x)
    raw = DR.raw_bytes(x)
    want = DR.image(raw, w)
    base = torch.full((off + (n * w + 3) // 4 * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    base[off: off + n * w] = torch.from_numpy(raw.copy()).cuda()
    assert base.data_ptr() % 16 == 0
    iw, img = g8(torch, len(want))
    rc = lib().fsehip_delta_encode(w, C.c_void_p(base.data_ptr() + off), n, ptr(img), stream_of(torch))
    assert rc == 0, (w, n, off, rc)
    torch.cuda.synchronize()
    assert_guards(iw, img, A5, f"encode w={w} n={n} off={off}")
    return img.cpu().numpy(), want


def _decode(torch, w, x):
    """fsehip_delta_decode of the reference image into exactly n * w bytes."""
    n = len(x)
    raw = DR.raw_bytes(x)
    want = DR.image(raw, w)
    image = torch.from_numpy(want).cuda() if len(want) else torch.empty(16, dtype=torch.uint8, device="cuda")
    ow, out = g8(torch, n * w)
    rc = lib().fsehip_delta_decode(w, ptr(image), n, ptr(out), stream_of(torch))
    assert rc == 0, (w, n, rc)
    torch.cuda.synchronize()
    assert_guards(ow, out, A5, f"decode w={w} n={n}")
    return out.cpu().numpy(), raw


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_encode_and_decode_against_numpy(torch_cuda, w):
    rng = np.random.default_rng(0x9A7E5 + w)
    for n in SIZES:
        for name, x in patterns(w, n, rng).items():
            for off in (range(0, 16, w) if name == "random" else (0,)):  # every element-aligned offset inside 16 bytes
                got, want = _encode(torch_cuda, w, x, off)
                same(got, want, f"delta image {name} w={w} n={n} off={off}")  # pads included: zero in `want`
            got, want = _decode(torch_cuda, w, x)
            same(got, want, f"decoded elements {name} w={w} n={n}")


@gpu
def test_encode_and_decode_beyond_one_grid_pass(torch_cuda):
    """More restart groups than the capped grids have workgroups: the second pass of both loops, and a ragged end."""
    n = ONE_PASS + G + 3
    x = np.frombuffer(np.random.default_rng(0x9A7E5).integers(0, 256, 2 * n, dtype=np.uint8).tobytes(), dtype="<u2")
    for off in (0, 2):
        got, want = _encode(torch_cuda, 2, x, off)
        same(got, want, f"delta image beyond one pass, off={off}")
    got, want = _decode(torch_cuda, 2, x)
    same(got, want, "decoded elements beyond one pass")


@gpu
def test_python_transforms_and_argument_errors(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    x = torch.from_numpy(walk(5000, 4)).cuda()
    img = codec.delta_encode(x)
    same(img.cpu().numpy(), DR.image(DR.raw_bytes(x.cpu().numpy()), 4), "delta_encode")
    assert torch.equal(codec.delta_decode(img, 5000, torch.int32), x)
    b = torch.arange(300, dtype=torch.uint8, device="cuda")  # a one-byte dtype is accepted here
    assert torch.equal(codec.delta_decode(codec.delta_encode(b), 300, torch.uint8), b)
    with pytest.raises(ValueError, match="contiguous"):
        codec.compress_delta(torch.zeros(10, 4, dtype=torch.int32, device="cuda").t())
    with pytest.raises(ValueError):
        codec.compress_delta(torch.zeros(10, dtype=torch.complex128, device="cuda"))  # 16-byte elements
    buf = codec.compress_delta(x)
    with pytest.raises(ValueError):
        codec.decompress_delta(buf, torch.int16)
    with pytest.raises(ValueError):
        codec.decompress_delta_ranges(buf, torch.int64, [(0, 1)])


# ---------------------------------------------------------------- container bytes
def device_sidecars(torch, codec, image):
    """The zero-filled sidecar array the block encoder fills for the image
    (host uint64), as tests/test_gpu_planes.py passes it to the reference: a
    single-symbol block has no oracle walk."""
    if codec.ckpt_interval == 0 or len(image) == 0:
        return None
    cb = codec.compress(dev_u8(torch, image))
    return cb["sidecar"].cpu().numpy().view(np.uint64)


def _bytes_case(torch, ints, block, ckpt, nstates, table_log=0, offset=1):
    """compress_delta_into of `ints` (a host integer array) at an odd byte
    address against delta_ref, guard bands round every output, then both
    decoders."""
    codec = codec_for(block, ckpt, nstates, table_log)
    w, n = ints.dtype.itemsize, len(ints)
    x = torch.from_numpy(ints).cuda()
    img = DR.image(DR.raw_bytes(ints), w)
    want = DR.build(ints, block, ckpt, nstates, table_log, sidecars=device_sidecars(torch, codec, img))
    cap = codec.delta_bound(n, w)
    assert len(want) <= cap == DR.bound(n, w, block)
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.delta_scratch_bytes(n, w))
    codec.compress_delta_into(x, scratch, out, out_len, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0, (out_len.tolist(), len(want), res.tolist())
    got = bytes(out[: len(want)].cpu().numpy())
    assert got == want
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the delta frame"
    dec, st = codec_for().decompress_delta(out[: len(want)], x.dtype)  # from the odd address
    assert not bool(st.any()) and dec.shape == (n,)
    same(host_u8(dec), DR.raw_bytes(ints), "device round trip")
    assert DR.decode(got)[2].tobytes() == DR.raw_bytes(ints).tobytes()
    return got


FORMATS = [(2, 128, 4096), (2, 0, 65536), (1, 128, 65536), (1, 0, 4096)]


@gpu
@pytest.mark.parametrize("nstates,ckpt,block", FORMATS)
@pytest.mark.parametrize("w", WIDTHS)
def test_bytes_against_the_reference(torch_cuda, w, nstates, ckpt, block):
    got = _bytes_case(torch_cuda, walk(N_ODD, w, w), block, ckpt, nstates, offset=1 + 2 * w)
    assert R.FSE in R.types_of(got[16:])


@gpu
def test_bytes_at_table_log_13(torch_cuda):
    _bytes_case(torch_cuda, walk(N_ODD, 2, 13, -3000, 3001), BLOCK, CKPT, 2, table_log=13, offset=7)


@gpu
def test_bytes_zero_constant_and_tiny(torch_cuda):
    torch = torch_cuda
    zero = _bytes_case(torch, np.zeros(5000, np.int32), BLOCK, CKPT, 2)
    assert set(R.types_of(zero[16:])) == {R.RLE}
    for w in WIDTHS:
        assert len(_bytes_case(torch, np.zeros(0, INT_OF[w]), BLOCK, CKPT, 2)) == 48
        _bytes_case(torch, np.array([0x95], dtype=np.uint8).astype(INT_OF[w]), BLOCK, CKPT, 2)
        _bytes_case(torch, np.full(G + 1, 77, dtype=INT_OF[w]), BLOCK, 0, 1)  # one value per restart, zeros between


@gpu
@pytest.mark.parametrize("w,ckpt,nstates", [(1, 128, 2), (2, 128, 2), (4, 0, 2), (8, 128, 1)])
def test_reference_built_buffers_decode_on_the_device(torch_cuda, w, ckpt, nstates):
    torch = torch_cuda
    ints = walk(20011, w, 11)
    blob = DR.build(ints, BLOCK, ckpt, nstates)  # the oracle's own checkpoints
    assert R.FSE in R.types_of(blob[16:])
    out, st = codec_for().decompress_delta(dev_u8(torch, np.frombuffer(blob, np.uint8)), torch_int(torch, w))
    assert not bool(st.any())
    same(out.cpu().numpy(), ints, "reference-built delta frame")


# ---------------------------------------------------------------- round trips
DTYPES = ["uint8", "int8", "int16", "int32", "int64", "bfloat16", "float32", "float64"]


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_round_trip_dtypes(torch_cuda, name):
    torch = torch_cuda
    dtype = getattr(torch, name)
    n = G + 3
    g = torch.Generator().manual_seed(0xD7 + len(name))
    if dtype.is_floating_point:
        x = (torch.randn(n, generator=g) * 0.02).to(dtype)
    else:
        x = torch.cumsum(torch.randint(-30, 70, (n,), generator=g), 0).to(dtype)
    w = x.element_size()
    codec = codec_for()
    buf = codec.compress_delta(x.cuda())
    info, inner = codec.delta_info(buf)
    assert (info.elem_bytes, info.n_elems, inner.n_total) == (w, n, w * DR.stride_of(n))
    ow, out = g8(torch, n * w)
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    codec.decompress_delta_into(buf, info, inner, scratch, out, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (sw, st, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    assert res.tolist() == [0, 0] and not bool(st.any())
    same(out.cpu().numpy(), DR.raw_bytes(x.view(torch_int(torch, w)).numpy()), name)
    assert DR.decode(host_u8(buf).tobytes())[2].tobytes() == out.cpu().numpy().tobytes()
    got, _ = codec.decompress_delta(buf, dtype)
    assert got.dtype == dtype and got.shape == (n,) and torch.equal(got.cpu(), x)


@gpu
def test_host_helpers(torch_cuda):
    from entropy_coders_amd import delta_compress, delta_decompress

    a = walk(37 * 111, 8, 5).reshape(37, 111)
    blob = delta_compress(a, block_size=BLOCK)
    assert DR.decode(blob)[2].tobytes() == a.tobytes()
    assert len(blob) < 0.3 * a.nbytes
    back = delta_decompress(blob, np.int64)
    assert back.dtype == np.int64 and back.shape == (37 * 111,) and back.tobytes() == a.tobytes()
    assert delta_decompress(blob, np.float64).dtype == np.float64  # the width is stored, the dtype is not
    b = np.arange(1000, dtype=np.uint8)
    assert delta_decompress(delta_compress(b), np.uint8).tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        delta_decompress(blob, np.int32)
    with pytest.raises(ValueError):
        delta_compress(np.zeros(4, np.complex128))


# ---------------------------------------------------------------- element ranges
RANGES = [(100, 50),                                   # inside one restart group
          (4000, 95), (4000, 96), (4000, 97),          # ending at 4095 / 4096 / 4097
          (G - 1, 10), (G, 10), (G + 1, 10),           # starting there
          (G - 1, 1), (G, 1),
          (4000, 2 * G + 200),                         # three restart groups
          (N_ODD - 13, 13),                            # ending at n_elems
          (5000, 0), (N_ODD, 0),                       # empty
          (0, N_ODD)]                                  # the whole tensor as one range


@pytest.fixture(scope="module", params=WIDTHS)
def buffer(request, torch_cuda):
    """(w, host source, its delta frame on the device) for the range and damage tests."""
    torch = torch_cuda
    w = request.param
    ints = walk(N_ODD, w, 2)
    ints.setflags(write=False)
    buf = codec_for().compress_delta(torch.from_numpy(ints.copy()).cuda())
    return w, ints, buf


def _ranges_into(torch, w, buf, triples, dst_elems, byte_shift=0, infos=None):
    """decompress_delta_ranges_into with guard bands round the destination
    (dst_elems elements, starting byte_shift bytes into the guarded array),
    the scratch and the statuses.  Returns (destination bytes, statuses, result)."""
    codec = codec_for()
    info, inner = infos or codec.delta_info(buf)
    dw, whole = g8(torch, byte_shift + w * dst_elems)
    dst = whole[byte_shift:]
    sw, st = g32(torch, len(triples))
    rw, res = g32(torch, 2)
    arr = codec.planes_ranges(triples)
    xw, scratch = g8(torch, max(codec.delta_ranges_scratch_bytes(w, arr), 16))
    codec.decompress_delta_ranges_into(buf, info, inner, arr, scratch, dst, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((dw, whole, A5, "d_out"), (sw, st, F32, "d_range_status"), (rw, res, F32, "d_result"),
                           (xw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert bool((whole[:byte_shift] == A5).all())
    return dst.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy()


def expected_dst(ints, triples, dst_elems):
    w = ints.dtype.itemsize
    want = np.full(w * dst_elems, A5, dtype=np.uint8)
    for s, n, d in triples:
        want[w * d: w * (d + n)] = DR.raw_bytes(ints[s: s + n])
    return want


@gpu
@pytest.mark.parametrize("off,count", RANGES)
def test_one_element_range_at_every_byte_shift(torch_cuda, buffer, off, count):
    w, ints, buf = buffer
    for byte_shift in (range(16) if count < 1000 else (0, 1, w)):
        dst, st, res = _ranges_into(torch_cuda, w, buf, [(off, count, 3)], count + 8, byte_shift)
        assert res.tolist() == [0, 0] and st.tolist() == [0]
        same(dst, expected_dst(ints, [(off, count, 3)], count + 8), f"w={w} range ({off}, {count}) shift {byte_shift}")


@gpu
def test_33_ranges_in_one_call_and_the_empty_list(torch_cuda, buffer):
    torch = torch_cuda
    w, ints, buf = buffer
    triples, at = [], 1
    for s, n in RANGES[:-1] + [(G - 7 + 3 * i, 40 + i) for i in range(20)]:  # 33: one more than a pieces launch takes
        triples.append((s, n, at))
        at += n + (len(triples) % 3)  # gaps of 0..2 elements stay untouched
    assert len(triples) == 33
    dst, st, res = _ranges_into(torch, w, buf, triples, at + 5, byte_shift=1)
    assert res.tolist() == [0, 0] and not st.any()
    same(dst, expected_dst(ints, triples, at + 5), "33 ranges")
    dst, st, res = _ranges_into(torch, w, buf, [], 64)
    assert res.tolist() == [0, 0] and bool((dst == A5).all())
    dt = torch_int(torch, w)
    views, st = codec_for().decompress_delta_ranges(buf, dt, RANGES)
    assert not bool(st.any()) and [v.numel() for v in views] == [n for _, n in RANGES]
    for (s, n), v in zip(RANGES, views):
        same(v.cpu().numpy(), ints[s: s + n], f"view ({s}, {n})")
    one = codec_for().decompress_delta_range(buf, dt, G - 1, 3)
    same(one.cpu().numpy(), ints[G - 1: G + 2], "decompress_delta_range")


@gpu
def test_range_argument_errors(torch_cuda, buffer):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    w, ints, buf = buffer
    for triples, code in (([(N_ODD - 5, 6, 0)], "BAD_ARG"), ([(N_ODD + 1, 0, 0)], "BAD_ARG"),
                          ([(0, 10, 0), (100, 10, 9)], "BAD_ARG"), ([(0, 10, 20), (50, 10, 0), (70, 5, 24)], "BAD_ARG"),
                          ([(0, 10, 60)], "DST_TOO_SMALL")):
        with pytest.raises(FseError) as e:
            _ranges_into(torch, w, buf, triples, 64)
        assert e.value.code == code, (triples, e.value.code)


# ---------------------------------------------------------------- damage
def _decode_into(torch, blob, infos):
    """fsehip_delta_decompress of host bytes with the given (info, inner):
    (output bytes, block statuses, result), guards asserted."""
    codec = codec_for()
    info, inner = infos
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    ow, out = g8(torch, info.n_elems * info.elem_bytes)
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    codec.decompress_delta_into(buf, info, inner, scratch, out, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (sw, st, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return out.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy()


DAMAGE = {
    "magic": lambda b: b"FSEP" + b[4:],
    "version": lambda b: b[:4] + b"\x02" + b[5:],
    "elem_bytes": lambda b: b[:5] + bytes([b[5] ^ 0x10]) + b[6:],
    "n_elems": lambda b: b[:10] + bytes([b[10] ^ 1]) + b[11:],  # 65,536 elements off: another stride
    "truncated": lambda b: b[:-1],
    "truncated-in-the-directory": lambda b: b[:60],
}


@gpu
@pytest.mark.parametrize("name", list(DAMAGE))
def test_damaged_buffers_are_bad_frame(torch_cuda, buffer, name):
    """The device's own checks, given the good buffer's info: BAD_FRAME, every
    status BAD_FRAME, the output untouched -- for the whole decode and for
    ranges.  The host parse rejects the damaged heads on its own."""
    from entropy_coders_amd import BlockCodec, FseError

    torch = torch_cuda
    w, ints, buf = buffer
    good = host_u8(buf).tobytes()
    bad = DAMAGE[name](good)
    infos = BlockCodec.delta_info(good)
    if not name.startswith("truncated"):
        with pytest.raises(FseError) as e:
            BlockCodec.delta_info(bad)
        assert e.value.code == "BAD_FRAME"
    out, st, res = _decode_into(torch, bad, infos)
    assert int(res[0]) == BAD_FRAME and int(res[1]) == infos[1].n_blocks and (st == BAD_FRAME).all(), (res, st[:4])
    assert (out == A5).all(), "a rejected delta frame must leave d_out untouched"
    triples = [(0, 0, 0), (5, 100, 3), (50001, 2, 110)]
    dst, rst, rres = _ranges_into(torch, w, dev_u8(torch, np.frombuffer(bad, np.uint8)), triples, 128, infos=infos)
    assert rres.tolist() == [BAD_FRAME, 3] and (rst == BAD_FRAME).all(), (rres, rst)
    assert (dst == A5).all(), "a rejected delta frame must leave the range destination untouched"


@gpu
def test_damaged_payload_byte_costs_its_restart_groups(torch_cuda, buffer):
    """A flipped byte inside one FSE record of the inner frame: that block
    fails, and every element whose restart group has no byte in it equals the
    source."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    w, ints, buf = buffer
    good = host_u8(buf).tobytes()
    finfo, directory, records = R.split_frame(good[16:])
    stride = DR.stride_of(N_ODD)
    b = next(i for i, (t, _) in enumerate(directory) if t == R.FSE and i >= 3)
    pos = finfo["records_off"] + sum(8 * len(c) + len(d) for c, d in records[:b])
    # the payload's first byte: all bits flipped, its table log is above the frame's, which no decoder can miss
    # (a flip further in can decode to other symbols and still end in step)
    at = 16 + pos + 8 * len(records[b][0])
    bad = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
    with pytest.raises(Exception):
        DR.decode(bad)
    out, st, res = _decode_into(torch, bad, BlockCodec.delta_info(good))
    assert int(res[0]) == 0 and int(res[1]) >= 1 and st[b] < 0, (res, st[b])
    assert not np.delete(st, b).any()
    hit = np.zeros(stride + G, dtype=bool)
    for p in np.arange(b * BLOCK, (b + 1) * BLOCK) % stride:
        hit[p // G * G: p // G * G + G] = True  # the whole restart group of an element with a byte in the block
    keep = ~hit[:N_ODD]
    assert N_ODD - 2 * G <= keep.sum() < N_ODD
    same(out.view(INT_OF[w])[keep], ints[keep], "elements outside the failed block's restart groups")
    # the same buffer through the ranges call: a range in a hit group fails, one in a clean group does not
    e0 = int(np.flatnonzero(hit)[0])
    clean = int(np.flatnonzero(keep)[0]) // G * G
    dst, rst, rres = _ranges_into(torch, w, dev_u8(torch, np.frombuffer(bad, np.uint8)),
                                  [(e0 + G - 20, 20, 0), (clean + 10, 20, 32)], 64)
    assert rres.tolist() == [0, 1] and rst[0] == st[b] and rst[1] == 0, (rres, rst)
    same(dst[32 * w: 52 * w], DR.raw_bytes(ints[clean + 10: clean + 30]), "the range outside the failed block")


# ---------------------------------------------------------------- stream order
class DeltaChain(Chain):
    """encode -> compress -> decompress -> ranges on one stream with no host
    synchronisation, inputs poison until the gate opens."""

    N = 10 * G + 333
    W = 4

    def __init__(self):
        self.ints = walk(self.N, self.W, 9)
        self.image = DR.image(DR.raw_bytes(self.ints), self.W)
        self.want = DR.build(self.ints, BLOCK, CKPT, 2)  # the oracle's checkpoints: no single-symbol block here
        self.triples = [(0, 1, 2), (G - 1, 3, 5), (self.N - 13, 13, 9), (1000, 9000, 40)]
        self.dst_elems = 40 + 9000 + 7
        self.want_dst = expected_dst(self.ints, self.triples, self.dst_elems)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        n, w = self.N, self.W
        self.info, self.inner = BlockCodec.delta_info(self.want)
        self.src = torch.empty(n, dtype=torch.int32, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.ints))]
        self.w_img, self.img = g8(torch, c.delta_scratch_bytes(n, w))
        self.scratch = torch.empty(c.delta_scratch_bytes(n, w), dtype=torch.uint8, device="cuda")
        self.w_buf, self.buf = g8(torch, c.delta_bound(n, w))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.w_out, self.out = g8(torch, w * n)
        self.w_bst, self.bst = g32(torch, self.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.w_dst, self.dst = g8(torch, w * self.dst_elems)
        self.w_rst, self.rst = g32(torch, len(self.triples))
        self.w_rres, self.rres = g32(torch, 2)
        self.arr = c.planes_ranges(self.triples)
        self.rscratch = torch.empty(c.delta_ranges_scratch_bytes(w, self.arr), dtype=torch.uint8, device="cuda")

    def poison(self):
        self.src.fill_(7)
        self.buf.zero_()  # what the decoders read: all zeros is BAD_FRAME
        self.len.fill_(F64)
        for t in (self.img, self.out, self.dst):
            t.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.rst, self.rres):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        rc = c.lib.fsehip_delta_encode(self.W, ptr(self.src), self.N, ptr(self.img), stream_of(self.torch))
        assert rc == 0, rc
        c.compress_delta_into(self.src, self.scratch, self.buf, self.len, self.cres)
        c.decompress_delta_into(buf, self.info, self.inner, self.scratch, self.out, self.bst, self.dres)
        c.decompress_delta_ranges_into(buf, self.info, self.inner, self.arr, self.rscratch, self.dst, self.rst,
                                       self.rres)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_img, self.img, A5, "delta image"), (self.w_buf, self.buf, A5, "d_out"),
                              (self.w_len, self.len, F64, "d_out_len"),
                              (self.w_cres, self.cres, F32, "compress d_result"), (self.w_out, self.out, A5, "elements"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_dst, self.dst, A5, "ranges d_out"), (self.w_rst, self.rst, F32, "d_range_status"),
                              (self.w_rres, self.rres, F32, "ranges d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        same(self.img.cpu().numpy(), self.image, "delta image")
        assert self.len.tolist() == [n], (self.len.tolist(), n)
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "delta frame bytes")
        assert bool((self.buf[n:] == 0).all()), "a store past out_len"
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        same(self.out.cpu().numpy(), DR.raw_bytes(self.ints), "delta frame decode")
        assert self.rres.tolist() == [0, 0] and not bool(self.rst.any()), (self.rres.tolist(), self.rst.tolist())
        same(self.dst.cpu().numpy(), self.want_dst, "range destination")


def test_host_side_of_the_delta_chain():
    chain = DeltaChain()
    assert len(chain.want) < 2 * chain.N and R.FSE in R.types_of(chain.want[16:])
    assert DR.decode(chain.want)[2].tobytes() == chain.ints.tobytes()


@gpu
def test_delta_chain_behind_the_gate(torch_cuda, warm):
    """One encode -> compress -> decompress -> ranges chain behind the gate of
    tests/test_gpu_stream_order.py: every call returns while its inputs are
    still poison, so none of them waits for the stream or reads device data
    on the host."""
    chain = DeltaChain()
    chain.alloc(torch_cuda)
    warm.chains["delta"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["delta"] = warm.run(chain, gated=False)
    behind_gate(warm, "delta")
