"""The plane frame on the GPU (include/fsehip.h section 2d): the split and
merge kernels alone against numpy, container bytes against tests/planes_ref.py
(the format restated over the CPU oracle), round trips over the dtypes, the
size condition on bf16 weights, element ranges, damaged buffers and stream
order.  Expected bytes never come from the code under test; outputs sit
between the guard bands of tests/test_gpu_guard_bands.py."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as R
import planes_ref as PR
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
BAD_FRAME = R.BAD_FRAME
BLOCK, CKPT = 4096, 128
N_ODD = 100003
# the split / merge grid is capped at 2048 workgroups of 256 lanes, 16 elements a lane
ONE_PASS = 2048 * 256 * 16
SIZES = [0, 1, 2, 3, 15, 16, 17, 31, 33, 63, 65, 255, 1021, 4099, 65539]
INT_OF = {2: np.int16, 4: np.int32, 8: np.int64}


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


def randn_ints(torch, n, dtype, seed=0):
    """Seeded randn * 0.02 cast to `dtype`, as a host integer array of the same width."""
    g = torch.Generator().manual_seed(0x5EED0F00 + seed)
    x = (torch.randn(n, generator=g) * 0.02).to(dtype)
    w = x.element_size()
    return x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[w]).numpy().copy()


def torch_int(torch, w):
    return {2: torch.int16, 4: torch.int32, 8: torch.int64}[w]


# ---------------------------------------------------------------- split and merge alone
def _split_merge(torch, w, n, offsets, rng):
    L = lib()
    raw = rng.integers(0, 256, n * w, dtype=np.uint8)
    want = PR.image(raw, w)
    for off in offsets:
        # the source at a w-aligned byte offset below 16, with nothing but poison behind roundup(n * w, 4)
        base = torch.full((off + (n * w + 3) // 4 * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        base[off: off + n * w] = torch.from_numpy(raw).cuda()
        assert base.data_ptr() % 16 == 0
        iw, img = g8(torch, len(want))
        rc = L.fsehip_planes_split(w, C.c_void_p(base.data_ptr() + off), n, ptr(img), stream_of(torch))
        assert rc == 0, (w, n, off, rc)
        torch.cuda.synchronize()
        assert_guards(iw, img, A5, f"split w={w} n={n} off={off}")
        same(img.cpu().numpy(), want, f"plane image w={w} n={n} off={off}")  # pads included: they are zero in `want`
    # merge: the reference image back into exactly n * w bytes
    image = torch.from_numpy(want).cuda() if len(want) else torch.empty(16, dtype=torch.uint8, device="cuda")
    ow, out = g8(torch, n * w)
    rc = L.fsehip_planes_merge(w, ptr(image), n, ptr(out), stream_of(torch))
    assert rc == 0, (w, n, rc)
    torch.cuda.synchronize()
    assert_guards(ow, out, A5, f"merge w={w} n={n}")
    same(out.cpu().numpy(), raw, f"merged elements w={w} n={n}")


@gpu
@pytest.mark.parametrize("w", [2, 4, 8])
def test_split_and_merge_against_numpy(torch_cuda, w):
    rng = np.random.default_rng(0x9A7E5 + w)
    for n in SIZES:
        _split_merge(torch_cuda, w, n, range(0, 16, w), rng)


@gpu
@pytest.mark.parametrize("w", [2, 4, 8])
def test_split_and_merge_beyond_one_grid_pass(torch_cuda, w):
    """More groups than the capped grid has lanes: the grid-stride loop's second pass, and a ragged end."""
    _split_merge(torch_cuda, w, ONE_PASS + 16 * 3 + 5, (0, w), np.random.default_rng(0x9A7E5))


@gpu
def test_python_split_merge_and_argument_errors(torch_cuda):
    torch = torch_cuda
    codec = codec_for()
    x = torch.from_numpy(randn_ints(torch, 1021, torch.float32)).cuda()
    img = codec.planes_split(x)
    same(img.cpu().numpy(), PR.image(PR.raw_bytes(x.cpu().numpy()), 4), "planes_split")
    assert torch.equal(codec.planes_merge(img, 1021, torch.int32), x)
    with pytest.raises(ValueError, match="compress_frame"):
        codec.compress_planes(torch.zeros(10, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        codec.compress_planes(torch.zeros(10, 4, dtype=torch.float32, device="cuda").t())
    buf = codec.compress_planes(x)
    with pytest.raises(ValueError):
        codec.decompress_planes(buf, torch.bfloat16)
    with pytest.raises(ValueError):
        codec.decompress_planes_ranges(buf, torch.float64, [(0, 1)])


# ---------------------------------------------------------------- container bytes
def device_sidecars(torch, codec, image):
    """The zero-filled sidecar array the block encoder fills for the plane
    image (host uint64), as tests/test_gpu_frame.py passes it to the
    reference: a single-symbol block has no oracle walk."""
    if codec.ckpt_interval == 0 or len(image) == 0:
        return None
    cb = codec.compress(dev_u8(torch, image))
    return cb["sidecar"].cpu().numpy().view(np.uint64)


def _bytes_case(torch, ints, block, ckpt, nstates, table_log=0, dtype=None):
    """compress_planes of `ints` (a host integer array; `dtype`: the torch
    dtype the device tensor is viewed as) against planes_ref, then both decoders."""
    codec = codec_for(block, ckpt, nstates, table_log)
    w = ints.dtype.itemsize
    x = torch.from_numpy(ints).cuda()
    if dtype is not None:
        x = x.view(dtype)
    got = host_u8(codec.compress_planes(x)).tobytes()
    img = PR.image(PR.raw_bytes(ints), w)
    want = PR.build(ints, block, ckpt, nstates, table_log, sidecars=device_sidecars(torch, codec, img))
    assert len(got) == len(want) and got == want, (len(got), len(want))
    assert len(got) <= codec.planes_bound(len(ints), w) == PR.bound(len(ints), w, block)
    out, st = codec_for().decompress_planes(dev_u8(torch, np.frombuffer(got, np.uint8)), x.dtype)
    assert not bool(st.any()) and out.shape == (len(ints),)
    same(host_u8(out), PR.raw_bytes(ints), "device round trip")
    assert PR.decode(got)[2].tobytes() == PR.raw_bytes(ints).tobytes()
    return got


@gpu
def test_bytes_bf16_weights_and_the_size_condition(torch_cuda):
    """131,072 bf16 weights at 64 KiB blocks: exact bytes, two of the four
    blocks RAW, and the plane frame under 0.9 of the byte frame of the same
    tensor (the CPU reference gives 0.841; 0.9 is the condition)."""
    torch = torch_cuda
    ints = randn_ints(torch, 131072, torch.bfloat16)
    got = _bytes_case(torch, ints, 65536, 128, 2, dtype=torch.bfloat16)
    assert R.types_of(got[16:]) == [R.RAW, R.RAW, R.FSE, R.FSE]
    codec = codec_for(65536, 128, 2)
    plain = codec.compress_frame(torch.from_numpy(ints).cuda().view(torch.uint8))
    ref_plain = R.build_frame(PR.raw_bytes(ints), 65536, 128, 2)
    assert plain.numel() == len(ref_plain)
    print(f"\n[planes] bf16 131,072: plane frame {len(got)} B, byte frame {plain.numel()} B, "
          f"ratio {len(got) / plain.numel():.3f}")
    assert len(got) < 0.9 * plain.numel()


@gpu
@pytest.mark.parametrize("w,dtype", [(2, "bfloat16"), (4, "float32"), (8, "float64")])
def test_bytes_odd_length_at_4k_blocks(torch_cuda, w, dtype):
    torch = torch_cuda
    _bytes_case(torch, randn_ints(torch, N_ODD, getattr(torch, dtype), w), BLOCK, CKPT, 2)


@gpu
@pytest.mark.parametrize("nstates,ckpt,table_log", [(2, 0, 0), (1, 128, 0), (1, 0, 0), (2, 128, 13)])
def test_bytes_other_formats(torch_cuda, nstates, ckpt, table_log):
    torch = torch_cuda
    _bytes_case(torch, randn_ints(torch, N_ODD, torch.float16, 7), BLOCK, ckpt, nstates, table_log)


@gpu
def test_bytes_small_integers_zero_and_tiny(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(0x1D5)
    idx = rng.integers(0, 1000, 65536, dtype=np.int32)  # stride 65,536: 16 blocks a plane, none straddles
    got = _bytes_case(torch, idx, BLOCK, CKPT, 2)
    types = R.types_of(got[16:])
    assert len(types) == 64 and set(types[32:]) == {R.RLE}, types  # planes 2 and 3 are zero
    zero = _bytes_case(torch, np.zeros(5000, np.int16), BLOCK, CKPT, 2)
    assert set(R.types_of(zero[16:])) == {R.RLE}
    assert len(_bytes_case(torch, np.zeros(0, np.int64), BLOCK, CKPT, 2)) == 48
    for w in (2, 4, 8):
        _bytes_case(torch, np.array([-12345], dtype=INT_OF[w]), BLOCK, CKPT, 2)
        _bytes_case(torch, np.array([-12345], dtype=INT_OF[w]), BLOCK, 0, 1)


@gpu
@pytest.mark.parametrize("offset", [1, 7, 16])
def test_plane_frame_at_any_byte_address(torch_cuda, offset):
    """compress_planes_into at an odd address, guard bands round every
    output; only the first out_len bytes are written; decoded from there."""
    torch = torch_cuda
    codec = codec_for()
    ints = randn_ints(torch, 4099, torch.float32, 3)
    x = torch.from_numpy(ints).cuda()
    want = PR.build(ints, BLOCK, CKPT, 2, sidecars=device_sidecars(torch, codec, PR.image(PR.raw_bytes(ints), 4)))
    cap = codec.planes_bound(4099, 4)
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.planes_scratch_bytes(4099, 4))
    codec.compress_planes_into(x, scratch, out, out_len, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0
    assert bytes(out[: len(want)].cpu().numpy()) == want
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the plane frame"
    got, st = codec.decompress_planes(out[: len(want)], torch.float32)
    assert not bool(st.any()) and torch.equal(got.view(torch.int32), x)


# ---------------------------------------------------------------- round trips
DTYPES = ["bfloat16", "float16", "float32", "float64", "int16", "int32", "int64"]


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_round_trip_dtypes(torch_cuda, name):
    torch = torch_cuda
    dtype = getattr(torch, name)
    g = torch.Generator().manual_seed(0xD7 + len(name))
    if dtype.is_floating_point:
        x = (torch.randn(4099, generator=g) * 0.02).to(dtype)
    else:
        x = torch.randint(-300, 70000, (4099,), generator=g).to(dtype)
    codec = codec_for()
    buf = codec.compress_planes(x.cuda())
    info, inner = codec.planes_info(buf)
    assert (info.elem_bytes, info.n_elems, inner.n_total) == (x.element_size(), 4099, x.element_size() * 4112)
    ow, out = g8(torch, 4099 * x.element_size())
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    codec.decompress_planes_into(buf, info, inner, scratch, out, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (sw, st, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    assert res.tolist() == [0, 0] and not bool(st.any())
    same(out.cpu().numpy(), PR.raw_bytes(x.view(torch_int(torch, x.element_size())).numpy()), name)
    got, _ = codec.decompress_planes(buf, dtype)
    assert got.dtype == dtype and got.shape == (4099,) and torch.equal(got.cpu(), x)


@gpu
def test_round_trip_constant_planes_and_host_helpers(torch_cuda):
    torch = torch_cuda
    from entropy_coders_amd import planes_compress, planes_decompress

    codec = codec_for()
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.ones(10000, dtype=dtype, device="cuda")  # every plane one repeated byte, some non-zero
        buf = codec.compress_planes(x)
        assert buf.numel() < 0.2 * x.numel() * x.element_size()
        out, st = codec.decompress_planes(buf, dtype)
        assert not bool(st.any()) and torch.equal(out, x)
    a = np.random.default_rng(5).normal(0, 0.02, (37, 111)).astype(np.float32)
    blob = planes_compress(a, block_size=BLOCK)
    assert PR.decode(blob)[2].tobytes() == a.tobytes()
    back = planes_decompress(blob, np.float32)
    assert back.dtype == np.float32 and back.shape == (37 * 111,) and back.tobytes() == a.tobytes()
    with pytest.raises(ValueError):
        planes_decompress(blob, np.float64)
    with pytest.raises(ValueError):
        planes_compress(np.zeros(4, np.uint8))


@gpu
@pytest.mark.parametrize("w,dtype,ckpt,nstates", [(2, "bfloat16", 128, 2), (4, "float32", 0, 2), (8, "float64", 128, 1)])
def test_reference_built_buffers_decode_on_the_device(torch_cuda, w, dtype, ckpt, nstates):
    torch = torch_cuda
    ints = randn_ints(torch, 20011, getattr(torch, dtype), 11)
    blob = PR.build(ints, BLOCK, ckpt, nstates)  # the oracle's own checkpoints
    assert R.FSE in R.types_of(blob[16:])
    out, st = codec_for().decompress_planes(dev_u8(torch, np.frombuffer(blob, np.uint8)), torch_int(torch, w))
    assert not bool(st.any())
    same(out.cpu().numpy(), ints, "reference-built plane frame")


# ---------------------------------------------------------------- element ranges
RANGES = [(0, 0), (0, 1), (1, 1), (4095, 3), (50001, 2), (99990, 13), (12345, 30000), (0, N_ODD)]


@pytest.fixture(scope="module")
def bf16_buffer(torch_cuda):
    """(host int16 source, its plane frame on the device) for the range and damage tests."""
    torch = torch_cuda
    ints = randn_ints(torch, N_ODD, torch.bfloat16, 2)
    ints.setflags(write=False)
    buf = codec_for().compress_planes(torch.from_numpy(ints.copy()).cuda().view(torch.bfloat16))
    return ints, buf


def _ranges_into(torch, buf, triples, dst_elems, byte_shift=0, infos=None):
    """decompress_planes_ranges_into with guard bands round the destination
    (dst_elems int16 elements, starting byte_shift bytes into the guarded
    array) and the statuses.  Returns (destination bytes, statuses, result)."""
    codec = codec_for()
    info, inner = infos or codec.planes_info(buf)
    dw, whole = g8(torch, byte_shift + 2 * dst_elems)
    dst = whole[byte_shift:]
    sw, st = g32(torch, len(triples))
    rw, res = g32(torch, 2)
    arr = codec.planes_ranges(triples)
    xw, scratch = g8(torch, max(codec.planes_ranges_scratch_bytes(2, arr), 16))
    codec.decompress_planes_ranges_into(buf, info, inner, arr, scratch, dst, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((dw, whole, A5, "d_out"), (sw, st, F32, "d_range_status"), (rw, res, F32, "d_result"),
                           (xw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert bool((whole[:byte_shift] == A5).all())
    return dst.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy()


def expected_dst(ints, triples, dst_elems):
    want = np.full(2 * dst_elems, A5, dtype=np.uint8)
    for s, n, d in triples:
        want[2 * d: 2 * (d + n)] = PR.raw_bytes(ints[s: s + n])
    return want


@gpu
@pytest.mark.parametrize("off,count", RANGES)
@pytest.mark.parametrize("byte_shift", [0, 1])
def test_one_element_range(torch_cuda, bf16_buffer, off, count, byte_shift):
    ints, buf = bf16_buffer
    dst, st, res = _ranges_into(torch_cuda, buf, [(off, count, 3)], count + 8, byte_shift)
    assert res.tolist() == [0, 0] and st.tolist() == [0]
    same(dst, expected_dst(ints, [(off, count, 3)], count + 8), f"range ({off}, {count})")


@gpu
def test_all_ranges_in_one_call_and_the_empty_list(torch_cuda, bf16_buffer):
    torch = torch_cuda
    ints, buf = bf16_buffer
    triples, at = [], 1
    for s, n in RANGES + [(7, 40)] * 40:  # more ranges than one pieces launch takes
        triples.append((s, n, at))
        at += n + (len(triples) % 3)  # gaps of 0..2 elements stay untouched
    dst, st, res = _ranges_into(torch, buf, triples, at + 5)
    assert res.tolist() == [0, 0] and not st.any()
    same(dst, expected_dst(ints, triples, at + 5), "all ranges")
    dst, st, res = _ranges_into(torch, buf, [], 64)
    assert res.tolist() == [0, 0] and bool((dst == A5).all())
    views, st = codec_for().decompress_planes_ranges(buf, torch.bfloat16, RANGES)
    assert not bool(st.any()) and [v.numel() for v in views] == [n for _, n in RANGES]
    for (s, n), v in zip(RANGES, views):
        same(v.view(torch.int16).cpu().numpy(), ints[s: s + n], f"view ({s}, {n})")
    one = codec_for().decompress_planes_range(buf, torch.bfloat16, 4095, 3)
    same(one.view(torch.int16).cpu().numpy(), ints[4095: 4098], "decompress_planes_range")


@gpu
def test_a_whole_tensor_as_one_range(torch_cuda):
    """2^20 elements at 64 KiB blocks: every plane range is a run of whole
    blocks at an aligned place in the scratch (the frame call's direct route)."""
    torch = torch_cuda
    n = 1 << 20
    ints = randn_ints(torch, n, torch.bfloat16, 4)
    buf = codec_for(65536, 128, 2).compress_planes(torch.from_numpy(ints).cuda())
    dst, st, res = _ranges_into(torch, buf, [(0, n, 0)], n)
    assert res.tolist() == [0, 0] and st.tolist() == [0]
    same(dst, PR.raw_bytes(ints), "whole tensor as one range")


@gpu
def test_range_argument_errors(torch_cuda, bf16_buffer):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    ints, buf = bf16_buffer
    for triples, code in (([(N_ODD - 5, 6, 0)], "BAD_ARG"), ([(N_ODD + 1, 0, 0)], "BAD_ARG"),
                          ([(0, 10, 0), (100, 10, 9)], "BAD_ARG"), ([(0, 10, 20), (50, 10, 0), (70, 5, 24)], "BAD_ARG"),
                          ([(0, 10, 60)], "DST_TOO_SMALL")):
        with pytest.raises(FseError) as e:
            _ranges_into(torch, buf, triples, 64)
        assert e.value.code == code, (triples, e.value.code)


# ---------------------------------------------------------------- damage
def _decode_into(torch, blob, infos):
    """fsehip_planes_decompress of host bytes with the given (info, inner):
    (output bytes, block statuses, result), guards asserted."""
    codec = codec_for()
    info, inner = infos
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    ow, out = g8(torch, info.n_elems * info.elem_bytes)
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    codec.decompress_planes_into(buf, info, inner, scratch, out, st, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (sw, st, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return out.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy()


DAMAGE = {
    "magic": lambda b: b"FSEF" + b[4:],
    "elem_bytes-3": lambda b: b[:5] + b"\x03" + b[6:],
    "inner-n_total-plus-16": lambda b: b[:32] + (int.from_bytes(b[32:40], "little") + 16).to_bytes(8, "little") + b[40:],
    "truncated": lambda b: b[:-1],
    "truncated-in-the-directory": lambda b: b[:60],
}


@gpu
@pytest.mark.parametrize("name", list(DAMAGE))
def test_damaged_buffers_are_bad_frame(torch_cuda, bf16_buffer, name):
    """The device's own checks, given the good buffer's info: BAD_FRAME, every
    status BAD_FRAME, the output untouched -- for the whole decode and for
    ranges.  The host parse rejects the damaged heads on its own."""
    from entropy_coders_amd import BlockCodec, FseError

    torch = torch_cuda
    ints, buf = bf16_buffer
    good = host_u8(buf).tobytes()
    bad = DAMAGE[name](good)
    infos = BlockCodec.planes_info(good)
    if not name.startswith("truncated"):
        with pytest.raises(FseError) as e:
            BlockCodec.planes_info(bad)
        assert e.value.code == "BAD_FRAME"
    out, st, res = _decode_into(torch, bad, infos)
    assert int(res[0]) == BAD_FRAME and int(res[1]) == infos[1].n_blocks and (st == BAD_FRAME).all(), (res, st[:4])
    assert (out == A5).all(), "a rejected plane frame must leave d_out untouched"
    triples = [(0, 0, 0), (5, 100, 3), (50001, 2, 110)]
    dst, rst, rres = _ranges_into(torch, dev_u8(torch, np.frombuffer(bad, np.uint8)), triples, 128, infos=infos)
    assert rres.tolist() == [BAD_FRAME, 3] and (rst == BAD_FRAME).all(), (rres, rst)
    assert (dst == A5).all(), "a rejected plane frame must leave the range destination untouched"


@gpu
def test_damaged_payload_byte_costs_one_block(torch_cuda, bf16_buffer):
    """A flipped byte inside one FSE record of the inner frame: that block
    fails, and every element with no byte in it equals the source."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    ints, buf = bf16_buffer
    good = host_u8(buf).tobytes()
    inner = good[16:]
    finfo, directory, records = R.split_frame(inner)
    stride = PR.stride_of(N_ODD)
    b = next(i for i, (t, _) in enumerate(directory) if t == R.FSE and i * BLOCK >= stride + BLOCK)  # inside plane 1
    pos = finfo["records_off"] + sum(8 * len(c) + len(d) for c, d in records[:b])
    at = 16 + pos + 8 * len(records[b][0]) + len(records[b][1]) - 700
    bad = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
    out, st, res = _decode_into(torch, bad, BlockCodec.planes_info(good))
    assert int(res[0]) == 0 and int(res[1]) >= 1 and st[b] != 0, (res, st[b])
    assert not np.delete(st, b).any()
    pos_in_image = np.arange(b * BLOCK, (b + 1) * BLOCK)
    hit = np.zeros(stride, dtype=bool)
    hit[pos_in_image % stride] = True
    keep = ~hit[:N_ODD]
    assert keep.sum() == N_ODD - BLOCK
    same(out.view(np.int16)[keep], ints[keep], "elements outside the failed block")
    # the same buffer through the ranges call: a range inside the block fails, one outside does not
    e0 = (b * BLOCK) % stride
    dst, rst, rres = _ranges_into(torch, dev_u8(torch, np.frombuffer(bad, np.uint8)),
                                  [(e0 + 10, 20, 0), (e0 + BLOCK + 10, 20, 32)], 64)
    assert rres.tolist() == [0, 1] and rst[0] == st[b] and rst[1] == 0, (rres, rst)
    same(dst[64: 104], PR.raw_bytes(ints[e0 + BLOCK + 10: e0 + BLOCK + 30]), "the range outside the failed block")


# ---------------------------------------------------------------- stream order
class PlanesChain(Chain):
    """compress -> decompress -> ranges on one stream with no host
    synchronisation, inputs poison until the gate opens."""

    N = 40 * BLOCK // 2 + 333

    def __init__(self):
        import torch

        self.ints = randn_ints(torch, self.N, torch.bfloat16, 9)
        self.want = PR.build(self.ints, BLOCK, CKPT, 2)  # the oracle's checkpoints: no single-symbol block here
        self.triples = [(0, 1, 2), (4095, 3, 5), (self.N - 13, 13, 9), (1000, 9000, 40)]
        self.dst_elems = 40 + 9000 + 7
        self.want_dst = expected_dst(self.ints, self.triples, self.dst_elems)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        n = self.N
        self.info, self.inner = BlockCodec.planes_info(self.want)
        self.src = torch.empty(n, dtype=torch.int16, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.ints))]
        self.scratch = torch.empty(c.planes_scratch_bytes(n, 2), dtype=torch.uint8, device="cuda")
        self.w_buf, self.buf = g8(torch, c.planes_bound(n, 2))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.w_out, self.out = g8(torch, 2 * n)
        self.w_bst, self.bst = g32(torch, self.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.w_dst, self.dst = g8(torch, 2 * self.dst_elems)
        self.w_rst, self.rst = g32(torch, len(self.triples))
        self.w_rres, self.rres = g32(torch, 2)
        self.arr = c.planes_ranges(self.triples)
        self.rscratch = torch.empty(c.planes_ranges_scratch_bytes(2, self.arr), dtype=torch.uint8, device="cuda")

    def poison(self):
        self.src.fill_(7)
        self.buf.zero_()  # what the decoders read: all zeros is BAD_FRAME
        self.len.fill_(F64)
        for t in (self.out, self.dst):
            t.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.rst, self.rres):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        c.compress_planes_into(self.src, self.scratch, self.buf, self.len, self.cres)
        c.decompress_planes_into(buf, self.info, self.inner, self.scratch, self.out, self.bst, self.dres)
        c.decompress_planes_ranges_into(buf, self.info, self.inner, self.arr, self.rscratch, self.dst, self.rst,
                                        self.rres)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_buf, self.buf, A5, "d_out"), (self.w_len, self.len, F64, "d_out_len"),
                              (self.w_cres, self.cres, F32, "compress d_result"), (self.w_out, self.out, A5, "elements"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_dst, self.dst, A5, "ranges d_out"), (self.w_rst, self.rst, F32, "d_range_status"),
                              (self.w_rres, self.rres, F32, "ranges d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        assert self.len.tolist() == [n], (self.len.tolist(), n)
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "plane frame bytes")
        assert bool((self.buf[n:] == 0).all()), "a store past out_len"
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        same(self.out.cpu().numpy(), PR.raw_bytes(self.ints), "plane frame decode")
        assert self.rres.tolist() == [0, 0] and not bool(self.rst.any()), (self.rres.tolist(), self.rst.tolist())
        same(self.dst.cpu().numpy(), self.want_dst, "range destination")


def test_host_side_of_the_planes_chain():
    chain = PlanesChain()
    assert len(chain.want) < 2 * chain.N and R.FSE in R.types_of(chain.want[16:])


@gpu
def test_planes_chain_behind_the_gate(torch_cuda, warm):
    """One compress -> decompress -> ranges chain behind the gate of
    tests/test_gpu_stream_order.py: every call returns while its inputs are
    still poison, so none of them waits for the stream or reads device data
    on the host."""
    chain = PlanesChain()
    chain.alloc(torch_cuda)
    warm.chains["planes"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["planes"] = warm.run(chain, gated=False)
    behind_gate(warm, "planes")
