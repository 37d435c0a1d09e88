"""The diff frame on the GPU (include/fsehip.h section 2h): the encode and
decode kernels alone against numpy -- every width, both sources at every
alignment, in place and out of place -- container bytes against
tests/diff_ref.py (the format restated over the CPU oracle), round trips over
the dtypes, element ranges, damaged buffers, sealed buffers with a wrong base
and stream order.  Expected bytes never come from the code under test; outputs
sit between the guard bands of tests/test_gpu_guard_bands.py.

The capped grid of fse_planes_dev.hpp is 2048 workgroups of 256 lanes, 16
elements a lane: one pass covers 2^23 elements, so 2^23 + 53 makes lane 0..3 of
the first workgroup take a second trip, the last of them a ragged one."""
import ctypes as C

import numpy as np
import pytest

import check_ref as CR
import diff_ref as DF
import frame_ref as R
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
BAD_FRAME = R.BAD_FRAME
CHECKSUM = -21
BLOCK, CKPT = 4096, 128
N_ODD = 70001
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65541]
ONE_PASS = 2048 * 256 * 16
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

    if t.numel() == 0:  # (an empty tensor has no stride to view through)
        return np.zeros(0, dtype=np.uint8)
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def dev_u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def torch_int(torch, w):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w]


def version_pair(n, w, seed=0, lo=-20, hi=60):
    """(x, base) as w-byte integers: a seeded random walk and the same walk
    moved by a little noise -- what the format is for."""
    rng = np.random.default_rng(0xD1FF + seed)
    base = np.cumsum(rng.integers(-2000, 2001, n)).astype(INT_OF[w])
    x = (base + rng.integers(lo, hi, n).astype(INT_OF[w])).astype(INT_OF[w])
    return x, base


# ---------------------------------------------------------------- encode and decode alone
def uint(w, values):
    """Python / uint64 values reduced mod 2^(8 w) as the w-byte unsigned array."""
    return np.asarray(values, dtype=np.uint64).astype(DF.UINT[w])


def patterns(w, n, rng):
    """name -> (x, base), n unsigned w-byte integers each."""
    u = DF.UINT[w]
    rand = lambda: np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=u)  # noqa: E731
    i = np.arange(n, dtype=np.uint64)
    r = rand()
    # 2^(8 (k + 1)) for k = i % w: the carry out of byte k, the top one wrapping to 0 (at w = 8, k = 3: 2^32)
    edge = np.array([(1 << (8 * (k + 1))) % (1 << (8 * w)) for k in range(w)], dtype=np.uint64)[(i % np.uint64(w)).astype(int)]
    half = np.uint64(1) << np.uint64(8 * w - 1)
    return {
        "identical": (r, r.copy()),
        "random": (rand(), rand()),  # wraps both ways
        "zero-base": (r, np.zeros(n, dtype=u)),
        "carry-up": (uint(w, edge), uint(w, edge - np.uint64(1))),    # x = b + 1 across the carry of every byte
        "carry-down": (uint(w, edge - np.uint64(1)), uint(w, edge)),  # x = b - 1 across the borrow of every byte
        "half": (uint(w, r.astype(np.uint64) + half), r),             # d = 2^(8 w - 1): zigzag's all-ones
        "sign-flip": (uint(w, np.uint64(0) - r.astype(np.uint64)), r),  # x = -b
    }


def placed(torch, raw, off):
    """`raw` at byte `off` of a fresh 16-byte aligned allocation that ends at
    roundup(off + len, 4) + a band of poison: (the allocation, the address)."""
    n = len(raw)
    whole = torch.full((off + (n + 3) // 4 * 4 + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    if n:
        whole[off: off + n] = torch.from_numpy(np.array(raw, dtype=np.uint8)).cuda()
    assert whole.data_ptr() % 16 == 0
    return whole, C.c_void_p(whole.data_ptr() + off)


def _encode(torch, w, x, b, xoff=0, boff=0):
    """fsehip_diff_encode with each source at its own byte offset below 16 and nothing but poison behind either."""
    n = len(x)
    want = DF.image(DF.raw_bytes(x), DF.raw_bytes(b), w)
    xs, xp = placed(torch, DF.raw_bytes(x), xoff)
    bs, bp = placed(torch, DF.raw_bytes(b), boff)
    iw, img = g8(torch, len(want))
    rc = lib().fsehip_diff_encode(w, xp, bp, n, ptr(img), stream_of(torch))
    assert rc == 0, (w, n, xoff, boff, rc)
    torch.cuda.synchronize()
    assert_guards(iw, img, A5, f"encode w={w} n={n} off={xoff},{boff}")
    return img.cpu().numpy(), want


def _decode(torch, w, x, b, boff=0):
    """fsehip_diff_decode of the reference image against the base at a byte offset into exactly n * w bytes."""
    n = len(x)
    want = DF.image(DF.raw_bytes(x), DF.raw_bytes(b), w)
    image = torch.from_numpy(want).cuda() if len(want) else torch.empty(16, dtype=torch.uint8, device="cuda")
    bs, bp = placed(torch, DF.raw_bytes(b), boff)
    ow, out = g8(torch, n * w)
    rc = lib().fsehip_diff_decode(w, ptr(image), n, ptr(out), bp, stream_of(torch))
    assert rc == 0, (w, n, boff, rc)
    torch.cuda.synchronize()
    assert_guards(ow, out, A5, f"decode w={w} n={n} off={boff}")
    return out.cpu().numpy(), DF.raw_bytes(x)


def _decode_in_place(torch, w, x, b):
    """fsehip_diff_decode with d_dst == d_base: the base becomes x, and nothing round it changes."""
    n = len(x)
    want = DF.image(DF.raw_bytes(x), DF.raw_bytes(b), w)
    image = torch.from_numpy(want).cuda() if len(want) else torch.empty(16, dtype=torch.uint8, device="cuda")
    bw, base = g8(torch, n * w)
    if n:
        base.copy_(torch.from_numpy(DF.raw_bytes(b).copy()).cuda())
    rc = lib().fsehip_diff_decode(w, ptr(image), n, ptr(base), ptr(base), stream_of(torch))
    assert rc == 0, (w, n, rc)
    torch.cuda.synchronize()
    assert_guards(bw, base, A5, f"in-place decode w={w} n={n}")
    return base.cpu().numpy(), DF.raw_bytes(x)


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_encode_and_decode_against_numpy(torch_cuda, w):
    rng = np.random.default_rng(0xD1FFE + w)
    for n in SIZES:
        for name, (x, b) in patterns(w, n, rng).items():
            got, want = _encode(torch_cuda, w, x, b)
            same(got, want, f"diff image {name} w={w} n={n}")  # pads included: zero in `want`
            got, want = _decode(torch_cuda, w, x, b)
            same(got, want, f"decoded elements {name} w={w} n={n}")
            got, want = _decode_in_place(torch_cuda, w, x, b)
            same(got, want, f"decoded in place {name} w={w} n={n}")


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_both_sources_at_every_alignment(torch_cuda, w):
    """n = 37: two whole groups and a ragged one of 5; x and the base each at
    every element-aligned byte offset inside 16, independently."""
    rng = np.random.default_rng(0xA119 + w)
    x, b = patterns(w, 37, rng)["random"]
    for xoff in range(0, 16, w):
        for boff in range(0, 16, w):
            got, want = _encode(torch_cuda, w, x, b, xoff, boff)
            same(got, want, f"diff image w={w} offsets {xoff}, {boff}")
    for boff in range(0, 16, w):
        got, want = _decode(torch_cuda, w, x, b, boff)
        same(got, want, f"decoded elements w={w} base offset {boff}")


@gpu
@pytest.mark.parametrize("w", [1, 2])
def test_encode_and_decode_beyond_one_grid_pass(torch_cuda, w):
    """More 16-element groups than the capped grid has lanes: the second trip of all three loops, and a ragged end."""
    n = ONE_PASS + 53
    rng = np.random.default_rng(0xB16 + w)
    b = np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=DF.UINT[w])
    x = (b + rng.integers(0, 7, n).astype(DF.UINT[w])).astype(DF.UINT[w])
    got, want = _encode(torch_cuda, w, x, b, w, 16 - w)
    same(got, want, "diff image beyond one pass")
    got, want = _decode(torch_cuda, w, x, b, w)
    same(got, want, "decoded elements beyond one pass")
    got, want = _decode_in_place(torch_cuda, w, x, b)
    same(got, want, "decoded in place beyond one pass")


@gpu
def test_python_transforms_and_argument_errors(torch_cuda):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    codec = codec_for()
    xi, bi = version_pair(5000, 4)
    x, b = torch.from_numpy(xi).cuda(), torch.from_numpy(bi).cuda()
    img = codec.diff_encode(x, b)
    same(img.cpu().numpy(), DF.image(DF.raw_bytes(xi), DF.raw_bytes(bi), 4), "diff_encode")
    assert torch.equal(codec.diff_decode(img, b), x)
    out = torch.empty_like(b)
    assert codec.diff_decode(img, b, out=out) is out and torch.equal(out, x)
    assert not bool(codec.diff_encode(x, x).any())  # src == base: both only read
    big = torch.zeros(5000 + 64, dtype=torch.int32, device="cuda")
    big[:5000] = b
    with pytest.raises(FseError) as e:  # overlapping, not equal
        codec.diff_decode(img, big[:5000], out=big[4:5004])
    assert e.value.code == "BAD_ARG" and torch.equal(big[:5000], b)
    buf = codec.compress_diff(x, b)
    with pytest.raises(FseError) as e:
        codec.decompress_diff(buf, big[:5000], out=big[8:5008])
    assert e.value.code == "BAD_ARG" and torch.equal(big[:5000], b)
    with pytest.raises(FseError) as e:  # the ranges call: no overlap at all, the base itself included
        info, inner = codec.diff_info(buf)
        scratch = torch.empty(codec.diff_ranges_scratch_bytes(4, [(0, 10, 0)]), dtype=torch.uint8, device="cuda")
        codec.decompress_diff_ranges_into(buf, info, inner, [(0, 10, 0)], b, scratch, b,
                                          torch.zeros(1, dtype=torch.int32, device="cuda"),
                                          torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert e.value.code == "BAD_ARG"
    for bad in (None, b[:4999], b.to(torch.float32), b.to(torch.int64), b.cpu(),
                torch.zeros(5000, 2, dtype=torch.int32, device="cuda")[:, 0]):
        with pytest.raises(ValueError):
            codec.compress_diff(x, bad)
        if bad is None or bad.dtype != torch.float32:  # the width is stored, the dtype is not: the base's is taken
            with pytest.raises(ValueError):
                codec.decompress_diff(buf, bad)
    assert codec.decompress_diff(buf, b.view(torch.float32))[0].dtype == torch.float32
    for bad_out in (torch.empty(4999, dtype=torch.int32, device="cuda"),
                    torch.empty(5000, dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            codec.decompress_diff(buf, b, out=bad_out)
    with pytest.raises(ValueError, match="contiguous"):
        t2 = torch.zeros(10, 4, dtype=torch.int32, device="cuda").t()
        codec.compress_diff(t2, t2)
    with pytest.raises(ValueError):
        z = torch.zeros(10, dtype=torch.complex128, device="cuda")  # 16-byte elements
        codec.compress_diff(z, z)
    with pytest.raises(ValueError, match="base"):
        codec.decompress_auto(buf, torch.int32)
    got, st = codec.decompress_auto(buf, torch.int32, base=b)
    assert torch.equal(got, x) and not bool(st.any())


# ---------------------------------------------------------------- container bytes
def device_sidecars(torch, codec, image):
    """The zero-filled sidecar array the block encoder fills for the image
    (host uint64), as tests/test_gpu_planes.py passes it to the reference: a
    single-symbol block has no oracle walk."""
    if codec.ckpt_interval == 0 or len(image) == 0:
        return None
    cb = codec.compress(dev_u8(torch, image))
    return cb["sidecar"].cpu().numpy().view(np.uint64)


def _bytes_case(torch, ints, base, block, ckpt, nstates, table_log=0, offset=1):
    """compress_diff_into of `ints` against `base` (host integer arrays) at an
    odd byte address against diff_ref, guard bands round every output, then
    the device decoder out of place and in place, and the reference's."""
    codec = codec_for(block, ckpt, nstates, table_log)
    w, n = ints.dtype.itemsize, len(ints)
    x, b = torch.from_numpy(ints).cuda(), torch.from_numpy(base).cuda()
    img = DF.image(DF.raw_bytes(ints), DF.raw_bytes(base), w)
    want = DF.build(ints, base, block, ckpt, nstates, table_log, sidecars=device_sidecars(torch, codec, img))
    cap = codec.diff_bound(n, w)
    assert len(want) <= cap == DF.bound(n, w, block)
    ww, whole = g8(torch, offset + cap)
    whole.zero_()
    out = whole[offset:]
    lw, out_len = g64(torch, 1)
    rw, res = g32(torch, 2)
    sw, scratch = g8(torch, codec.diff_scratch_bytes(n, w))
    codec.compress_diff_into(x, b, scratch, out, out_len, res)
    torch.cuda.synchronize()
    for w_, v, f, what in ((ww, whole, A5, "d_out"), (lw, out_len, F64, "d_out_len"), (rw, res, F32, "d_result"),
                           (sw, scratch, A5, "d_scratch")):
        assert_guards(w_, v, f, what)
    assert out_len.tolist() == [len(want)] and res.tolist()[0] == 0, (out_len.tolist(), len(want), res.tolist())
    got = bytes(out[: len(want)].cpu().numpy())
    assert got == want
    assert not bool(whole[:offset].any()) and not bool(out[len(want):].any()), "a store outside the diff frame"
    assert torch.equal(b.cpu(), torch.from_numpy(base)), "the encode side only reads the base"
    dec, st = codec_for().decompress_diff(out[: len(want)], b)  # from the odd address
    assert not bool(st.any()) and dec.shape == (n,) and dec.dtype == b.dtype
    same(host_u8(dec), DF.raw_bytes(ints), "device round trip")
    dec, st = codec_for().decompress_diff(out[: len(want)], b, out=b)
    assert dec is b and not bool(st.any())
    same(host_u8(b), DF.raw_bytes(ints), "device round trip in place")
    assert DF.decode(got, base)[2].tobytes() == DF.raw_bytes(ints).tobytes()
    return got


FORMATS = [(2, 128, 4096), (2, 0, 65536), (1, 128, 65536), (1, 0, 4096)]


@gpu
@pytest.mark.parametrize("nstates,ckpt,block", FORMATS)
@pytest.mark.parametrize("w", WIDTHS)
def test_bytes_against_the_reference(torch_cuda, w, nstates, ckpt, block):
    x, b = version_pair(N_ODD, w, w)
    got = _bytes_case(torch_cuda, x, b, block, ckpt, nstates, offset=1 + 2 * w)
    assert R.FSE in R.types_of(got[16:])


@gpu
def test_bytes_at_table_log_13(torch_cuda):
    x, b = version_pair(N_ODD, 2, 13, -3000, 3001)
    _bytes_case(torch_cuda, x, b, BLOCK, CKPT, 2, table_log=13, offset=7)


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_bytes_identical_empty_and_tiny(torch_cuda, w):
    torch = torch_cuda
    x, _ = version_pair(5000, w, 3)
    same_as_base = _bytes_case(torch, x, x.copy(), BLOCK, CKPT, 2)
    n_blocks = R.n_blocks_of(w * DF.stride_of(5000), BLOCK)
    assert set(R.types_of(same_as_base[16:])) == {R.RLE} and len(same_as_base) == 16 + 32 + 5 * n_blocks
    e = np.zeros(0, INT_OF[w])
    assert len(_bytes_case(torch, e, e, BLOCK, CKPT, 2)) == 48
    one = np.array([0x95], dtype=np.uint8).astype(INT_OF[w])
    _bytes_case(torch, one, one + 3, BLOCK, CKPT, 2)
    for n in (15, 17, 4097):
        x, b = version_pair(n, w, n)
        _bytes_case(torch, x, b, BLOCK, 0, 1)


@gpu
@pytest.mark.parametrize("w,ckpt,nstates", [(1, 128, 2), (2, 128, 2), (4, 0, 2), (8, 128, 1)])
def test_reference_built_buffers_decode_on_the_device(torch_cuda, w, ckpt, nstates):
    torch = torch_cuda
    x, b = version_pair(20011, w, 11)
    blob = DF.build(x, b, BLOCK, ckpt, nstates)  # the oracle's own checkpoints
    assert R.FSE in R.types_of(blob[16:])
    out, st = codec_for().decompress_diff(dev_u8(torch, np.frombuffer(blob, np.uint8)), torch.from_numpy(b).cuda())
    assert not bool(st.any())
    same(out.cpu().numpy(), x, "reference-built diff frame")


# ---------------------------------------------------------------- round trips
DTYPES = ["uint8", "int8", "int16", "int32", "int64", "bfloat16", "float32", "float64"]


@gpu
@pytest.mark.parametrize("name", DTYPES)
def test_round_trip_dtypes(torch_cuda, name):
    torch = torch_cuda
    dtype = getattr(torch, name)
    n = 4099
    g = torch.Generator().manual_seed(0xD7 + len(name))
    if dtype.is_floating_point:
        master = torch.randn(n, generator=g) * 0.02
        b, x = master.to(dtype), (master + 1e-4 * torch.randn(n, generator=g)).to(dtype)
    else:
        b = torch.cumsum(torch.randint(-30, 70, (n,), generator=g), 0).to(dtype)
        x = (b + torch.randint(-3, 4, (n,), generator=g).to(dtype)).to(dtype)
    w = x.element_size()
    codec = codec_for()
    db = b.cuda()
    buf = codec.compress_diff(x.cuda(), db)
    info, inner = codec.diff_info(buf)
    assert (info.elem_bytes, info.n_elems, inner.n_total) == (w, n, w * DF.stride_of(n))
    ow, out = g8(torch, n * w)
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    rc = lib().fsehip_diff_decompress(C.byref(info), C.byref(inner), 0, ptr(buf), buf.numel(), ptr(scratch),
                                      scratch.numel(), ptr(out), ptr(db), out.numel(), ptr(st), ptr(res),
                                      stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (sw, st, F32, "d_block_status"), (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    assert res.tolist() == [0, 0] and not bool(st.any())
    int_view = lambda t: t.view(torch_int(torch, w)).numpy()  # noqa: E731
    same(out.cpu().numpy(), DF.raw_bytes(int_view(x)), name)
    assert DF.decode(host_u8(buf).tobytes(), int_view(b))[2].tobytes() == out.cpu().numpy().tobytes()
    got, _ = codec.decompress_diff(buf, db)
    assert got.dtype == dtype and got.shape == (n,) and torch.equal(got.cpu().view(torch_int(torch, w)),
                                                                    x.view(torch_int(torch, w)))
    if w > 1:
        assert buf.numel() < codec.compress_planes(x.cuda()).numel()


@gpu
def test_host_helpers(torch_cuda):
    from entropy_coders_amd import (FseError, auto_decompress, container_kind, diff_compress, diff_decompress,
                                    planes_compress, sealed_compress, sealed_decompress)

    x, b = version_pair(37 * 111, 8, 5)
    x, b = x.reshape(37, 111), b.reshape(37, 111)
    blob = diff_compress(x, b, block_size=BLOCK)
    assert container_kind(blob) == "diff"
    assert DF.decode(blob, b)[2].tobytes() == x.tobytes()
    assert len(blob) < 0.5 * len(planes_compress(x, block_size=BLOCK))
    back = diff_decompress(blob, b)
    assert back.dtype == np.int64 and back.shape == (37 * 111,) and back.tobytes() == x.tobytes()
    assert diff_decompress(blob, b.view(np.float64)).dtype == np.float64  # the width is stored, the dtype is not
    assert auto_decompress(blob, np.int64, base=b).tobytes() == x.tobytes()
    with pytest.raises(ValueError, match="base"):
        auto_decompress(blob, np.int64)
    c = np.arange(1000, dtype=np.uint8)
    assert diff_decompress(diff_compress(c, c[::-1]), c[::-1]).tobytes() == c.tobytes()
    for bad in (b.astype(np.int32), b.reshape(-1)[:-1], None):
        with pytest.raises(ValueError):
            diff_decompress(blob, bad)
        with pytest.raises(ValueError):
            diff_compress(x, bad)
    with pytest.raises(ValueError):
        z = np.zeros(4, np.complex128)
        diff_compress(z, z)
    sealed = sealed_compress(x, kind="diff", base=b, block_size=BLOCK)
    assert container_kind(sealed) == "sealed"
    assert sealed_decompress(sealed, np.int64, base=b).tobytes() == x.tobytes()
    other = b.copy()
    other[3, 5] += 1
    with pytest.raises(FseError) as e:
        sealed_decompress(sealed, np.int64, base=other)
    assert e.value.code == "CHECKSUM"
    with pytest.raises(ValueError, match="base"):
        sealed_decompress(sealed, np.int64)
    with pytest.raises(ValueError):
        sealed_compress(x, kind="diff")


# ---------------------------------------------------------------- element ranges
RANGES = [(0, 1), (0, 50),                             # at the first element
          (N_ODD - 1, 1), (N_ODD - 13, 13),            # at the last
          (4000, 200), (4095, 2), (4096, 5),           # across the inner frame's first block boundary (plane 0)
          (65530, 20),                                 # and a 64 KiB one
          (100, 3), (101, 4), (102, 7),                # the bytewise tail of a range: 3, 0 and 3 elements
          (5000, 0), (N_ODD, 0),                       # empty
          (0, N_ODD)]                                  # the whole tensor as one range


@pytest.fixture(scope="module", params=WIDTHS)
def buffer(request, torch_cuda):
    """(w, host source, host base, the diff frame and the base on the device) for the range and damage tests."""
    torch = torch_cuda
    w = request.param
    ints, base = version_pair(N_ODD, w, 2)
    ints.setflags(write=False)
    base.setflags(write=False)
    db = torch.from_numpy(base.copy()).cuda()
    buf = codec_for().compress_diff(torch.from_numpy(ints.copy()).cuda(), db)
    return w, ints, base, buf, db


def _ranges_into(torch, w, buf, db, triples, dst_elems, byte_shift=0, infos=None):
    """decompress_diff_ranges_into with guard bands round the destination
    (dst_elems elements, starting byte_shift bytes into the guarded array),
    the scratch and the statuses.  Returns (destination bytes, statuses, result)."""
    codec = codec_for()
    info, inner = infos or codec.diff_info(buf)
    dw, whole = g8(torch, byte_shift + w * dst_elems)
    dst = whole[byte_shift:]
    sw, st = g32(torch, len(triples))
    rw, res = g32(torch, 2)
    arr = codec.planes_ranges(triples)
    xw, scratch = g8(torch, max(codec.diff_ranges_scratch_bytes(w, arr), 16))
    rc = codec.lib.fsehip_diff_decompress_ranges(
        C.byref(info), C.byref(inner), 0, ptr(buf), buf.numel(), arr, len(triples), ptr(scratch), scratch.numel(),
        ptr(dst), ptr(db), dst.numel(), ptr(st), ptr(res), stream_of(torch))
    if rc:
        from entropy_coders_amd import FseError

        raise FseError(rc, "fsehip_diff_decompress_ranges")
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
        want[w * d: w * (d + n)] = DF.raw_bytes(ints[s: s + n])
    return want


@gpu
@pytest.mark.parametrize("off,count", RANGES)
def test_one_element_range_at_every_byte_shift(torch_cuda, buffer, off, count):
    w, ints, base, buf, db = buffer
    for byte_shift in (range(16) if count < 1000 else (0, 1, w)):
        dst, st, res = _ranges_into(torch_cuda, w, buf, db, [(off, count, 3)], count + 8, byte_shift)
        assert res.tolist() == [0, 0] and st.tolist() == [0]
        same(dst, expected_dst(ints, [(off, count, 3)], count + 8), f"w={w} range ({off}, {count}) shift {byte_shift}")


@gpu
def test_33_ranges_in_one_call_and_the_empty_list(torch_cuda, buffer):
    torch = torch_cuda
    w, ints, base, buf, db = buffer
    triples, at = [], 1
    for s, n in RANGES[:-1] + [(4089 + 3 * i, 40 + i) for i in range(20)]:  # 33: one more than a pieces launch takes
        triples.append((s, n, at))
        at += n + (len(triples) % 3)  # gaps of 0..2 elements stay untouched
    assert len(triples) == 33
    dst, st, res = _ranges_into(torch, w, buf, db, triples, at + 5, byte_shift=1)
    assert res.tolist() == [0, 0] and not st.any()
    same(dst, expected_dst(ints, triples, at + 5), "33 ranges")
    dst, st, res = _ranges_into(torch, w, buf, db, [], 64)
    assert res.tolist() == [0, 0] and bool((dst == A5).all())
    views, st = codec_for().decompress_diff_ranges(buf, db, RANGES)
    assert not bool(st.any()) and [v.numel() for v in views] == [n for _, n in RANGES]
    for (s, n), v in zip(RANGES, views):
        assert v.dtype == db.dtype
        same(v.cpu().numpy(), ints[s: s + n], f"view ({s}, {n})")
    one = codec_for().decompress_diff_range(buf, db, 4095, 3)
    same(one.cpu().numpy(), ints[4095: 4098], "decompress_diff_range")
    same(db.cpu().numpy(), base, "the ranges call only reads the base")


@gpu
def test_range_argument_errors(torch_cuda, buffer):
    from entropy_coders_amd import FseError

    torch = torch_cuda
    w, ints, base, buf, db = buffer
    for triples, code in (([(N_ODD - 5, 6, 0)], "BAD_ARG"), ([(N_ODD + 1, 0, 0)], "BAD_ARG"),
                          ([(0, 10, 0), (100, 10, 9)], "BAD_ARG"), ([(0, 10, 20), (50, 10, 0), (70, 5, 24)], "BAD_ARG"),
                          ([(0, 10, 60)], "DST_TOO_SMALL")):
        with pytest.raises(FseError) as e:
            _ranges_into(torch, w, buf, db, triples, 64)
        assert e.value.code == code, (triples, e.value.code)
    with pytest.raises(ValueError):
        codec_for().decompress_diff_ranges(buf, db[:-1], [(0, 1)])


# ---------------------------------------------------------------- damage
def _decode_into(torch, blob, infos, base, in_place=False):
    """fsehip_diff_decompress of host bytes with the given (info, inner)
    against the host array `base`: (output bytes, block statuses, result,
    the base's bytes afterwards), guards asserted.  in_place: d_out == d_base."""
    info, inner = infos
    buf = dev_u8(torch, np.frombuffer(blob, np.uint8))
    nbytes = info.n_elems * info.elem_bytes
    bw, db = g8(torch, nbytes)
    db.copy_(torch.from_numpy(DF.raw_bytes(base).copy()).cuda())
    ow, out = (bw, db) if in_place else g8(torch, nbytes)
    sw, st = g32(torch, inner.n_blocks)
    rw, res = g32(torch, 2)
    scratch = torch.empty(inner.n_total, dtype=torch.uint8, device="cuda")
    rc = lib().fsehip_diff_decompress(C.byref(info), C.byref(inner), 0, ptr(buf), buf.numel(), ptr(scratch),
                                      scratch.numel(), ptr(out), ptr(db), nbytes, ptr(st), ptr(res), stream_of(torch))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for w_, v, f, what in ((ow, out, A5, "d_out"), (bw, db, A5, "d_base"), (sw, st, F32, "d_block_status"),
                           (rw, res, F32, "d_result")):
        assert_guards(w_, v, f, what)
    return out.cpu().numpy(), st.cpu().numpy(), res.cpu().numpy(), db.cpu().numpy()


DAMAGE = {
    "magic-FSEP": lambda b: b"FSEP" + b[4:],
    "magic-FSED": lambda b: b"FSED" + b[4:],
    "magic-FSEF": lambda b: b"FSEF" + b[4:],
    "version": lambda b: b[:4] + b"\x02" + b[5:],
    "elem_bytes": lambda b: b[:5] + bytes([b[5] ^ 0x10]) + b[6:],
    "n_elems": lambda b: b[:10] + bytes([b[10] ^ 1]) + b[11:],  # 65,536 elements off: the header differs from `info`
    "truncated": lambda b: b[:-1],
    "truncated-in-the-directory": lambda b: b[:60],
}


@gpu
@pytest.mark.parametrize("name", list(DAMAGE))
def test_damaged_buffers_are_bad_frame(torch_cuda, buffer, name):
    """The device's own checks, given the good buffer's info: BAD_FRAME, every
    status BAD_FRAME, the output untouched -- for the whole decode, for the
    in-place decode (the base untouched) and for ranges.  The host parse
    rejects the damaged heads on its own."""
    from entropy_coders_amd import BlockCodec, FseError

    torch = torch_cuda
    w, ints, base, buf, db = buffer
    good = host_u8(buf).tobytes()
    bad = DAMAGE[name](good)
    infos = BlockCodec.diff_info(good)
    if not name.startswith("truncated"):
        with pytest.raises(FseError) as e:
            BlockCodec.diff_info(bad)
        assert e.value.code == "BAD_FRAME"
    out, st, res, after = _decode_into(torch, bad, infos, base)
    assert int(res[0]) == BAD_FRAME and int(res[1]) == infos[1].n_blocks and (st == BAD_FRAME).all(), (res, st[:4])
    assert (out == A5).all(), "a rejected diff frame must leave d_out untouched"
    same(after, DF.raw_bytes(base), "the base after a rejected decode")
    out, st, res, after = _decode_into(torch, bad, infos, base, in_place=True)
    assert int(res[0]) == BAD_FRAME and (st == BAD_FRAME).all(), (res, st[:4])
    same(after, DF.raw_bytes(base), "the base after a rejected in-place decode")
    triples = [(0, 0, 0), (5, 100, 3), (50001, 2, 110)]
    dst, rst, rres = _ranges_into(torch, w, dev_u8(torch, np.frombuffer(bad, np.uint8)), db, triples, 128, infos=infos)
    assert rres.tolist() == [BAD_FRAME, 3] and (rst == BAD_FRAME).all(), (rres, rst)
    assert (dst == A5).all(), "a rejected diff frame must leave the range destination untouched"


@gpu
def test_damaged_payload_byte_costs_only_its_own_elements(torch_cuda, buffer):
    """A flipped byte inside one FSE record of the inner frame: that block
    fails, and every element without a byte in it equals the source -- out of
    place and in place."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    w, ints, base, buf, db = buffer
    good = host_u8(buf).tobytes()
    finfo, directory, records = R.split_frame(good[16:])
    stride = DF.stride_of(N_ODD)
    b = next(i for i, (t, _) in enumerate(directory) if t == R.FSE and i >= 3)
    pos = finfo["records_off"] + sum(8 * len(c) + len(d) for c, d in records[:b])
    # the payload's first byte: all bits flipped, its table log is above the frame's, which no decoder can miss
    at = 16 + pos + 8 * len(records[b][0])
    bad = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
    with pytest.raises(Exception):
        DF.decode(bad, base)
    hit = np.zeros(stride, dtype=bool)
    hit[np.arange(b * BLOCK, (b + 1) * BLOCK) % stride] = True  # the elements with a byte in the block
    keep = ~hit[:N_ODD]
    assert N_ODD - BLOCK <= keep.sum() < N_ODD
    for in_place in (False, True):
        out, st, res, _ = _decode_into(torch, bad, BlockCodec.diff_info(good), base, in_place)
        assert int(res[0]) == 0 and int(res[1]) >= 1 and st[b] < 0, (res, st[b])
        assert not np.delete(st, b).any()
        same(out.view(INT_OF[w])[keep], ints[keep], f"elements outside the failed block, in_place={in_place}")
    # the same buffer through the ranges call: a range with an element in the block fails, one beside it does not
    e0 = int(np.flatnonzero(hit)[0])
    clean = int(np.flatnonzero(keep)[0])
    dst, rst, rres = _ranges_into(torch, w, dev_u8(torch, np.frombuffer(bad, np.uint8)), db,
                                  [(e0, 20, 0), (clean, 20, 32)], 64)
    assert rres.tolist() == [0, 1] and rst[0] == st[b] and rst[1] == 0, (rres, rst)
    same(dst[32 * w: 52 * w], DF.raw_bytes(ints[clean: clean + 20]), "the range outside the failed block")


# ---------------------------------------------------------------- sealed
@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_sealed_diff_buffer(torch_cuda, w):
    """Layout against check_ref over diff_ref, the round trip, ranges, and a
    wrong base: every block status OK, CHECKSUM for exactly the check block of
    the changed element."""
    from entropy_coders_amd import BlockCodec, FseError, _lib

    torch = torch_cuda
    codec = codec_for()
    n, check_block = 20011, 4096
    ints, base = version_pair(n, w, 21)
    x, b = torch.from_numpy(ints).cuda(), torch.from_numpy(base).cuda()
    img = DF.image(DF.raw_bytes(ints), DF.raw_bytes(base), w)
    want = CR.record(DF.raw_bytes(ints), 12) + DF.build(ints, base, BLOCK, CKPT, 2,
                                                       sidecars=device_sidecars(torch, codec, img))
    buf = codec.compress_sealed(x, kind="diff", check_block=check_block, base=b)
    assert host_u8(buf).tobytes() == want
    info, kind, off = BlockCodec.sealed_info(buf)
    assert kind == "diff" and _lib.SEALED_KINDS.index(kind) == 3 and off == CR.record_bytes(n * w, 12)
    assert info.n_content == n * w
    out, st, cs, res = codec.decompress_sealed(buf, base=b, with_result=True)
    assert out.dtype == b.dtype and torch.equal(out, x)
    assert not bool(st.any()) and not bool(cs.any()) and res.tolist() == [0, 0]
    views, rst, rcs = codec.decompress_sealed_ranges(buf, None, [(0, 5), (4000, 3000), (n - 1, 1)], base=b)
    assert not bool(rst.any()) and not bool(rcs.any())
    same(views[1].cpu().numpy(), ints[4000:7000], "sealed diff range")
    assert torch.equal(codec.decompress_sealed_range(buf, b.dtype, n - 7, 7, base=b), x[n - 7:])
    # one element of the base changed
    e = 9001
    wrong = b.clone()
    wrong[e] += 1
    out, st, cs, res = codec.decompress_sealed(buf, base=wrong, with_result=True)
    assert not bool(st.any()), "the container cannot tell a wrong base"
    cb = e * w // check_block
    assert cs.tolist() == [CHECKSUM if i == cb else 0 for i in range(info.n_cb)]
    assert res.tolist() == [CHECKSUM, 1]
    keep = np.arange(n) != e
    same(out.cpu().numpy()[keep], ints[keep], "every other element")
    with pytest.raises(FseError) as err:
        codec.decompress_sealed_range(buf, None, cb * check_block // w, 2 * check_block // w, base=wrong)
    assert err.value.code == "CHECKSUM"
    with pytest.raises(ValueError, match="base"):
        codec.decompress_sealed(buf)
    with pytest.raises(ValueError):
        codec.compress_sealed(x, kind="diff")
    with pytest.raises(ValueError):
        codec.compress_sealed(x, kind="delta", base=b)
    plain = codec.compress_sealed(x, kind="delta")  # existing calls without base behave as before
    assert torch.equal(codec.decompress_sealed(plain, b.dtype)[0], x)


# ---------------------------------------------------------------- stream order
class DiffChain(Chain):
    """encode -> compress -> decompress -> ranges -> in-place decompress on
    one stream with no host synchronisation, inputs poison until the gate
    opens."""

    N = 40000 + 333
    W = 4

    def __init__(self):
        self.ints, self.base = version_pair(self.N, self.W, 9)
        self.image = DF.image(DF.raw_bytes(self.ints), DF.raw_bytes(self.base), self.W)
        self.want = DF.build(self.ints, self.base, BLOCK, CKPT, 2)  # the oracle's checkpoints: no single-symbol block
        self.triples = [(0, 1, 2), (4095, 3, 5), (self.N - 13, 13, 9), (1000, 9000, 40)]
        self.dst_elems = 40 + 9000 + 7
        self.want_dst = expected_dst(self.ints, self.triples, self.dst_elems)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = codec_for()
        n, w = self.N, self.W
        self.info, self.inner = BlockCodec.diff_info(self.want)
        self.src = torch.empty(n, dtype=torch.int32, device="cuda")
        self.dbase = torch.empty(n, dtype=torch.int32, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.ints)), (self.dbase, pinned(torch, self.base))]
        self.w_img, self.img = g8(torch, c.diff_scratch_bytes(n, w))
        self.scratch = torch.empty(c.diff_scratch_bytes(n, w), dtype=torch.uint8, device="cuda")
        self.w_buf, self.buf = g8(torch, c.diff_bound(n, w))
        self.w_len, self.len = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.w_out, self.out = g32(torch, n)
        self.w_bst, self.bst = g32(torch, self.inner.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.w_dst, self.dst8 = g8(torch, w * self.dst_elems)
        self.dst = self.dst8.view(torch.int32)
        self.w_rst, self.rst = g32(torch, len(self.triples))
        self.w_rres, self.rres = g32(torch, 2)
        self.w_ist, self.ist = g32(torch, self.inner.n_blocks)
        self.w_ires, self.ires = g32(torch, 2)
        self.arr = c.planes_ranges(self.triples)
        self.rscratch = torch.empty(c.diff_ranges_scratch_bytes(w, self.arr), dtype=torch.uint8, device="cuda")

    def poison(self):
        self.src.fill_(7)
        self.dbase.fill_(9)
        self.buf.zero_()  # what the decoders read: all zeros is BAD_FRAME
        self.len.fill_(F64)
        for t in (self.img, self.dst8):
            t.fill_(A5)
        for t in (self.out, self.cres, self.bst, self.dres, self.rst, self.rres, self.ist, self.ires):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        buf = self.buf[: len(self.want)]  # the expected length: out_len itself stays on the device
        rc = c.lib.fsehip_diff_encode(self.W, ptr(self.src), ptr(self.dbase), self.N, ptr(self.img),
                                      stream_of(self.torch))
        assert rc == 0, rc
        c.compress_diff_into(self.src, self.dbase, self.scratch, self.buf, self.len, self.cres)
        c.decompress_diff_into(buf, self.info, self.inner, self.dbase, self.scratch, self.out, self.bst, self.dres)
        c.decompress_diff_ranges_into(buf, self.info, self.inner, self.arr, self.dbase, self.rscratch, self.dst,
                                      self.rst, self.rres)
        c.decompress_diff_into(buf, self.info, self.inner, self.dbase, self.scratch, self.dbase, self.ist, self.ires)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_img, self.img, A5, "diff image"), (self.w_buf, self.buf, A5, "d_out"),
                              (self.w_len, self.len, F64, "d_out_len"),
                              (self.w_cres, self.cres, F32, "compress d_result"), (self.w_out, self.out, F32, "elements"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_dst, self.dst8, A5, "ranges d_out"), (self.w_rst, self.rst, F32, "d_range_status"),
                              (self.w_rres, self.rres, F32, "ranges d_result"),
                              (self.w_ist, self.ist, F32, "in-place d_block_status"),
                              (self.w_ires, self.ires, F32, "in-place d_result")):
            assert_guards(w, v, f, name)
        n = len(self.want)
        same(self.img.cpu().numpy(), self.image, "diff image")
        assert self.len.tolist() == [n], (self.len.tolist(), n)
        same(self.buf[:n].cpu().numpy(), np.frombuffer(self.want, dtype=np.uint8), "diff frame bytes")
        assert bool((self.buf[n:] == 0).all()), "a store past out_len"
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        same(self.out.cpu().numpy(), self.ints, "diff frame decode")
        assert self.rres.tolist() == [0, 0] and not bool(self.rst.any()), (self.rres.tolist(), self.rst.tolist())
        same(self.dst8.cpu().numpy(), self.want_dst, "range destination")
        assert self.ires.tolist() == [0, 0] and not bool(self.ist.any())
        same(self.dbase.cpu().numpy(), self.ints, "the base after the in-place decode")


def test_host_side_of_the_diff_chain():
    chain = DiffChain()
    assert len(chain.want) < 2 * chain.N and R.FSE in R.types_of(chain.want[16:])
    assert DF.decode(chain.want, chain.base)[2].tobytes() == chain.ints.tobytes()


@gpu
def test_diff_chain_behind_the_gate(torch_cuda, warm):
    """One encode -> compress -> decompress -> ranges -> in-place chain behind
    the gate of tests/test_gpu_stream_order.py: every call returns while its
    inputs are still poison, so none of them waits for the stream or reads
    device data on the host."""
    chain = DiffChain()
    chain.alloc(torch_cuda)
    warm.chains["diff"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code; workspaces grow here
    warm.enqueue_ms["diff"] = warm.run(chain, gated=False)
    behind_gate(warm, "diff")
