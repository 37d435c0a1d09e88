"""The estimate with a base on the GPU (include/fsehip.h section 2i) against
tests/estimate_diff_ref.py: the diff image's histogram between guard bands,
fsehip_estimate_base, compress_auto / compress_sealed(kind="auto") /
auto_compress with a base, and the estimate chain behind the gate of
tests/test_gpu_stream_order.py.  Shapes are those of tests/test_gpu_estimate.py:
ragged groups, tile edges, plane starts inside blocks, blocks below and above
one 4,096-byte tile (the histogram's two paths), more tiles than one workgroup
takes.  Expected numbers never come from the code under test."""
import ctypes as C

import numpy as np
import pytest

import diff_ref as D
import estimate_diff_ref as X
import estimate_ref as E
import frame_ref as R
import planes_ref as PR
from test_gpu_estimate import BLOCKS, INT_OF, SIZES, codec_for, host_u8, lib, stream_of, to_dev, torch_cuda  # noqa: F401
from test_gpu_guard_bands import FILL, assert_guards, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

F32, F64 = FILL["int32"], FILL["int64"]
CHECKSUM = -21
MASKS = [m for m in range(1, 24) if not m & 8]  # bits 0, 1, 2 and 4
NAMES5 = ("frame", "planes", "delta", None, "diff")


def named(est):
    return {NAMES5[k]: v for k, v in enumerate(est) if NAMES5[k] and v != X.NONE}


def pairs(w, n):
    """name -> (x, base): n unsigned w-byte integers each."""
    rng = np.random.default_rng(0xD1FF + 16 * w + n)
    u = D.UINT[w]
    top = (1 << (8 * w)) - 1

    def rand():
        return np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=u).copy()

    b = rand()
    # 2^(8 k) - 1 for k = 1..w in turn: +1 carries into byte k (at w = 8, k = 4: from the low dword into the high one)
    ones = np.array([(1 << (8 * k)) - 1 for k in range(1, w + 1)], dtype=np.uint64)[np.arange(n) % w].astype(u)
    one, half = np.array(1, dtype=u), np.array(1 << (8 * w - 1), dtype=u)
    return {
        "identical": (b.copy(), b),
        "random": (rand(), b),
        "zero-base": (b, np.zeros(n, dtype=u)),
        "small-step": (b + rng.integers(-3, 4, n).astype(np.int64).astype(u), b),  # mod 2^(8 w)
        "carry-up": (ones + one, ones),
        "carry-down": (ones, ones + one),
        "zero-against-ones": (np.zeros(n, dtype=u), np.full(n, top, dtype=u)),
        "ones-against-zero": (np.full(n, top, dtype=u), np.zeros(n, dtype=u)),
        "half-range": (b + half, b),
    }


# ---------------------------------------------------------------- the diff image's histogram
def diff_histogram(torch, w, x, b, bs, src=None, base=None):
    """fsehip_diff_image_histogram into guarded counts: (rc, uint32 [n_blocks, 256])."""
    n = len(x)
    nb = R.n_blocks_of(w * PR.stride_of(n), bs)
    src = torch.from_numpy(PR.raw_bytes(x).copy()).cuda() if src is None else src
    base = torch.from_numpy(PR.raw_bytes(b).copy()).cuda() if base is None else base
    wc, counts = g32(torch, nb * 256)
    rc = lib().fsehip_diff_image_histogram(w, ptr(src), ptr(base), n, bs, ptr(counts), stream_of(torch))
    torch.cuda.synchronize()
    assert_guards(wc, counts, F32, f"w={w} n={n} bs={bs}")
    return rc, counts.cpu().numpy().view(np.uint32).reshape(nb, 256)


@gpu
@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_diff_histogram_against_numpy(torch_cuda, w):
    for n in SIZES:
        for name, (x, b) in pairs(w, n).items():
            for bs in BLOCKS:
                rc, got = diff_histogram(torch_cuda, w, x, b, bs)
                assert rc == 0, (name, n, bs, rc)
                same(got, X.diff_counts(PR.raw_bytes(x), PR.raw_bytes(b), w, bs), f"w={w} n={n} bs={bs} {name}")


@gpu
@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_diff_histogram_any_alignment_and_no_read_past_the_sources(torch_cuda, w):
    """Each source on its own at every element-aligned offset inside 16
    bytes; whatever lies behind roundup(n * w, 4) -- and the bytes a ragged
    last dword holds behind the source -- is poison that no count may show."""
    torch = torch_cuda
    for n in (17, 4097):
        x, b = pairs(w, n)["small-step"]
        raw_x, raw_b = PR.raw_bytes(x), PR.raw_bytes(b)
        want = {bs: X.diff_counts(raw_x, raw_b, w, bs) for bs in (64, 4096)}
        for off_x in range(0, 16, w):
            for off_b in range(0, 16, w):
                bufs = []
                for raw, off, poison in ((raw_x, off_x, 0xA5), (raw_b, off_b, 0x5A)):
                    host = np.full(16 + len(raw) + 64, poison, dtype=np.uint8)
                    host[off: off + len(raw)] = raw
                    bufs.append(torch.from_numpy(host).cuda())
                for bs in (64, 4096):
                    rc, got = diff_histogram(torch, w, x, b, bs, bufs[0][off_x:], bufs[1][off_b:])
                    assert rc == 0
                    same(got, want[bs], f"w={w} n={n} bs={bs} src+{off_x} base+{off_b}")


@gpu
@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_diff_histogram_of_a_tensor_against_itself(torch_cuda, w):
    """src and base the same pointer: every byte of the image is zero."""
    torch = torch_cuda
    for n in (17, 4097, 70001):
        x, _ = pairs(w, n)["random"]
        src = torch.from_numpy(PR.raw_bytes(x).copy()).cuda()
        for bs in (64, 4096, 65536):
            rc, got = diff_histogram(torch, w, x, x, bs, src, src)
            assert rc == 0
            same(got, X.diff_counts(PR.raw_bytes(x), PR.raw_bytes(x), w, bs), f"w={w} n={n} bs={bs}")
            assert got[:, 1:].sum() == 0 and got[:, 0].sum() == w * PR.stride_of(n)


@gpu
def test_diff_histogram_more_tiles_than_workgroups(torch_cuda):
    """2,048 workgroups at most: 2,052 tiles give them two tiles each and the last ones none."""
    w, n = 2, 2051 * 4096 + 77
    rng = np.random.default_rng(6)
    b = rng.integers(0, 1 << 16, n).astype(D.UINT[w])
    for name, x in (("small-step", b + rng.integers(-40, 41, n).astype(np.int64).astype(D.UINT[w])),
                    ("unrelated", rng.integers(0, 1 << 16, n).astype(D.UINT[w]))):
        rc, got = diff_histogram(torch_cuda, w, x, b, 65536)
        assert rc == 0
        same(got, X.diff_counts(PR.raw_bytes(x), PR.raw_bytes(b), w, 65536), name)


@gpu
def test_python_histogram(torch_cuda):
    torch = torch_cuda
    c = codec_for(block=4096)
    x, b = pairs(4, 5000)["small-step"]
    dx, db = to_dev(torch, x), to_dev(torch, b)
    counts = c.image_histogram(dx, "diff", base=db)
    assert counts.dtype == torch.uint32 and tuple(counts.shape) == (5, 256)
    same(counts.cpu().numpy(), X.diff_counts(PR.raw_bytes(x), PR.raw_bytes(b), 4, 4096), "diff")
    same(c.image_histogram(dx, "delta", base=db).cpu().numpy(), c.image_histogram(dx, "delta").cpu().numpy(), "delta")
    with pytest.raises(ValueError, match="base"):
        c.image_histogram(dx, "diff")
    with pytest.raises(ValueError):
        c.image_histogram(dx, "diff", base=db[:-1])
    with pytest.raises(ValueError):
        c.image_histogram(dx, "diff", base=db.to(torch.int64))


# ---------------------------------------------------------------- fsehip_estimate_base
def estimate_base(torch, codec, x, b, mask):
    """fsehip_estimate_base into five guarded u64: a list of Python ints."""
    from entropy_coders_amd import _lib

    w, n = x.dtype.itemsize, len(x)
    src, base = to_dev(torch, x), to_dev(torch, b)
    need = lib().fsehip_estimate_base_scratch_bytes(n, w, mask, codec.block_size)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    we, est = g64(torch, 5)
    p = codec._frame_params()
    rc = lib().fsehip_estimate_base(C.byref(p), mask, w, ptr(src), ptr(base), n, ptr(scratch), need, ptr(est),
                                    stream_of(torch))
    assert rc == 0, _lib.STATUS[rc]
    torch.cuda.synchronize()
    assert_guards(we, est, F64, f"d_est mask={mask}")
    return [int(v) for v in est.cpu().numpy().view(np.uint64)]


@pytest.fixture(scope="module")
def ten():
    """name -> (x, base, reference estimates) of diff_ref.table_rows at 2^16 elements, 64 KiB blocks."""
    return {name: (a, b, X.estimates5(a, b, 65536, nstates=2, ckpt=64))
            for name, (a, b) in D.table_rows(1 << 16, 1).items()}


def test_host_side_of_the_ten_rows(ten):
    chosen = {name: X.choose5(est) for name, (_, _, est) in ten.items()}
    assert chosen[D.CONTROL] == X.PLANES and set(chosen.values()) == {X.PLANES, X.DIFF}, chosen


@gpu
def test_estimate_base_ten_rows(torch_cuda, ten):
    codec = codec_for()
    for name, (a, b, want) in ten.items():
        assert estimate_base(torch_cuda, codec, a, b, 23) == want, name
        assert codec.estimate(to_dev(torch_cuda, a), base=to_dev(torch_cuda, b)) == named(want), name


@gpu
@pytest.mark.parametrize("nstates,ckpt,table_log,block,row,n", [
    (1, 0, 0, 4096, "int32 table 2% replaced", 20011), (2, 128, 12, 4096, "bf16 master 1e-5", 20011),
    (1, 64, 9, 65536, "fp32 Adam m", 40000)])
def test_estimate_base_other_parameters(torch_cuda, ten, nstates, ckpt, table_log, block, row, n):
    codec = codec_for(block=block, ckpt=ckpt, nstates=nstates, table_log=table_log)
    a, b = ten[row][0][:n], ten[row][1][:n]
    want = X.estimates5(a, b, block, nstates=nstates, ckpt=ckpt, table_log=table_log)
    assert estimate_base(torch_cuda, codec, a, b, 23) == want
    for m in (0, 1):  # the empty containers, and one element
        want = X.estimates5(a[:m], b[:m], block, nstates=nstates, ckpt=ckpt, table_log=table_log)
        assert estimate_base(torch_cuda, codec, a[:m], b[:m], 23) == want
        assert m or want[X.DIFF] == 48


@gpu
@pytest.mark.parametrize("w", [1, 4])
def test_estimate_base_every_mask(torch_cuda, w):
    torch = torch_cuda
    codec = codec_for(block=4096, ckpt=128)
    x, b = pairs(w, 9000)["small-step"]
    x, b = x.view(INT_OF[w]), b.view(INT_OF[w])
    full = X.estimates5(x, b, 4096, nstates=2, ckpt=128)
    assert full[3] == X.NONE and (full[X.PLANES] == X.NONE) == (w == 1)
    src = to_dev(torch, x)
    for mask in MASKS:
        got = estimate_base(torch, codec, x, b, mask)
        assert got == [full[k] if mask >> k & 1 else X.NONE for k in range(5)], mask
        assert got[3] == X.NONE
        if not mask & 16:  # fsehip_estimate's own three
            scratch = torch.empty(max(codec.estimate_scratch_bytes(src), 16), dtype=torch.uint8, device="cuda")
            est3 = torch.zeros(3, dtype=torch.int64, device="cuda")
            p = codec._frame_params()
            assert lib().fsehip_estimate(C.byref(p), mask, w, ptr(src), len(x), ptr(scratch), scratch.numel(),
                                         ptr(est3), stream_of(torch)) == 0
            assert [int(v) for v in est3.cpu().numpy().view(np.uint64)] == got[:3], mask


# ---------------------------------------------------------------- the choice, compressed
@gpu
def test_compress_auto_ten_rows(torch_cuda, ten):
    """The reference's kind, the direct call's bytes, and the way back."""
    from entropy_coders_amd import container_kind

    torch = torch_cuda
    codec = codec_for()
    for name, (a, b, want) in ten.items():
        x, base = to_dev(torch, a), to_dev(torch, b)
        direct = {"frame": lambda: codec.compress_frame(x.view(torch.uint8)), "planes": lambda: codec.compress_planes(x),
                  "delta": lambda: codec.compress_delta(x), "diff": lambda: codec.compress_diff(x, base)}
        buf, kind = codec.compress_auto(x, base=base)
        assert kind == X.NAMES[X.choose5(want)], (name, kind, want)
        assert container_kind(buf) == kind
        same(buf.cpu().numpy(), direct[kind]().cpu().numpy(), f"{name}: compress_auto against compress_{kind}")
        out, status = codec.decompress_auto(buf, x.dtype, base=base)
        assert not bool(status.any()) and torch.equal(out, x), name


@gpu
def test_compress_auto_without_a_base_is_unchanged(torch_cuda, ten):
    torch = torch_cuda
    codec = codec_for()
    for name in ("bf16 master 1e-5", "int8 weights 1e-4", D.CONTROL):
        a, b, want = ten[name]
        x, base = to_dev(torch, a), to_dev(torch, b)
        buf, kind = codec.compress_auto(x)
        buf3, kind3 = codec.compress_auto(x, kinds=("frame", "planes", "delta"), base=base)
        assert kind == kind3 == E.NAMES[E.choose(want[:3])] != "diff", name
        same(buf.cpu().numpy(), buf3.cpu().numpy(), name)
        assert codec.estimate(x) == codec.estimate(x, kinds=("frame", "planes", "delta"), base=base) == named(want[:3])


@gpu
def test_python_errors(torch_cuda):
    torch = torch_cuda
    codec = codec_for(block=4096)
    x, b = pairs(4, 5000)["small-step"]
    dx, db = to_dev(torch, x), to_dev(torch, b)
    for call in (codec.estimate, codec.estimate_scratch_bytes, codec.compress_auto):
        with pytest.raises(ValueError, match="base"):
            call(dx, kinds=["delta", "diff"])  # "diff" without a base
        with pytest.raises(ValueError):
            call(dx, base=db[:-1])  # another element count
        with pytest.raises(ValueError):
            call(dx, base=db.to(torch.int16))  # another width
        with pytest.raises(ValueError):
            call(dx, base=torch.stack([db, db], 1)[:, 0])  # not contiguous
        with pytest.raises(ValueError):
            call(dx, base=b)  # not a device tensor
        with pytest.raises(ValueError):
            call(dx, kinds=[3], base=db)
    est = torch.zeros(3, dtype=torch.int64, device="cuda")
    scratch = torch.empty(codec.estimate_scratch_bytes(dx, base=db), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        codec.estimate_into(dx, scratch, est, base=db)  # five int64
    assert set(codec.estimate(dx, base=db)) == {"frame", "planes", "delta", "diff"}
    assert codec.estimate(dx, kinds=["diff"], base=db) == {"diff": codec.estimate(dx, base=db)["diff"]}
    assert codec.estimate(dx, kinds=[4, 0], base=db).keys() == {"frame", "diff"}
    with pytest.raises(ValueError):  # compress_diff's own rule: the base has x's dtype
        codec.compress_auto(dx, base=db.view(torch.float32))


@gpu
@pytest.mark.parametrize("w", [1, 2, 4])
def test_sealed_auto(torch_cuda, ten, w):
    """kind='auto' seals the chosen kind: the bytes of compress_sealed of that
    kind, the round trip, and a wrong base named by exactly one check block."""
    from entropy_coders_amd import BlockCodec

    torch = torch_cuda
    codec = codec_for()
    near = {1: "int8 weights 1e-4", 2: "bf16 master 1e-5", 4: "int32 table 2% replaced"}[w]
    far = {1: None, 2: D.CONTROL, 4: None}[w]
    for name in (near, far):
        if name is None:
            continue
        a, b, want = ten[name]
        x, base = to_dev(torch, a), to_dev(torch, b)
        cands = (X.FRAME if w == 1 else X.PLANES, X.DELTA)
        for use_base in (True, False):
            kinds = cands + ((X.DIFF,) if use_base else ())
            chosen = X.NAMES[X.choose5([v if k in kinds else X.NONE for k, v in enumerate(want)])]
            buf = codec.compress_sealed(x, kind="auto", base=base if use_base else None)
            info, kind, off = BlockCodec.sealed_info(buf)
            assert kind == chosen, (name, use_base, kind, want)
            kb = base if kind == "diff" else None
            same(buf.cpu().numpy(), codec.compress_sealed(x, kind=kind, base=kb).cpu().numpy(), f"{name} sealed {kind}")
            assert buf.numel() <= codec.sealed_bound(x, "auto")
            out, st, cs, res = codec.decompress_sealed(buf, x.dtype, base=kb, with_result=True)
            assert torch.equal(out, x) and not bool(st.any()) and not bool(cs.any()) and res.tolist() == [0, 0]
            if kind == "diff":
                e = 9001
                wrong = base.clone()
                wrong[e] += 1
                out, st, cs, res = codec.decompress_sealed(buf, x.dtype, base=wrong, with_result=True)
                assert not bool(st.any())
                assert cs.tolist() == [CHECKSUM if i == e * w // 65536 else 0 for i in range(info.n_cb)]
                assert res.tolist() == [CHECKSUM, 1]
        assert X.NAMES[X.choose5(want)] == ("diff" if name == near else "planes")
    assert codec.sealed_bound(x, "auto") == max(codec.sealed_bound(x, k) for k in
                                                 (("frame",) if w == 1 else ("planes",)) + ("delta", "diff"))
    with pytest.raises(ValueError):
        codec.compress_sealed(x, kind="auto", base=base[:-1])


@gpu
def test_host_helpers(torch_cuda, ten):
    from entropy_coders_amd import (BlockCodec, auto_compress, auto_decompress, container_kind, sealed_compress,
                                    sealed_decompress)

    n = 20011
    for name, dtype in (("int8 weights 1e-4", np.int8), ("bf16 master 1e-4", np.uint16),
                        ("fp32 master 1e-5", np.float32), (D.CONTROL, np.int16)):
        a, b = ten[name][0][:n].view(dtype), ten[name][1][:n].view(dtype)
        want = X.estimates5(ten[name][0][:n], ten[name][1][:n], 4096, nstates=2, ckpt=128)
        blob, kind = auto_compress(a, block_size=4096, base=b)
        assert kind == X.NAMES[X.choose5(want)] == container_kind(blob), (name, kind, want)
        assert auto_decompress(blob, dtype, base=b).tobytes() == a.tobytes()
        blob3, kind3 = auto_compress(a, block_size=4096)
        assert kind3 == E.NAMES[E.choose(want[:3])]
        cands = (X.FRAME if a.dtype.itemsize == 1 else X.PLANES, X.DELTA, X.DIFF)  # what a sealed buffer chooses among
        skind = X.NAMES[X.choose5([v if k in cands else X.NONE for k, v in enumerate(want)])]
        sealed = sealed_compress(a, kind="auto", block_size=4096, base=b)
        assert BlockCodec.sealed_info(sealed)[1] == skind, (name, skind, want)
        assert sealed == sealed_compress(a, kind=skind, block_size=4096, base=b if skind == "diff" else None)
        back = sealed_decompress(sealed, dtype, base=b if skind == "diff" else None)
        assert np.asarray(back).tobytes() == a.tobytes()
    x64 = np.cumsum(np.random.default_rng(8).integers(0, 9, 5000)).astype(np.int64)
    blob, kind = auto_compress(x64, block_size=4096, base=x64 - 1)
    assert kind == "diff" and auto_decompress(blob, np.int64, base=x64 - 1).tobytes() == x64.tobytes()
    with pytest.raises(ValueError):
        auto_compress(x64, base=x64[:-1])
    with pytest.raises(ValueError):
        auto_compress(x64, base=x64.astype(np.int32))


# ---------------------------------------------------------------- stream order
class EstimateBaseChain(Chain):
    """The copies of x and of the base, the diff histogram and estimate_into
    with a base on one stream with no host synchronisation, inputs poison
    until the gate opens."""

    N = 5 * 4096 + 333
    W = 4
    BLOCK = 4096

    def __init__(self):
        rng = np.random.default_rng(0xE5D)
        self.base = rng.integers(0, 1 << 20, self.N).astype(np.int32)
        self.ints = self.base + rng.integers(-30, 31, self.N).astype(np.int32)
        self.counts = X.diff_counts(PR.raw_bytes(self.ints), PR.raw_bytes(self.base), self.W, self.BLOCK)
        self.est = X.estimates5(self.ints, self.base, self.BLOCK, nstates=2, ckpt=128)

    def alloc(self, torch):
        self.torch = torch
        c = self.codec = codec_for(block=self.BLOCK, ckpt=128)
        self.src = torch.empty(self.N, dtype=torch.int32, device="cuda")
        self.d_base = torch.empty(self.N, dtype=torch.int32, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.ints)), (self.d_base, pinned(torch, self.base))]
        self.w_cnt, self.cnt = g32(torch, len(self.counts) * 256)
        self.w_est, self.est_d = g64(torch, 5)
        self.scratch = torch.empty(c.estimate_scratch_bytes(self.src, base=self.d_base), dtype=torch.uint8,
                                   device="cuda")

    def poison(self):
        self.src.fill_(7)
        self.d_base.fill_(-9)
        self.cnt.fill_(F32)
        self.est_d.fill_(F64)

    def enqueue(self, step9):
        c, s = self.codec, stream_of(self.torch)
        assert c.lib.fsehip_diff_image_histogram(self.W, ptr(self.src), ptr(self.d_base), self.N, self.BLOCK,
                                                 ptr(self.cnt), s) == 0
        c.estimate_into(self.src, self.scratch, self.est_d, base=self.d_base)
        step9()

    def check(self):
        assert_guards(self.w_cnt, self.cnt, F32, "d_counts")
        assert_guards(self.w_est, self.est_d, F64, "d_est")
        same(self.cnt.cpu().numpy().view(np.uint32).reshape(-1, 256), self.counts, "counts")
        assert [int(v) for v in self.est_d.cpu().numpy().view(np.uint64)] == self.est


def test_host_side_of_the_estimate_base_chain():
    chain = EstimateBaseChain()
    assert X.choose5(chain.est) == X.DIFF and chain.est[3] == X.NONE and X.NONE not in chain.est[:3]


@gpu
def test_estimate_base_chain_behind_the_gate(torch_cuda, warm):
    """Poison, then the copies of the real x and base, then the histogram and
    estimate_into on a side stream behind the gate: both calls return while
    their inputs are still poison, and the five totals are the reference's."""
    chain = EstimateBaseChain()
    chain.alloc(torch_cuda)
    warm.chains["estimate-base"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code
    warm.enqueue_ms["estimate-base"] = warm.run(chain, gated=False)
    behind_gate(warm, "estimate-base")
