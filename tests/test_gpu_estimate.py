"""The size estimate on the GPU (include/fsehip.h section 2g) against
tests/estimate_ref.py: the image histograms between guard bands, the per-block
estimate, the container estimates, compress_auto / decompress_auto, and the
whole chain behind the gate of tests/test_gpu_stream_order.py.  Shapes are the
smallest at which the kernels can go wrong: ragged groups, restart and tile
edges, plane starts inside blocks, blocks below and above one 4,096-byte tile
(the histogram's two paths), more tiles than one workgroup takes."""
import ctypes as C

import numpy as np
import pytest

import caller_cases as CC
import delta_ref as DR
import estimate_ref as E
import frame_ref as R
import planes_ref as PR
from oracle import oracle as O
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr
from test_gpu_stream_order import Chain, behind_gate, pinned, same, warm  # noqa: F401  (warm: the fixture)

gpu = pytest.mark.gpu

F32, F64 = FILL["int32"], FILL["int64"]
INT_OF = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8207, 70001]
# 64 and 1040: several blocks per tile (the direct path); 4096 and 4112: a tile in two blocks, aligned to the
# planes and not; 65536: the product's, plane starts inside blocks
BLOCKS = [64, 1040, 4096, 4112, 65536]
KIND_W = [(k, w) for k in (E.PLANES, E.DELTA) for w in (1, 2, 4, 8)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def codec_for(block=65536, ckpt=64, nstates=2, table_log=0):
    from entropy_coders_amd import BlockCodec

    return BlockCodec(block_size=block, table_log=table_log, ckpt_interval=ckpt, nstates=nstates)


def lib():
    from entropy_coders_amd import _lib

    return _lib.load()


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_dev(torch, a):
    """A numpy array of any integer dtype on the device, as the integer tensor of its width."""
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(INT_OF[a.dtype.itemsize]).copy()).cuda()


def host_u8(torch, t):
    """A device tensor's bytes as a host uint8 array (an empty tensor has no stride to view through)."""
    return t.reshape(-1).view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8)


def patterns(w, n):
    """name -> n unsigned w-byte integers."""
    rng = np.random.default_rng(0xE571 + 16 * w + n)
    u = DR.UINT[w]
    top = (1 << (8 * w)) - 1
    i = np.arange(n, dtype=np.uint64)
    return {
        "random": np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=u),
        "zeros": np.zeros(n, dtype=u),
        "small": rng.integers(0, 200, n).astype(u),  # every plane above the first is zero
        # a rising ramp: for 8 bytes across 2^32 (the borrow between the halves), for the others through the wrap
        "ramp": ((np.uint64(0xFFFFFF00) + i * np.uint64(977)) & np.uint64(top)).astype(u),
        "wrap": np.where(i % 2 == 0, np.uint64(top), np.uint64(0)).astype(u),  # deltas of -1 and +1 mod 2^(8 w)
    }


# ---------------------------------------------------------------- the image histogram
def image_histogram(torch, kind, w, x, bs):
    """fsehip_image_histogram into guarded counts: (rc, counts as uint32 [n_blocks, 256])."""
    raw = PR.raw_bytes(x)
    n_image = w * PR.stride_of(len(x)) if kind else len(raw)
    nb = R.n_blocks_of(n_image, bs)
    src = torch.from_numpy(raw.copy()).cuda()
    wc, counts = g32(torch, nb * 256)
    rc = lib().fsehip_image_histogram(kind, w, ptr(src), len(x), bs, ptr(counts), stream_of(torch))
    torch.cuda.synchronize()
    assert_guards(wc, counts, F32, f"kind={kind} w={w} n={len(x)} bs={bs}")
    return rc, counts.cpu().numpy().view(np.uint32).reshape(nb, 256)


@gpu
@pytest.mark.parametrize("kind,w", KIND_W)
def test_image_histogram_against_numpy(torch_cuda, kind, w):
    if kind == E.PLANES and w == 1:  # the plane frame has no 1-byte form
        rc, _ = image_histogram(torch_cuda, kind, w, np.zeros(100, np.uint8), 64)
        assert lib().fsehip_estimate_image_bytes(kind, 100, 1) == 0
        from entropy_coders_amd import _lib
        assert _lib.STATUS[rc] == "UNSUPPORTED"
        return
    for n in SIZES:
        for name, x in patterns(w, n).items():
            raw = PR.raw_bytes(x)
            for bs in BLOCKS:
                rc, got = image_histogram(torch_cuda, kind, w, x, bs)
                assert rc == 0, (name, n, bs, rc)
                same(got, E.image_counts(raw, w, kind, bs), f"{E.NAMES[kind]} w={w} n={n} bs={bs} {name}")


@gpu
@pytest.mark.parametrize("w", [2])
def test_image_histogram_more_tiles_than_workgroups(torch_cuda, w):
    """2,048 workgroups at most: 2,052 tiles give them two tiles each and the last ones none."""
    n = 2051 * DR.RESTART + 77
    x = (np.cumsum(np.random.default_rng(5).integers(0, 1 << 20, n)).astype(np.uint64) & np.uint64((1 << 8 * w) - 1))
    x = x.astype(DR.UINT[w])
    for kind in (E.PLANES, E.DELTA):
        rc, got = image_histogram(torch_cuda, kind, w, x, 65536)
        assert rc == 0
        same(got, E.image_counts(PR.raw_bytes(x), w, kind, 65536), f"{E.NAMES[kind]} w={w}")


@gpu
@pytest.mark.parametrize("w", [1, 4])
def test_frame_kind_is_histogram_blocks(torch_cuda, w):
    torch = torch_cuda
    for n in (1, 17, 4097, 70001):
        x = patterns(w, n)["random"]
        raw = PR.raw_bytes(x)
        for bs in (64, 65536):
            rc, got = image_histogram(torch, E.FRAME, w, x, bs)
            assert rc == 0
            nb = R.n_blocks_of(len(raw), bs)
            src = torch.from_numpy(raw.copy()).cuda()
            ref = torch.zeros(nb * 256, dtype=torch.int32, device="cuda")
            assert lib().fsehip_histogram_blocks(ptr(src), len(raw), bs, ptr(ref), None, stream_of(torch)) == 0
            same(got.reshape(-1), ref.cpu().numpy().view(np.uint32), f"frame w={w} n={n} bs={bs}")
            same(got, E.image_counts(raw, w, E.FRAME, bs), f"frame w={w} n={n} bs={bs} against numpy")


@gpu
def test_python_histogram_shape_and_errors(torch_cuda):
    torch = torch_cuda
    c = codec_for(block=4096)
    x = to_dev(torch, patterns(4, 5000)["small"])
    for kind in ("frame", "planes", "delta"):
        counts = c.image_histogram(x, kind)
        assert counts.dtype == torch.uint32 and tuple(counts.shape) == (5, 256)
        raw = PR.raw_bytes(x.cpu().numpy())
        k = ("frame", "planes", "delta").index(kind)
        same(counts.cpu().numpy(), E.image_counts(raw, 4, k, 4096), kind)
    with pytest.raises(ValueError):
        c.image_histogram(x, "auto")
    with pytest.raises(ValueError):
        c.image_histogram(torch.zeros((4, 4), dtype=torch.int32, device="cuda").t(), "delta")
    from entropy_coders_amd import FseError
    with pytest.raises(FseError) as e:
        c.image_histogram(torch.zeros(100, dtype=torch.uint8, device="cuda"), "planes")
    assert e.value.code == "UNSUPPORTED"


# ---------------------------------------------------------------- the per-block estimate
def block_images():
    """name -> (image bytes, block size)."""
    rng = np.random.default_rng(0xB10C)
    rle, raw = np.zeros(4096, np.uint8), rng.integers(0, 256, 4096, dtype=np.uint8)
    fse = O.generate(0, 0.155, 7, 0, 4096)
    out = {"rle-raw-fse": (np.concatenate([rle, raw, fse]), 4096)}
    for tail in (1, 2, 17):
        out[f"tail-{tail}"] = (np.concatenate([fse, rle, rng.integers(0, 3, tail, dtype=np.uint8) + 1]), 4096)
    out["tail-1-zero"] = (np.concatenate([raw, np.zeros(1, np.uint8)]), 4096)
    out["single-symbol"] = (np.full(4096, 9, np.uint8), 4096)
    out["corpus"] = (R.corpus(1000), R.BLOCK)
    out["lut-64k"] = (np.concatenate([O.generate(0, p, 3, b, 65536) for b, p in enumerate((0.05, 0.5, 0.77))]), 65536)
    return out


def run_estimate_blocks(torch, codec, counts, n_image):
    d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).cuda()
    out = codec.estimate_blocks(d, n_image)
    torch.cuda.synchronize()
    got = list(zip(out["type"].tolist(), out["rec"].tolist(), out["bits"].tolist(), out["log"].tolist()))
    return got, int(out["total"].item())


@gpu
@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("ckpt", [0, 64])
@pytest.mark.parametrize("table_log", [0, 9, 12, 13])
def test_estimate_blocks_against_the_reference(torch_cuda, table_log, ckpt, nstates):
    seen = set()
    for name, (img, bs) in block_images().items():
        codec = codec_for(block=bs, ckpt=ckpt, nstates=nstates, table_log=table_log)
        counts = E.counts_of(img, bs)
        want = E.block_estimates(counts, img.size, bs, nstates=nstates, ckpt=ckpt, table_log=table_log)
        got, total = run_estimate_blocks(torch_cuda, codec, counts, img.size)
        assert got == want, (name, got, want)
        assert total == 32 + 4 * len(want) + sum(e[1] for e in want) == E.frame_estimate(
            counts, img.size, bs, nstates=nstates, ckpt=ckpt, table_log=table_log), name
        seen |= {e[0] for e in want}
        if name == "rle-raw-fse":
            assert [e[0] for e in want] == [R.RLE, R.RAW, R.FSE]
    assert seen == {R.RAW, R.RLE, R.FSE}


@gpu
@pytest.mark.parametrize("nstates", [2, 1])
def test_estimate_blocks_caller_counts_on_the_slow_path(torch_cuda, nstates):
    """Count arrays no sampled block gives (tests/caller_cases.py): the ones
    whose normalisation leaves the fast path, at their own table log."""
    cases = [c for c in CC.HIST_CASES if c[5].startswith("slow") and CC.consistent(c) and 2 <= c[2] <= 1 << 28]
    assert any(c[0] == "slow_prop_search" for c in cases) and len(cases) >= 4
    for name, counts, size, tl, log2, label in cases:
        bs = (size + 15) // 16 * 16
        codec = codec_for(block=bs, ckpt=64, nstates=nstates, table_log=log2)
        want = [E.block_estimate(counts, size, nstates=nstates, ckpt=64, table_log=log2)]
        got, total = run_estimate_blocks(torch_cuda, codec, np.asarray(counts, np.uint32).reshape(1, 256), size)
        assert got == want, (name, label, got, want)
        assert total == 36 + want[0][1]


@gpu
def test_estimate_blocks_kernel_class_and_null_outputs(torch_cuda):
    """A table log above the kernel class is stored RAW, as the encoder's
    UNSUPPORTED blocks are; every per-block output may be null."""
    from entropy_coders_amd import _lib

    torch = torch_cuda
    img = O.generate(0, 0.155, 7, 0, 8192)
    counts = E.counts_of(img, 4096)
    d = torch.from_numpy(counts.view(np.int32)).cuda()
    for lmax, want_type in ((13, R.FSE), (12, R.RAW)):
        p = _lib.FrameParams(4096, 13, 0, lmax, 2, 0)
        wt, total = g64(torch, 1)
        typ = torch.zeros(2, dtype=torch.uint8, device="cuda")
        assert lib().fsehip_estimate_blocks(C.byref(p), ptr(d), 8192, ptr(typ), None, None, None, ptr(total),
                                            stream_of(torch)) == 0
        torch.cuda.synchronize()
        assert_guards(wt, total, F64, "d_total")
        want = E.block_estimates(counts, 8192, 4096, table_log=13, max_table_log=lmax)
        assert typ.tolist() == [e[0] for e in want] == [want_type] * 2
        assert total.item() == 40 + sum(e[1] for e in want)
        assert lib().fsehip_estimate_blocks(C.byref(p), ptr(d), 8192, None, None, None, None, ptr(total),
                                            stream_of(torch)) == 0
        torch.cuda.synchronize()
        assert total.item() == 40 + sum(e[1] for e in want)


# ---------------------------------------------------------------- the container estimates and the choice
@pytest.fixture(scope="module")
def six():
    """name -> (array, reference estimates) of the six tensors at 2^16 elements, 64 KiB blocks."""
    return {name: (a, E.container_estimates(a, 65536, nstates=2, ckpt=64))
            for name, a in E.six_tensors(1 << 16).items()}


def named(est):
    return {E.NAMES[k]: v for k, v in est.items() if v != E.NONE}


@gpu
def test_estimate_six_tensors(torch_cuda, six):
    codec = codec_for()
    for name, (a, want) in six.items():
        assert codec.estimate(to_dev(torch_cuda, a)) == named(want), name


@gpu
@pytest.mark.parametrize("nstates,ckpt,table_log,block", [(1, 0, 0, 4096), (2, 128, 12, 4096), (1, 64, 9, 65536)])
def test_estimate_other_parameters_and_sizes(torch_cuda, nstates, ckpt, table_log, block):
    codec = codec_for(block=block, ckpt=ckpt, nstates=nstates, table_log=table_log)
    for w, n in ((1, 0), (4, 0), (1, 5000), (2, 4097), (8, 9000), (4, 1)):
        x = patterns(w, n)["small" if n % 2 else "ramp"]
        want = E.container_estimates(x, block, nstates=nstates, ckpt=ckpt, table_log=table_log)
        assert codec.estimate(to_dev(torch_cuda, x)) == named(want), (w, n)


@gpu
def test_compress_auto_six_tensors(torch_cuda, six):
    """The reference's kind, the direct call's bytes, and the way back."""
    from entropy_coders_amd import container_kind

    codec = codec_for()
    direct = {"frame": lambda x: codec.compress_frame(x.view(torch_cuda.uint8)), "planes": codec.compress_planes,
              "delta": codec.compress_delta}
    for name, (a, want) in six.items():
        x = to_dev(torch_cuda, a)
        buf, kind = codec.compress_auto(x)
        assert kind == E.NAMES[E.choose(want)], (name, kind, want)
        assert container_kind(buf) == kind
        same(buf.cpu().numpy(), direct[kind](x).cpu().numpy(), f"{name}: compress_auto against compress_{kind}")
        out, status = codec.decompress_auto(buf, x.dtype)
        assert not bool(status.any()) and bool((out == x).all()), name


@gpu
@pytest.mark.parametrize("dtype", ["int16", "int32", "int64", "bfloat16", "float32", "uint8"])
def test_auto_round_trip_dtypes(torch_cuda, dtype):
    torch = torch_cuda
    td = getattr(torch, dtype)
    w = torch.empty(0, dtype=td).element_size()
    codec = codec_for(block=4096, ckpt=128)
    rng = np.random.default_rng(0xD7 + w)
    for n in (0, 1, 4097, 20011):
        if dtype in ("bfloat16", "float32"):
            x = torch.from_numpy((rng.standard_normal(n) * 0.02).astype(np.float32)).cuda().to(td)
        else:
            x = to_dev(torch, np.cumsum(rng.integers(-3, 40, n)).astype(INT_OF[w])).view(td)
        raw = host_u8(torch, x)
        want = E.container_estimates(raw.view(INT_OF[w]), 4096, nstates=2, ckpt=128)
        buf, kind = codec.compress_auto(x)
        assert kind == E.NAMES[E.choose(want)], (n, kind, want)
        assert w > 1 or kind != "planes"
        out, status = codec.decompress_auto(buf, td)
        assert out.dtype == td and out.numel() == n and not bool(status.any())
        same(host_u8(torch, out), raw, f"{dtype} n={n} through {kind}")


@gpu
def test_kind_masks_and_width_one(torch_cuda):
    from entropy_coders_amd import _lib

    torch = torch_cuda
    codec = codec_for(block=4096, ckpt=128)
    x8 = to_dev(torch, (np.arange(9000) // 7 % 251).astype(np.uint8))
    est = codec.estimate(x8)
    assert set(est) == {"frame", "delta"}  # width 1 never has a plane estimate
    assert codec.estimate(x8, kinds=["planes", "delta"]) == {"delta": est["delta"]}
    with pytest.raises(ValueError):
        codec.compress_auto(x8, kinds=["planes"])
    x = to_dev(torch, np.cumsum(np.random.default_rng(3).integers(0, 9, 9000)).astype(np.int32))
    full = codec.estimate(x)
    assert set(full) == {"frame", "planes", "delta"} and min(full, key=full.get) == "delta"
    for kinds in (["frame"], ["planes"], ["frame", "planes"], [0, 2], ["delta", "planes"]):
        names = {_lib.KINDS[k] if isinstance(k, int) else k for k in kinds}
        sub = codec.estimate(x, kinds=kinds)
        assert sub == {k: full[k] for k in names}, kinds
        buf, kind = codec.compress_auto(x, kinds=kinds)
        assert kind == min(sorted(names, key=_lib.KINDS.index), key=sub.get), kinds
        out, _ = codec.decompress_auto(buf, torch.int32)
        assert bool((out == x).all())
    with pytest.raises(ValueError):
        codec.estimate(x, kinds=[])


@gpu
def test_host_helpers(torch_cuda):
    from entropy_coders_amd import auto_compress, auto_decompress, container_kind

    def want(a, kinds=E.KINDS):
        return E.NAMES[E.choose(E.container_estimates(a, 4096, kinds=kinds, nstates=2, ckpt=128))]

    ids = np.cumsum(np.random.default_rng(1).geometric(1 / 1000, 5000)).astype(np.int64)
    blob, kind = auto_compress(ids, block_size=4096)
    assert kind == want(ids) == "delta" and container_kind(blob) == "delta"
    assert auto_decompress(blob, np.int64).tobytes() == ids.tobytes()
    noise = np.random.default_rng(2).integers(0, 256, 5000, dtype=np.uint8)
    blob, kind = auto_compress(noise, block_size=4096)
    assert kind == want(noise) == "frame" and auto_decompress(blob, np.uint8).tobytes() == noise.tobytes()
    bf = E.bf16_weights(5000)
    blob, kind = auto_compress(bf, kinds=["planes", "delta"], block_size=4096)
    assert kind == want(bf, (E.PLANES, E.DELTA)) != "frame" and container_kind(blob) == kind
    assert auto_decompress(blob, np.uint16).tobytes() == bf.tobytes()


# ---------------------------------------------------------------- stream order
class EstimateChain(Chain):
    """image histogram -> per-block estimate -> the three container estimates
    on one stream with no host synchronisation, inputs poison until the gate
    opens."""

    N = 5 * DR.RESTART + 333
    W = 4
    BLOCK = 4096

    def __init__(self):
        rng = np.random.default_rng(0xE5)
        self.ints = np.cumsum(rng.integers(0, 50, self.N)).astype(np.int32)
        raw = PR.raw_bytes(self.ints)
        self.counts = E.image_counts(raw, self.W, E.DELTA, self.BLOCK)
        self.n_image = self.W * PR.stride_of(self.N)
        self.blocks = E.block_estimates(self.counts, self.n_image, self.BLOCK, nstates=2, ckpt=128)
        self.est = E.container_estimates(self.ints, self.BLOCK, nstates=2, ckpt=128)

    def alloc(self, torch):
        self.torch = torch
        c = self.codec = codec_for(block=self.BLOCK, ckpt=128)
        nb = len(self.counts)
        self.src = torch.empty(self.N, dtype=torch.int32, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.ints))]
        self.w_cnt, self.cnt = g32(torch, nb * 256)
        self.w_typ, self.typ = g8(torch, nb)
        self.w_rec, self.rec = g32(torch, nb)
        self.w_bits, self.bits = g32(torch, nb)
        self.w_log, self.log = g8(torch, nb)
        self.w_tot, self.tot = g64(torch, 1)
        self.w_est, self.est_d = g64(torch, 3)
        self.scratch = torch.empty(c.estimate_scratch_bytes(self.src), dtype=torch.uint8, device="cuda")

    def poison(self):
        self.src.fill_(7)
        for t in (self.cnt, self.rec, self.bits):
            t.fill_(F32)
        for t in (self.typ, self.log):
            t.fill_(FILL["uint8"])
        for t in (self.tot, self.est_d):
            t.fill_(F64)

    def enqueue(self, step9):
        c, s = self.codec, stream_of(self.torch)
        assert c.lib.fsehip_image_histogram(E.DELTA, self.W, ptr(self.src), self.N, self.BLOCK, ptr(self.cnt), s) == 0
        p = c._frame_params()
        assert c.lib.fsehip_estimate_blocks(C.byref(p), ptr(self.cnt), self.n_image, ptr(self.typ), ptr(self.rec),
                                            ptr(self.bits), ptr(self.log), ptr(self.tot), s) == 0
        c.estimate_into(self.src, self.scratch, self.est_d)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_cnt, self.cnt, F32, "d_counts"), (self.w_typ, self.typ, FILL["uint8"], "d_type"),
                              (self.w_rec, self.rec, F32, "d_rec"), (self.w_bits, self.bits, F32, "d_bits"),
                              (self.w_log, self.log, FILL["uint8"], "d_log"), (self.w_tot, self.tot, F64, "d_total"),
                              (self.w_est, self.est_d, F64, "d_est")):
            assert_guards(w, v, f, name)
        same(self.cnt.cpu().numpy().view(np.uint32).reshape(-1, 256), self.counts, "counts")
        got = list(zip(self.typ.tolist(), self.rec.tolist(), self.bits.tolist(), self.log.tolist()))
        assert got == self.blocks
        assert self.tot.tolist() == [32 + 4 * len(self.blocks) + sum(e[1] for e in self.blocks)]
        assert self.est_d.tolist() == [self.est[k] for k in E.KINDS]


def test_host_side_of_the_estimate_chain():
    chain = EstimateChain()
    assert R.FSE in {e[0] for e in chain.blocks} and E.choose(chain.est) == E.DELTA
    assert chain.est[E.DELTA] == 16 + 32 + 4 * len(chain.blocks) + sum(e[1] for e in chain.blocks)


@gpu
def test_estimate_chain_behind_the_gate(torch_cuda, warm):
    """The histogram -> estimate_blocks -> estimate chain behind the gate of
    tests/test_gpu_stream_order.py: every call returns while its input is
    still poison, so none of them waits for the stream or reads device data
    on the host."""
    chain = EstimateChain()
    chain.alloc(torch_cuda)
    warm.chains["estimate"] = chain
    warm.run(chain, gated=False)  # the first call of a kernel loads its code
    warm.enqueue_ms["estimate"] = warm.run(chain, gated=False)
    behind_gate(warm, "estimate")
